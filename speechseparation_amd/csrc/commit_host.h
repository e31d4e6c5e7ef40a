// The committed weight image: everything bsrnn_commit_params puts on the device, built on the host from the parameters, the band
// table and a few knobs.  Host arithmetic only (api.hip uploads the result), so tests run it without a GPU
// (tests/test_weight_image.py).  The operand layouts the kernels read are defined here and in split_host.h.
#pragma once
#include "descriptors.h"
#include "split_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>

namespace bsrnn {

// layer slots of the per-layer flow: one grouped launch each (the ten Linear layers of the bands, the fc of the four blocks)
enum Slot { PRE0, PRE2, FC0, FC2, FC4, BACK0, BACK2, BACK4, POST0, POST2, BLK_FC0, BLK_FC1, BLK_FC2, BLK_FC3, NSLOT };

inline int imax(int a, int b) { return a > b ? a : b; }
inline int round8(int a) { return (a + 7) & ~7; }

// Column layout of the rows the Linear layers work on: band i starts at aoff[i] in an activation row of LDA floats and at poff[i] in a
// band-padded spectrum row of LDP floats
struct BandColumns { std::vector<int> aoff, poff; int LDA, LDP; };
inline BandColumns band_columns(const std::vector<int>& widths)
{
    BandColumns bc;
    int ao = 0, po = 0;
    for (int w : widths) {
        // 32-column granularity: the same per-band offsets (x 2, in 16-bit elements) address the slab-format activations,
        // whose bands are padded to whole 32-deep slabs
        bc.aoff.push_back(ao); ao += (imax(2 * w, 2 * HID) + 31) & ~31;
        bc.poff.push_back(po); po += round8(2 * w);
    }
    bc.LDA = ao; bc.LDP = imax(po, 8);
    return bc;
}

// a parameter's values by its state_dict key (every key of the inventory is present: commit checks that first)
using ParamLookup = std::function<const std::vector<float>&(const std::string&)>;

// Everything the image depends on besides the parameters and the band table (api.hip reads the environment)
struct CommitKnobs {
    int gemm_mode;       // GemmMode
    bool mlp_layers;     // BSRNN_MLP=layers: no fused chains
    bool no48, no80;     // BSRNN_CHAIN_NO48 / BSRNN_CHAIN_NO80: keep the bands of those classes on the 32 x 32 geometry
    bool rag;            // the ragged split (off: BSRNN_CHAIN_RAG=0)
};

// ------------------------------------------------------------------ geometry of one band's fused chain
struct LayerDims { const char* fmt; int N, Kd, leaky; };      // key format of the Linear layer, its output and input widths
struct ChainGeometry {
    bool fits;           // false: the band is too wide for the fused kernel (the whole model takes the per-layer flow)
    bool g48;            // the 16 x 16 x 32 geometries (48, 64 or 80 rows)
    long cost;           // k-steps x feature tiles over the layers: the order of the bands inside a class
    ChainDesc d;         // the geometry fields only: L[].K16 / NTL / bias_off / leaky / rag, RT, NW, plane_units, nbias, zpad
};
inline ChainGeometry chain_geometry(const LayerDims ld[CHAIN_LAYERS], const CommitKnobs& kn)
{
    ChainGeometry g;
    memset(&g, 0, sizeof g);
    ChainDesc& d = g.d;
    int units = 0, maxntl = 0, nbias = 0;
    long cost = 0;
    for (int l = 0; l < CHAIN_LAYERS; ++l) {
        d.L[l].K16 = (ld[l].Kd + 15) / 16; d.L[l].NTL = (ld[l].N + 31) / 32; d.L[l].leaky = ld[l].leaky;
        d.L[l].bias_off = nbias; nbias += 32 * d.L[l].NTL;
        units = imax(units, 2 * d.L[l].K16);
        if (l + 1 < CHAIN_LAYERS) units = imax(units, 4 * d.L[l].NTL);
        maxntl = imax(maxntl, d.L[l].NTL);
        cost += (long)d.L[l].K16 * d.L[l].NTL;
    }
    const int img = 2 * units * 512;                                  // bytes of one row tile's image (both pieces)
    // geometry (mlp_chain.hip): RT row tiles per wave group (each weight fragment is used for all of them), GR groups
    int RT = 0, GR = 1;
    if (8 * img <= CHAIN_LDS_EX && maxntl <= 4) { RT = 1; GR = 8; }          // narrowest: every wave a chain of its own
    else if (4 * img <= CHAIN_LDS_EX && maxntl <= 6) { RT = 1; GR = 4; }     // narrow: four groups of two waves
    else if (4 * img <= CHAIN_LDS_EX && maxntl <= 12) { RT = 2; GR = 2; }    // two groups of four waves, two row tiles each
    else if (2 * img <= CHAIN_LDS_EX) { RT = 2; GR = 1; }
    else if (img <= CHAIN_LDS_EX) { RT = 1; GR = 1; }
    // the widest bands (32 rows would be all the LDS holds): 48 rows on 16 x 16 x 32 MFMAs instead (chain_body48); there the
    // layer fields count k-steps of 32 and feature tiles of 16
    // ... and bands of the 64-row class whose image leaves room for FIVE row tiles of 16 and whose feature tiles of 16 are at most
    // three per wave (the 384-wide band: 24 tiles = 3 x 8 where the 32 x 32 geometry has twelve tiles for eight waves): 80 rows
    // per weight fragment instead of 64, every wave busy (BSRNN_CHAIN_NO80=1 keeps them on the 32 x 32 geometry)
    const bool try48 = RT == 1 && GR == 1 && !kn.no48;
    const bool try80 = RT == 2 && GR == 1 && !kn.no48 && !kn.no80;
    // ... and the other bands of the 64-row class (the 514-wide band: 33 feature tiles of 16, ragged) on FOUR row tiles of 16: the same 64
    // rows, but two feature tiles' fragments per k-step and four k-steps in flight per wave (128 KB per CU instead of the 64 KB the
    // two-row-tile 32 x 32 body has registers for, which held its K loops at 48 GB/s per CU against the 70 the fill path gives:
    // profiles/r03_chain_trace.txt)
    bool try64 = false;
    if (try48 || try80) {
        int rt16 = try48 ? 3 : 5, ctr = try48 ? 6 : 3;
        int u48 = 0, maxft = 0, nb48 = 0;
        bool whole = true;                                   // every layer's width a multiple of 16 (no ragged tile of 16)
        bool gap = false;                                    // a layer's output (whole tiles of 16) ends short of the next layer's
                                                             // K loop (whole k-steps of 32): N % 32 != 0
        for (int l = 0; l < CHAIN_LAYERS; ++l) {
            const int K32 = (ld[l].Kd + 31) / 32, FT = (ld[l].N + 15) / 16;
            u48 = imax(u48, 4 * K32);
            if (l + 1 < CHAIN_LAYERS) u48 = imax(u48, 2 * FT);
            maxft = imax(maxft, FT); nb48 += 16 * FT;
            whole = whole && ld[l].N % 16 == 0;
            gap = gap || (l + 1 < CHAIN_LAYERS && ld[l].N % 32 != 0);
        }
        if (try80 && !(whole && maxft % 8 == 0 && maxft <= 8 * ctr && 2 * u48 * (16 * rt16) * 16 <= CHAIN_LDS_EX)) {
            try64 = true; rt16 = 4; ctr = 5;
        }
        if (2 * u48 * (16 * rt16) * 16 <= CHAIN_LDS_EX && maxft <= 8 * ctr && nb48 * 4 <= CHAIN_LDS_BIAS && (try48 || try64 || (whole && maxft % 8 == 0))) {
            g.g48 = true; RT = rt16; GR = 1; units = u48; nbias = 0; cost = 0; d.zpad = rt16 == 4 || gap;   // (the 64-row body always zeroes)
            for (int l = 0; l < CHAIN_LAYERS; ++l) {
                d.L[l].K16 = (ld[l].Kd + 31) / 32; d.L[l].NTL = (ld[l].N + 15) / 16;
                d.L[l].bias_off = nbias; nbias += 16 * d.L[l].NTL;
                cost += (long)d.L[l].K16 * d.L[l].NTL;          // (half the MACs of a 32 x 32 x 16 unit each: same scale per row)
            }
        }
    }
    const int ct_max = GR == 8 ? 4 : CHAIN_CT;                                // feature tiles per wave the geometry's body holds
    if (!g.g48 && (RT < 1 || (8 / GR) * ct_max < maxntl || nbias * 4 > CHAIN_LDS_BIAS)) return g;   // a band too wide for the fused kernel: per-layer flow
    g.fits = true;
    d.RT = RT; d.NW = 8 / GR; d.plane_units = units; d.nbias = nbias;
    // a last feature tile with at most 4 real features (514 columns = 16 tiles + 2) is split over the k-steps of all eight
    // waves instead of costing one wave a whole tile (mlp_chain.hip, split_host.h): the geometry that implements it is
    // RT 2 / GR 1, and the partial sums need 8 KB of LDS behind the two activation images
    if (kn.rag && !g.g48 && RT == 2 && GR == 1 && 2 * img + CHAIN_RAG_LDS <= CHAIN_LDS_EX)
        for (int l = 0; l < CHAIN_LAYERS; ++l) {
            const int tail = ld[l].N % 32;
            if (tail >= 1 && tail <= 4 && d.L[l].NTL >= 2) {
                d.L[l].rag = 1;
                cost -= (long)d.L[l].K16 - d.L[l].K16 / 8;
            }
        }
    g.cost = cost;
    return g;
}

// What bsrnn_chain_geometry (include/bsrnn_hip.h) answers for a band's descriptor:
// {rows per workgroup, MFMA shape 32 | 16, RT, NW, bit l = layer l's last tile is split, pad zeroing}
inline void chain_geometry_answer(const ChainDesc& d, int out[6])
{
    out[0] = chain_rows(d); out[1] = d.RT >= 3 ? 16 : 32; out[2] = d.RT; out[3] = d.NW; out[4] = 0;
    for (int l = 0; l < CHAIN_LAYERS; ++l) out[4] |= d.L[l].rag ? 1 << l : 0;
    out[5] = d.zpad;
}

// ------------------------------------------------------------------ operand packing of the 16 x 16 x 32 MFMA (lstm.hip)
// A matrix as two fp16 pieces in the B-operand order, out[n_tiles][n_blk][2 piece][64 lane][8]: lane (n = l & 15, kb = l >> 4) of
// block (tile, bk) holds elem(tile, n, 32 bk + 8 kb + e), e < 8 - the fp32 element of row n of the tile, column k.  The caller says
// which matrix rows a tile is (and, by what it passes as `out` and adds to k, where its blocks sit among others).
template <class Elem>
inline void pack_bfrag16(uint16_t* out, int n_tiles, int n_blk, Elem elem)
{
    for (int tile = 0; tile < n_tiles; ++tile)
        for (int bk = 0; bk < n_blk; ++bk)
            for (int ln = 0; ln < 64; ++ln)
                for (int e = 0; e < 8; ++e) {
                    const float v = elem(tile, ln & 15, 32 * bk + 8 * (ln >> 4) + e);
                    uint16_t pc[2];
                    split_planes_host(&v, 1, 2, pc);
                    uint16_t* o = out + (((size_t)tile * n_blk + bk) * 2 * 64 + ln) * 8 + e;
                    o[0] = pc[0];
                    o[64 * 8] = pc[1];
                }
}

// [W_ih (fc_in folded for layer 0) | W_hh] and the summed bias of one LSTM layer/direction
inline void lstm_cat(const ParamLookup& P, int j, int layer, const char* sfx, int n_in, std::vector<double>& wcat, std::vector<double>& bsum)
{
    char b[128];
    const int H = HID, KT = n_in + H;
    snprintf(b, sizeof b, "lstms.%d.m.rnn.weight_ih_l%d%s", j, layer, sfx); const std::vector<float>& wih = P(b);
    snprintf(b, sizeof b, "lstms.%d.m.rnn.weight_hh_l%d%s", j, layer, sfx); const std::vector<float>& whh = P(b);
    snprintf(b, sizeof b, "lstms.%d.m.rnn.bias_ih_l%d%s", j, layer, sfx); const std::vector<float>& bih = P(b);
    snprintf(b, sizeof b, "lstms.%d.m.rnn.bias_hh_l%d%s", j, layer, sfx); const std::vector<float>& bhh = P(b);
    wcat.assign((size_t)4 * H * KT, 0.0);
    bsum.assign(4 * H, 0.0);
    for (int r = 0; r < 4 * H; ++r) bsum[r] = (double)bih[r] + (double)bhh[r];
    if (layer == 0) {
        // fc_in folded: W' = W_ih W_in, b' += W_ih b_in   (bsrnn.py:82-83: rnn(fc_in(x)), no activation between)
        snprintf(b, sizeof b, "lstms.%d.m.fc_in.weight", j); const std::vector<float>& win = P(b);
        snprintf(b, sizeof b, "lstms.%d.m.fc_in.bias", j); const std::vector<float>& bin = P(b);
        for (int r = 0; r < 4 * H; ++r) {
            for (int k = 0; k < H; ++k) {
                double s = 0;
                for (int u = 0; u < H; ++u) s += (double)wih[(size_t)r * H + u] * (double)win[(size_t)u * H + k];
                wcat[(size_t)r * KT + k] = s;
            }
            double sb = 0;
            for (int u = 0; u < H; ++u) sb += (double)wih[(size_t)r * H + u] * (double)bin[u];
            bsum[r] += sb;
        }
    } else {
        for (int r = 0; r < 4 * H; ++r)
            for (int k = 0; k < n_in; ++k) wcat[(size_t)r * KT + k] = wih[(size_t)r * n_in + k];
    }
    for (int r = 0; r < 4 * H; ++r)
        for (int k = 0; k < H; ++k) wcat[(size_t)r * KT + n_in + k] = whh[(size_t)r * H + k];
}

// ------------------------------------------------------------------ the image
// A descriptor and, beside it, the arena offsets (in floats) that its pointer fields get once the arena has a device address;
// the pointer fields themselves stay null on the host.
struct JobRec { GemmJob j; size_t w, b, wp; };
struct ChainRec { ChainDesc d; size_t w, b; long cost; };       // cost < 0: constant band
struct SlotTables { int job0[NSLOT], njobs[NSLOT], tile0[NSLOT], ntiles[NSLOT], tile_n[NSLOT]; };
// Arena offsets of the recurrent weights of dual-path block blk (lstms.2blk over bands, lstms.2blk+1 over time) in the kernels'
// register order (kernels.h: launch_band_lstm, launch_time_lstm, launch_band_block_small)
struct BlockSegs {
    size_t bandW[2], bandB[2], bandW16[2];     // per layer: fp32 [2 dir][4 wave][(IN+64)/4 step][4 gate][64 lane], bias [2][256], fp16x2 fragments
    size_t bandFc16, bandFcB;                  // the block's fc (128 -> 64) as fp16x2 B fragments [4 tile][4 blk][2 piece][64 lane][8], its bias
    size_t timeW, timeB, timeW16;              // both layers: fp32 [2 layer][4 wave][128 k][64 lane], bias [2][256], fp16x2 fragments
    size_t timeFc16, timeFcB;                  // the block's fc (64 -> 64): [4 wave][2 blk][2 piece][64 lane][8], its bias
};
struct WeightImage {
    std::vector<float> arena;                  // 16-byte aligned segments
    std::vector<JobRec> jobs;
    std::vector<GemmTile> tiles;               // .job is relative to the slot's first job
    SlotTables slots;
    bool fused = false;                        // false: per-layer launches (BSRNN_MLP=layers, fp32 mode, or a band too wide for the LDS image)
    std::vector<ChainRec> chains[2];           // grouped by class (rows per workgroup), heaviest band first inside a class
    BlockSegs blk[2];

    size_t put(const float* p, size_t n)
    {
        size_t o = (arena.size() + 3) & ~size_t(3);
        arena.resize(o + n);
        if (n) memcpy(&arena[o], p, n * sizeof(float));
        return o;
    }
    size_t put(const std::vector<float>& v) { return put(v.data(), v.size()); }
    size_t put(const std::vector<uint16_t>& v) { return put(reinterpret_cast<const float*>(v.data()), v.size() / 2); }   // (an even count)
};

// One Linear layer as a job of its slot: fp32 weights, bias and (fp16x2 / fp16 modes) the same matrix as two fp16 pieces,
// slab-interleaved, rows padded to a multiple of 32 (gemm_h2_kernel), packed into arena floats
inline void add_job(WeightImage& im, const ParamLookup& P, int gmode, const char* prefix, int N, int Kd, int x_off, int y_off, int r_off, int m_off)
{
    JobRec r;
    memset(&r, 0, sizeof r);
    GemmJob& j = r.j;
    j.N = N; j.x_off = x_off; j.y_off = y_off; j.r_off = r_off; j.m_off = m_off;
    const std::vector<float>& w = P(std::string(prefix) + ".weight");
    // weight rows padded with zeros to a multiple of 8: every row is 16-byte aligned in fp32 and in the 16-bit
    // planes, and the kernels' K loops run over whole 16-byte units (the matching input pad columns are zero,
    // see ensure_ws and the GEMM epilogue)
    const int Kp = round8(Kd), K32 = (Kp + 31) & ~31;
    j.K = Kp;
    j.wrow = h2_row_stride(K32);
    std::vector<float> wp((size_t)N * Kp, 0.f);
    for (int row = 0; row < N; ++row) memcpy(&wp[(size_t)row * Kp], &w[(size_t)row * Kd], Kd * sizeof(float));
    r.w = im.put(wp);
    r.b = im.put(P(std::string(prefix) + ".bias"));
    if (gmode != GEMM_F32 && !wp.empty()) {
        std::vector<uint16_t> pl((size_t)N * j.wrow + 1, 0);
        pack_h2_slabs_host(wp.data(), N, Kp, Kp, K32, j.wrow, pl.data());
        std::vector<float> packed(pl.size() / 2 + 1);
        memcpy(packed.data(), pl.data(), pl.size() * sizeof(uint16_t));
        r.wp = im.put(packed);
    }
    im.jobs.push_back(r);
}

// Column tiles of a slot whose jobs are im.jobs[job0[slot] ...]: 128 wide when any layer of the slot is wider than 64 columns (the
// 128 x 128 kernel does twice the MFMA work per barrier), else 64; heaviest K first so the tail of a launch is made of cheap tiles.
inline void end_slot(WeightImage& im, int gmode, int slot)
{
    SlotTables& s = im.slots;
    const int j0 = s.job0[slot], j1 = (int)im.jobs.size();
    s.njobs[slot] = j1 - j0;
    int maxn = 0;
    for (int ji = j0; ji < j1; ++ji) maxn = imax(maxn, im.jobs[ji].j.N);
    // 128-wide tiles pay off only when the launch has many more workgroups than CU slots (uniform
    // large GEMMs: 114 vs 99 TFLOP/s); at M = C*T ~ 8k rows the 64-wide tiling balances the ragged
    // per-band costs better (measured 2.75 vs 2.79 ms per step), so it is the default.
    // The split-precision kernels do 2-3x less matrix-pipe work per tile and are bound by the CU's load
    // path instead: there the 128-wide tile (2/3 of the bytes per flop) wins (tools/gemm_planes_bench.hip).
    const int tn = (maxn > 64 && gmode != GEMM_F32) ? 128 : 64;
    s.tile_n[slot] = tn;
    std::vector<int> order;
    for (int ji = j0; ji < j1; ++ji) order.push_back(ji);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return im.jobs[a].j.K > im.jobs[b].j.K; });
    for (int ji : order)
        for (int t = 0; t < (im.jobs[ji].j.N + tn - 1) / tn; ++t) im.tiles.push_back(GemmTile{ji - j0, t});
    s.ntiles[slot] = (int)im.tiles.size() - s.tile0[slot];
}

// Job and tile tables of the 14 layer slots.  aoff / poff: first column of band i in the activation rows (32-column granularity) and
// in the band-padded spectrum rows (16-byte aligned)
inline void build_jobs(WeightImage& im, const ParamLookup& P, const std::vector<int>& widths, const std::vector<int>& aoff,
                       const std::vector<int>& poff, int gmode)
{
    const int H = HID, K = (int)widths.size();
    char b[128];
    auto begin_slot = [&](int slot) { im.slots.job0[slot] = (int)im.jobs.size(); im.slots.tile0[slot] = (int)im.tiles.size(); };
    // per-band MLP chains
    for (int slot = PRE0; slot <= POST2; ++slot) {
        begin_slot(slot);
        for (int i = 0; i < K; ++i) {
            const int a = 2 * widths[i], m = imax(a, H), pz = imax(a, 2 * H);
            const int xin = poff[i], act = aoff[i];
            if (a == 0) {
                if (slot == FC4) {                 // TrainableConstantModule -> Z[:, :, i, :] = constant
                    JobRec r;
                    memset(&r, 0, sizeof r);
                    r.j.N = H; r.j.K = 0; r.j.y_off = i * H;
                    snprintf(b, sizeof b, "bandFCs.%d.0.trainable_constant", i);
                    const std::vector<float>& cst = P(b);
                    r.w = im.put(cst); r.b = im.put(cst);
                    im.jobs.push_back(r);
                }
                continue;
            }
            switch (slot) {
            case PRE0:  snprintf(b, sizeof b, "bandFCs_pre.%d.0", i); add_job(im, P, gmode, b, a, a, xin, act, 0, 0); break;
            case PRE2:  snprintf(b, sizeof b, "bandFCs_pre.%d.2", i); add_job(im, P, gmode, b, a, a, act, xin, 0, 0); break;
            case FC0:   snprintf(b, sizeof b, "bandFCs.%d.0", i); add_job(im, P, gmode, b, m, a, xin, act, 0, 0); break;
            case FC2:   snprintf(b, sizeof b, "bandFCs.%d.2", i); add_job(im, P, gmode, b, H, m, act, act, 0, 0); break;
            case FC4:   snprintf(b, sizeof b, "bandFCs.%d.4", i); add_job(im, P, gmode, b, H, H, act, i * H, 0, 0); break;
            case BACK0: snprintf(b, sizeof b, "bandFCs_back.%d.0", i); add_job(im, P, gmode, b, 2 * H, H, i * H, act, 0, 0); break;
            case BACK2: snprintf(b, sizeof b, "bandFCs_back.%d.2", i); add_job(im, P, gmode, b, pz, 2 * H, act, act, 0, 0); break;
            case BACK4: snprintf(b, sizeof b, "bandFCs_back.%d.4", i); add_job(im, P, gmode, b, a, pz, act, act, 0, 0); break;
            case POST0: snprintf(b, sizeof b, "bandFCs_back_post.%d.0", i); add_job(im, P, gmode, b, a, a, act, act, 0, 0); break;
            case POST2: snprintf(b, sizeof b, "bandFCs_back_post.%d.2", i); add_job(im, P, gmode, b, a, a, act, xin, xin, xin); break;
            }
        }
        end_slot(im, gmode, slot);
    }
    // fc of the four NormRNNResidual blocks (bsrnn.py:84), one job each over M*K rows
    for (int j = 0; j < 4; ++j) {
        begin_slot(BLK_FC0 + j);
        snprintf(b, sizeof b, "lstms.%d.m.fc", j);
        add_job(im, P, gmode, b, H, (j % 2 == 0) ? 2 * H : H, 0, 0, 0, 0);
        end_slot(im, gmode, BLK_FC0 + j);
    }
}

// Fused chains (mlp_chain.hip): per band and chain the five layers' fragment streams, the concatenated biases and a descriptor;
// classes by rows per workgroup (the activation image of a row tile must fit 96 KB / RT of LDS).  Returns false when a band does
// not fit the fused kernel (what was packed until then stays in the arena, unused).
inline bool build_chains(WeightImage& im, const ParamLookup& P, const std::vector<int>& widths, const std::vector<int>& poff, const CommitKnobs& kn)
{
    const int H = HID, K = (int)widths.size(), gmode = kn.gemm_mode;
    char b[128];
    for (int ch = 0; ch < 2; ++ch) {
        std::vector<ChainRec> built;
        for (int i = 0; i < K; ++i) {
            const int a = 2 * widths[i], m = imax(a, H), pz = imax(a, 2 * H);
            ChainRec bu;
            memset(&bu, 0, sizeof bu);
            if (a == 0) {
                if (ch != CHAIN_SPLIT) continue;
                snprintf(b, sizeof b, "bandFCs.%d.0.trainable_constant", i);
                bu.d.constant = 1; bu.d.NW = 1; bu.d.RT = 1; bu.d.nbias = H;     // (a 256-row class member, like the GR = 8 geometry)
                bu.b = im.put(P(b)); bu.cost = -1;
            } else {
                const LayerDims split_l[5] = {{"bandFCs_pre.%d.0", a, a, 1}, {"bandFCs_pre.%d.2", a, a, 1}, {"bandFCs.%d.0", m, a, 1},
                                              {"bandFCs.%d.2", H, m, 1}, {"bandFCs.%d.4", H, H, 0}};
                const LayerDims mask_l[5] = {{"bandFCs_back.%d.0", 2 * H, H, 1}, {"bandFCs_back.%d.2", pz, 2 * H, 1}, {"bandFCs_back.%d.4", a, pz, 1},
                                             {"bandFCs_back_post.%d.0", a, a, 1}, {"bandFCs_back_post.%d.2", a, a, 0}};
                const LayerDims* ld = ch == CHAIN_SPLIT ? split_l : mask_l;
                const ChainGeometry g = chain_geometry(ld, kn);
                if (!g.fits) return false;
                ChainDesc& d = bu.d;
                d = g.d;
                d.in_off = ch == CHAIN_SPLIT ? poff[i] : i * H;
                d.K0 = ch == CHAIN_SPLIT ? round8(a) : H;
                std::vector<uint16_t> stream;
                std::vector<float> biases(d.nbias, 0.f);
                for (int l = 0; l < CHAIN_LAYERS; ++l) {
                    snprintf(b, sizeof b, ld[l].fmt, i);
                    const std::vector<float>& w = P(std::string(b) + ".weight");
                    const std::vector<float>& bi = P(std::string(b) + ".bias");
                    d.L[l].w_off = (unsigned)(stream.size() * sizeof(uint16_t));
                    const int npl = (gmode == GEMM_FP16 || gmode == GEMM_BF16) ? 1 : 2;
                    if (g.g48) pack_chain_layer16_host(w.data(), ld[l].N, ld[l].Kd, ld[l].Kd, 8, npl, stream, gmode == GEMM_BF16);
                    else pack_chain_layer_host(w.data(), ld[l].N, ld[l].Kd, ld[l].Kd, d.NW, npl, stream, d.L[l].rag, gmode == GEMM_BF16);
                    memcpy(&biases[d.L[l].bias_off], bi.data(), ld[l].N * sizeof(float));
                }
                stream.resize((stream.size() + 7) & ~size_t(7), 0);
                bu.w = im.put(stream);
                bu.b = im.put(biases);
                bu.cost = g.cost;
            }
            bu.d.p_off = poff[i]; bu.d.a8 = round8(a); bu.d.z_off = i * H;
            built.push_back(bu);
        }
        // class = rows per workgroup (RT = 1, 2, 4, constant bands), heaviest band first inside a class
        std::stable_sort(built.begin(), built.end(), [](const ChainRec& x, const ChainRec& y) {
            auto cls = [](const ChainDesc& d) { const int rows = chain_rows(d); return d.constant ? 4 : (rows <= 48 ? 0 : (rows <= 80 ? 1 : (rows == 128 ? 2 : 3))); };
            const int cx = cls(x.d), cy = cls(y.d);
            return cx != cy ? cx < cy : x.cost > y.cost;
        });
        im.chains[ch] = built;
    }
    return true;
}

// LSTM weights, folded and packed in the kernels' register order (lstm.hip), and the blocks' fc layers as B fragments
inline void build_blocks(WeightImage& im, const ParamLookup& P)
{
    const int H = HID;
    char b[128];
    std::vector<double> wcat, bsum;
    for (int blk = 0; blk < 2; ++blk) {
        BlockSegs& s = im.blk[blk];
        const int jb = 2 * blk;                                // lstms.0 / lstms.2: bidirectional over bands
        for (int layer = 0; layer < 2; ++layer) {
            const int IN = layer == 0 ? H : 2 * H, KT = IN + H, NS = KT / 4, NB = KT / 32;
            std::vector<float> pk((size_t)2 * 4 * NS * 4 * 64), pb(2 * 256);
            std::vector<uint16_t> pk16((size_t)2 * 4 * NB * 4 * 2 * 64 * 8);       // [2 dir][4 wave][NB blk][4 gate][2 piece][64 lane][8]
            for (int d = 0; d < 2; ++d) {
                lstm_cat(P, jb, layer, d ? "_reverse" : "", IN, wcat, bsum);
                for (int wv = 0; wv < 4; ++wv)
                    for (int bk = 0; bk < NB; ++bk)
                        pack_bfrag16(&pk16[((((size_t)d * 4 + wv) * NB + bk) * 4) * 2 * 64 * 8], 4, 1,
                                     [&](int g, int n, int k) { return (float)wcat[(size_t)(g * 64 + 16 * wv + n) * KT + 32 * bk + k]; });
                for (int wv = 0; wv < 4; ++wv)
                    for (int st = 0; st < NS; ++st)
                        for (int g = 0; g < 4; ++g)
                            for (int ln = 0; ln < 64; ++ln) {
                                const int row = g * 64 + 16 * wv + (ln & 15);
                                const int k = 16 * (st / 4) + 4 * (ln >> 4) + (st % 4);
                                pk[((((size_t)d * 4 + wv) * NS + st) * 4 + g) * 64 + ln] = (float)wcat[(size_t)row * KT + k];
                            }
                for (int r = 0; r < 256; ++r) pb[d * 256 + r] = (float)bsum[r];
            }
            s.bandW[layer] = im.put(pk);
            s.bandB[layer] = im.put(pb);
            s.bandW16[layer] = im.put(pk16);
        }
        {   // the block's fc (128 -> 64, bsrnn.py:84) for band_block_small_kernel: tile = 16 output features
            snprintf(b, sizeof b, "lstms.%d.m.fc.weight", jb); const std::vector<float>& wfc = P(b);
            std::vector<uint16_t> f16((size_t)4 * 4 * 2 * 64 * 8);
            pack_bfrag16(f16.data(), 4, 4, [&](int tl, int n, int k) { return wfc[(size_t)(16 * tl + n) * 2 * H + k]; });
            s.bandFc16 = im.put(f16);
            snprintf(b, sizeof b, "lstms.%d.m.fc.bias", jb);
            s.bandFcB = im.put(P(b));
        }
        const int jt = 2 * blk + 1;                            // lstms.1 / lstms.3: causal over time
        std::vector<float> pk((size_t)2 * 4 * 128 * 64), pb(2 * 256);
        std::vector<uint16_t> pk16((size_t)2 * 4 * 4 * 4 * 2 * 64 * 8);            // [2 layer][4 wave][4 blk][4 gate][2 piece][64 lane][8]
        for (int layer = 0; layer < 2; ++layer) {
            lstm_cat(P, jt, layer, "", H, wcat, bsum);
            for (int wv = 0; wv < 4; ++wv)
                for (int bk = 0; bk < 4; ++bk)
                    pack_bfrag16(&pk16[((((size_t)layer * 4 + wv) * 4 + bk) * 4) * 2 * 64 * 8], 4, 1,
                                 [&](int g, int n, int k) { return (float)wcat[(size_t)(g * 64 + 16 * wv + n) * 128 + 32 * bk + k]; });
            for (int wv = 0; wv < 4; ++wv)
                for (int k = 0; k < 128; ++k)
                    for (int ln = 0; ln < 64; ++ln) {
                        const int row = (ln & 3) * 64 + 16 * wv + (ln >> 2);
                        pk[(((size_t)layer * 4 + wv) * 128 + k) * 64 + ln] = (float)wcat[(size_t)row * 128 + k];
                    }
            for (int r = 0; r < 256; ++r) pb[layer * 256 + r] = (float)bsum[r];
        }
        s.timeW = im.put(pk);
        s.timeW16 = im.put(pk16);
        s.timeB = im.put(pb);
        {   // the block's fc (64 -> 64, bsrnn.py:84), fused into the time-axis launch: tile = the 16 output features of a wave
            snprintf(b, sizeof b, "lstms.%d.m.fc.weight", jt); const std::vector<float>& wfc = P(b);
            std::vector<uint16_t> f16((size_t)4 * 2 * 2 * 64 * 8);
            pack_bfrag16(f16.data(), 4, 2, [&](int wv, int n, int k) { return wfc[(size_t)(16 * wv + n) * H + k]; });
            s.timeFc16 = im.put(f16);
            snprintf(b, sizeof b, "lstms.%d.m.fc.bias", jt);
            s.timeFcB = im.put(P(b));
        }
    }
}

inline WeightImage build_weight_image(const ParamLookup& P, const std::vector<int>& widths, const std::vector<int>& aoff,
                                      const std::vector<int>& poff, const CommitKnobs& kn)
{
    WeightImage im;
    build_jobs(im, P, widths, aoff, poff, kn.gemm_mode);
    im.fused = kn.gemm_mode != GEMM_F32 && !kn.mlp_layers && build_chains(im, P, widths, poff, kn);
    build_blocks(im, P);
    return im;
}

}  // namespace bsrnn
