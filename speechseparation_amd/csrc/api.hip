// C ABI of libbsrnn_hip.so (include/bsrnn_hip.h): context, parameter intake by the reference's
// state_dict key names, host-side folding/packing, workspace, and the launch sequence of
// BSRNN.forward / forward_recurrent (bsrnn.py:385-510) and of the callers' STFT sandwich.
// There is no CPU compute path here: every entry point either enqueues HIP kernels or fails.
// This unit: context, parameters and commit, call plan and dual path, the offline / ragged / long-form / evaluate / training entry points,
// measurement, memory helpers - and what api_internal.h declares for the other host units (api_stream.hip, api_resample.hip, api_pool.hip).
#include "api_internal.h"
#include "metrics_host.h"
#include "sections_host.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace bsrnn::host {

std::atomic<long long> g_dbg[5];

static thread_local char g_err[512] = "";
int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// --------------------------------------------------------------------------- the upload ring (api_internal.h)
hipError_t UploadRing::reserve(size_t bytes)
{
    if (bytes <= cap) return hipSuccess;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return e;
    if (d) { (void)hipFree(d); (void)hipHostFree(h); d = h = nullptr; cap = 0; }
    g_dbg[DBG_ALLOC] += 2;
    if ((e = hipHostMalloc((void**)&h, MIRRORS * bytes, hipHostMallocDefault)) != hipSuccess) { h = nullptr; return e; }
    if ((e = hipMalloc((void**)&d, bytes)) != hipSuccess) { (void)hipHostFree(h); h = d = nullptr; return e; }
    for (hipEvent_t& v : ev)
        if (!v && (e = hipEventCreateWithFlags(&v, hipEventDisableTiming)) != hipSuccess) return e;
    cap = bytes;
    return hipSuccess;
}
void UploadRing::release()
{
    if (d) { (void)hipFree(d); (void)hipHostFree(h); d = h = nullptr; cap = 0; }      // (both or neither: reserve)
    for (hipEvent_t& v : ev)
        if (v) { (void)hipEventDestroy(v); v = nullptr; }
}

// --------------------------------------------------------------------------- context
const char* kStageNames[NSTAGE] = {"layout", "stft", "bandsplit_mlp", "band_lstm", "band_fc", "time_lstm", "time_fc",
                                   "mask_mlp", "istft", "stream_dsp"};

int add_param(bsrnn_ctx* c, const std::string& key, int64_t d0, int64_t d1, int ndim)
{
    Param p;
    p.key = key; p.d0 = d0; p.d1 = d1; p.ndim = ndim;
    c->index[key] = (int)c->params.size();
    c->params.push_back(p);
    return 0;
}
void add_linear(bsrnn_ctx* c, const std::string& prefix, int n_out, int n_in)
{
    add_param(c, prefix + ".weight", n_out, n_in, 2);
    add_param(c, prefix + ".bias", n_out, 0, 1);
}

// parameter inventory in the reference's state_dict order (bsrnn.py:329-376)
void build_inventory(bsrnn_ctx* c)
{
    char b[128];
    const int H = HID;
    for (int i = 0; i < c->K; ++i) {
        const int a = 2 * c->widths[i];
        if (a > 0) {
            snprintf(b, sizeof b, "bandFCs_pre.%d.0", i); add_linear(c, b, a, a);
            snprintf(b, sizeof b, "bandFCs_pre.%d.2", i); add_linear(c, b, a, a);
        } else { snprintf(b, sizeof b, "bandFCs_pre.%d.0.trainable_constant", i); add_param(c, b, 0, 0, 1); }
    }
    for (int i = 0; i < c->K; ++i) {
        const int a = 2 * c->widths[i], m = imax(a, H);
        if (a > 0) {
            snprintf(b, sizeof b, "bandFCs.%d.0", i); add_linear(c, b, m, a);
            snprintf(b, sizeof b, "bandFCs.%d.2", i); add_linear(c, b, H, m);
            snprintf(b, sizeof b, "bandFCs.%d.4", i); add_linear(c, b, H, H);
        } else { snprintf(b, sizeof b, "bandFCs.%d.0.trainable_constant", i); add_param(c, b, H, 0, 1); }
    }
    for (int j = 0; j < 4; ++j) {
        const bool bidir = (j % 2 == 0);
        snprintf(b, sizeof b, "lstms.%d.m.fc_in", j); add_linear(c, b, H, H);
        for (int layer = 0; layer < 2; ++layer) {
            const int n_in = layer == 0 ? H : (bidir ? 2 * H : H);
            for (int d = 0; d < (bidir ? 2 : 1); ++d) {
                const char* sfx = d ? "_reverse" : "";
                snprintf(b, sizeof b, "lstms.%d.m.rnn.weight_ih_l%d%s", j, layer, sfx); add_param(c, b, 4 * H, n_in, 2);
                snprintf(b, sizeof b, "lstms.%d.m.rnn.weight_hh_l%d%s", j, layer, sfx); add_param(c, b, 4 * H, H, 2);
                snprintf(b, sizeof b, "lstms.%d.m.rnn.bias_ih_l%d%s", j, layer, sfx); add_param(c, b, 4 * H, 0, 1);
                snprintf(b, sizeof b, "lstms.%d.m.rnn.bias_hh_l%d%s", j, layer, sfx); add_param(c, b, 4 * H, 0, 1);
            }
        }
        snprintf(b, sizeof b, "lstms.%d.m.fc", j); add_linear(c, b, H, bidir ? 2 * H : H);
    }
    for (int i = 0; i < c->K; ++i) {
        const int a = 2 * c->widths[i], pz = imax(a, 2 * H);
        if (a > 0) {
            snprintf(b, sizeof b, "bandFCs_back.%d.0", i); add_linear(c, b, 2 * H, H);
            snprintf(b, sizeof b, "bandFCs_back.%d.2", i); add_linear(c, b, pz, 2 * H);
            snprintf(b, sizeof b, "bandFCs_back.%d.4", i); add_linear(c, b, a, pz);
        } else { snprintf(b, sizeof b, "bandFCs_back.%d.0.trainable_constant", i); add_param(c, b, 0, 0, 1); }
    }
    for (int i = 0; i < c->K; ++i) {
        const int a = 2 * c->widths[i];
        if (a > 0) {
            snprintf(b, sizeof b, "bandFCs_back_post.%d.0", i); add_linear(c, b, a, a);
            snprintf(b, sizeof b, "bandFCs_back_post.%d.2", i); add_linear(c, b, a, a);
        } else { snprintf(b, sizeof b, "bandFCs_back_post.%d.0.trainable_constant", i); add_param(c, b, 0, 0, 1); }
    }
}

int ensure_ws(bsrnn_ctx* c, size_t rows)
{
    if (rows <= c->cap_rows) return 0;
    // Grow-only, geometrically, and the outgrown buffer is RETIRED, not freed: a hipGraph captured by the caller (train.GraphedTrainStep keeps
    // one per clip length; a user's torch.cuda.graph around forward) holds workspace addresses in its kernel nodes, and work of the previous
    // call may still be running in it.  It stays valid scratch for whoever knows it; everything new uses the new one (streaming graphs of
    // this library re-capture: generation counter).  At most ~3x the final size in all, released with the context.
    if (c->cap_rows) rows = std::max(rows, c->cap_rows + c->cap_rows / 2);
    size_t sizes[WS_SEGS], total = 0;
    workspace_segments(rows, c->LDP, c->LDA, c->K, sizes);
    for (size_t s : sizes) total += s;
    float* fresh = nullptr;
    ++g_dbg[DBG_ALLOC];
    HIP_TRY(hipMalloc((void**)&fresh, total * sizeof(float)));
    // pad columns (band segments are 16-byte aligned, rows padded) are read as K-padding by the GEMM and are
    // never written afterwards: they must be finite, so the whole workspace starts at zero
    HIP_TRY(hipMemset(fresh, 0, total * sizeof(float)));
    if (c->d_ws) c->retired.push_back(c->d_ws);
    c->d_ws = fresh;
    float* p = c->d_ws;
    float** dst[10] = {&c->Xf, &c->Yf, &c->A1, &c->A2, &c->P, &c->Z0, &c->Z1, &c->HB0, &c->HB1, &c->H1};
    for (int i = 0; i < 10; ++i) { *dst[i] = p; p += sizes[i]; }
    c->band_flags = reinterpret_cast<int*>(p);
    c->cap_rows = rows;
    ++c->gen;
    return 0;
}
int ensure_tap(bsrnn_ctx* c, size_t rows)
{
    if (rows <= c->tap_rows) return 0;
    if (c->tap_rows) rows = std::max(rows, c->tap_rows + c->tap_rows / 2);
    float* fresh = nullptr;
    ++g_dbg[DBG_ALLOC];
    HIP_TRY(hipMalloc((void**)&fresh, rows * c->LDP * sizeof(float)));
    if (c->d_tap) c->retired.push_back(c->d_tap);          // (retired like the workspace, see ensure_ws)
    c->d_tap = fresh;
    c->tap_rows = rows;
    ++c->gen;
    return 0;
}

int ensure_streams(bsrnn_ctx* c, int parts)
{
    if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    for (int j = 0; j < parts; ++j) {
        if (!c->aux[j]) { ++g_dbg[DBG_ALLOC]; HIP_TRY(hipStreamCreateWithFlags(&c->aux[j], hipStreamNonBlocking)); }
        if (!c->ev_join[j]) HIP_TRY(hipEventCreateWithFlags(&c->ev_join[j], hipEventDisableTiming));
    }
    return 0;
}

// A small table on the device: `bytes` of h behind a fresh allocation of bytes + slack.  On failure nothing is left allocated and *d is null.
static_assert(sizeof(ChainTask) == sizeof(int2) && alignof(ChainTask) <= alignof(int2), "the kernels read a ChainTask as an int2");
template <class T>
hipError_t upload_table(T** d, const void* h, size_t bytes, size_t slack = 0)
{
    *d = nullptr;
    hipError_t e = hipMalloc((void**)d, bytes + slack);
    if (e == hipSuccess && (e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice)) != hipSuccess) { (void)hipFree(*d); *d = nullptr; }
    return e;
}

// Task tables (build_chain_tasks, plan_host.h) for the row counts of ONE call (several when the call runs as concurrent row blocks).  The cache is bounded; when it
// is full it is dropped once, before any of this call's tables is made, so a call never evicts a table it is about to use
// (captured streaming graphs notice through ctx->gen and re-capture).
void free_chain_tasks(bsrnn_ctx* c)
{
    for (auto& kv : c->chain_tasks)
        for (int ch = 0; ch < 2; ++ch) (void)hipFree(kv.second.d[ch]);
    c->chain_tasks.clear();
}
int ensure_tasks(bsrnn_ctx* c, const int* Ms, int n)
{
    if (!c->fused) return 0;
    int missing = 0;
    for (int i = 0; i < n; ++i) missing += c->chain_tasks.find(Ms[i]) == c->chain_tasks.end();
    if (!missing) return 0;
    if (c->chain_tasks.size() + missing > c->task_cap) {
        HIP_TRY(hipDeviceSynchronize());
        free_chain_tasks(c);
        ++c->gen;
    }
    for (int i = 0; i < n; ++i) {
        if (c->chain_tasks.find(Ms[i]) != c->chain_tasks.end()) continue;
        bsrnn_ctx::TaskTable t;
        t.d[0] = t.d[1] = nullptr;
        std::vector<ChainTask> h;
        for (int ch = 0; ch < 2; ++ch) {
            build_chain_tasks(c->h_chain[ch], Ms[i], h);
            t.n[ch] = (int)h.size();
            ++g_dbg[DBG_ALLOC];
            const hipError_t e = upload_table(&t.d[ch], h.data(), h.size() * sizeof(int2), sizeof(int2));
            if (e != hipSuccess) {
                (void)hipFree(t.d[0]);
                return fail(BSRNN_EHIP, "task table: %s", hipGetErrorString(e));
            }
        }
        c->chain_tasks.emplace(Ms[i], t);
    }
    return 0;
}
int ensure_tasks(bsrnn_ctx* c, int M) { return ensure_tasks(c, &M, 1); }

void gemm_slot(bsrnn_ctx* c, bool gemv, int slot, const float* X, int ldx, float* Y, int ldy, const float* R, int ldr,
               const float* Mul, int ldm, float* tap, int M, int epi, hipStream_t s)
{
    GemmLaunch g;
    memset(&g, 0, sizeof g);
    g.range_flag = c->d_range;
    g.jobs = c->d_jobs + c->slots.job0[slot];
    g.tiles = c->d_tiles + c->slots.tile0[slot];
    g.n_tiles = c->slots.ntiles[slot];
    g.tile_n = c->slots.tile_n[slot];
    g.X = X; g.ldx = ldx; g.Y = Y; g.ldy = ldy; g.R = R; g.ldr = ldr; g.Mul = Mul; g.ldm = ldm;
    g.tap = tap; g.ldt = c->LDP; g.M = M; g.epilogue = epi;
    // a call of a few frame rows: its per-band layers (M = C rows) run as exact-fp32 GEMV launches instead of 128-row MFMA
    // tiles; the block fc layers (M K rows against a 64 x 128 matrix) stay on the MFMA kernel (measured: 5.7 vs 28 us)
    if (gemv && M <= 2 * GEMV_MAX_FRAME_ROWS) launch_gemv(g, s);
    else launch_gemm(g, s);
}

// --------------------------------------------------------------------------- the call plan (plan_host.h)
// The knobs of the plan, read from the environment once per process, at the first call that plans
static const PlanKnobs& plan_knobs()
{
    static const PlanKnobs knobs = [] {
        auto is = [](const char* name, const char* value) { const char* e = getenv(name); return e && !strcmp(e, value); };
        const char *tk = getenv("BSRNN_TIME_KERNEL"), *s8 = getenv("BSRNN_TIME_SEQ8");
        if (tk && *tk && strcmp(tk, "fused") && strcmp(tk, "v3")) fprintf(stderr, "bsrnn: unknown BSRNN_TIME_KERNEL='%s' (v3 | fused), using fused\n", tk);
        return PlanKnobs{!is("BSRNN_BAND_PAIR", "0"), !is("BSRNN_BAND_FC", "gemm"), !is("BSRNN_TIME_KERNEL", "v3"), s8 ? atoi(s8) : -1,
                         gemm_mode(), lstm_mode(), device_cus(), is("BSRNN_BAND_PAIR", "tiles1") ? 1 : is("BSRNN_BAND_PAIR", "tiles2") ? 2 : 0};
    }();
    return knobs;
}
Flow plan_call(const bsrnn_ctx* c, int C, int T, bool gemv, bool overlap)
{
    return plan_call(c->K, C, T, gemv, overlap, plan_knobs(), PlanState{force_f32(), c->fused, c->band_pair_off, c->overlap_env, c->overlap_off});
}

// A contiguous block of rows (utterance-channels) of one call, with its slice of the workspace
// and the stream it runs on.  Rows are independent (bsrnn.py:394-395), so a call can be cut into
// several such parts that run concurrently on separate HIP streams.
struct Part {
    int C, T;                       // rows and frames of this part
    Flow f;                         // this part's plan (plan_call; made again for every run of the call)
    hipStream_t s;
    const float* Xf; float* Yf; float* tap;              // [C*T][LDP], band-padded spectrum layout
    float *A1, *A2, *P, *Z0, *Z1, *HB0, *HB1, *H1;
    int* band_flags;                                     // this part's hand-over flags of the band-pair launch
    const float* state_in; float* state_out;             // [4][2][C_total*K][64] slabs already offset to this part's first row
    size_t state_slab;                                   // floats between the two Time blocks' slabs (uses C_total)
    const float* wave; float* wave_out; int64_t n;       // only for the fused sandwich
    const int64_t* lens;                                 // non-null: rows of different lengths (bsrnn_separate_ragged) - device array [C]; n unused,
    int64_t wave_stride, out_stride;                     //   rows of wave / wave_out this many floats apart
    const int2* tasks[2]; int n_tasks[2];                // non-null: this call's own task tables of the two chains (else the cache, chain_launch)
    const bsrnn_ctx::OvlTable* ovl;                      // non-null: the overlapped flow (run_overlapped) - producers publish, consumers wait
    int ovl_base;                                        // this call's epoch << OVL_EPOCH_SHIFT
    hipEvent_t band_done[2];                             // events the two band launches signal themselves when they complete (or null)
    const int* row_frames;                               // non-null: frames per row [C] on the device - the time-axis launches return the state after them (bsrnn_stream_process_hops)
};

Part make_part(bsrnn_ctx* c, int row0, int C, int T, hipStream_t s, int j = 0)
{
    Part p;
    memset(&p, 0, sizeof p);
    const size_t m0 = (size_t)row0 * T, KH = (size_t)c->K * HID;
    p.C = C; p.T = T; p.s = s;
    p.Xf = c->Xf + m0 * c->LDP; p.Yf = c->Yf + m0 * c->LDP;
    p.A1 = c->A1 + m0 * c->LDA; p.A2 = c->A2 + m0 * c->LDA; p.P = c->P + m0 * c->LDP;
    p.Z0 = c->Z0 + m0 * KH; p.Z1 = c->Z1 + m0 * KH; p.H1 = c->H1 + m0 * KH;
    p.HB0 = c->HB0 + m0 * KH * 2; p.HB1 = c->HB1 + m0 * KH * 2;
    p.band_flags = c->band_flags + flag_offset(m0, j);
    return p;
}

enum { MS_STFT, MS_BANDSPLIT, MS_BAND0, MS_BANDFC0, MS_TIME0, MS_TIMEFC0, MS_BAND1, MS_BANDFC1, MS_TIME1, MS_TIMEFC1, MS_MASK, MS_ISTFT, MS_COUNT };

// What the launches of both fused chains share for a part: the task table of its M frame rows (made by ensure_tasks() before any launch,
// and outside graph capture) and the common operands.  False: no such table (stage_error is set).
bool chain_launch(bsrnn_ctx* c, const Part& p, int chain, ChainLaunch& g)
{
    memset(&g, 0, sizeof g);
    g.desc = c->d_chain[chain];
    if (p.tasks[chain]) { g.tasks = p.tasks[chain]; g.n_tasks = p.n_tasks[chain]; }
    else {
        auto tti = c->chain_tasks.find(p.C * p.T);
        if (tti == c->chain_tasks.end()) { c->stage_error = true; return false; }
        g.tasks = tti->second.d[chain]; g.n_tasks = tti->second.n[chain];
    }
    g.M = p.C * p.T; g.P = p.P; g.ldp = c->LDP; g.range_flag = c->d_range;
    return true;
}

// One stage of the model for one part.  Xf [M][2050] -> Yf [M][2050], M = C*T, row = c*T + t.
void run_stage(bsrnn_ctx* c, const Part& p, int stage)
{
    const int M = p.C * p.T, K = c->K, KH = K * HID;
    const Flow& f = p.f;
    hipStream_t s = p.s;
    switch (stage) {
    case MS_STFT:
        if (p.wave) {
            StageScope sc(c, ST_STFT, s);
            if (p.lens) launch_stft_ragged(c->tb, p.wave, p.wave_stride, p.lens, const_cast<float*>(p.Xf), p.C, p.T, s);
            else launch_stft(c->tb, p.wave, const_cast<float*>(p.Xf), p.C, p.n, p.T, s);
        }
        break;
    case MS_BANDSPLIT: {   // bandFCs_pre (2 linears) -> residual P; bandFCs (3 linears) -> Z0   bsrnn.py:404-415
        StageScope sc(c, ST_BANDSPLIT, s);
        if (f.chains) {                   // all five layers of every band in one launch, intermediates in LDS
            ChainLaunch g;
            if (!chain_launch(c, p, CHAIN_SPLIT, g)) break;
            g.Xin = p.Xf; g.ldx = c->LDP; g.Z = p.Z0; g.ldz = KH;
            launch_mlp_chain(g, CHAIN_SPLIT, s);
            break;
        }
        gemm_slot(c, f.gemv, PRE0, p.Xf, c->LDP, p.A1, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, PRE2, p.A1, c->LDA, p.P, c->LDP, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, FC0, p.P, c->LDP, p.A1, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, FC2, p.A1, c->LDA, p.A2, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, FC4, p.A2, c->LDA, p.Z0, KH, nullptr, 0, nullptr, 0, nullptr, M, EPI_LINEAR, s);
        break;
    }
    case MS_BAND0: case MS_BAND1: {   // BandwiseLSTM: N = M sequences of length K   bsrnn.py:138-153
        const int blk = stage == MS_BAND1;
        StageScope sc(c, ST_BAND_LSTM, s);
        if (f.band == BAND_SMALL) {               // a few frame rows (streaming): the whole block, fc + residual included, in one launch
            launch_band_block_small(p.Z0, p.Z1, c->bandW16[blk][0], c->bandB[blk][0], c->bandW16[blk][1], c->bandB[blk][1],
                                    c->bandFc16[blk], c->bandFcB[blk], M, K, c->d_range, s);
            break;
        }
        // parts flow: block 0 reads Z0 and its time block writes Z1, block 1 reads Z1 and its time block writes Z0 - the block's fc +
        // residual are formed inside the two launches around them (kernels.h), MS_BANDFC does not exist
        const bool parts = f.band == BAND_PAIR_PARTS;
        const float* zi = parts && blk ? p.Z1 : p.Z0;
        if (f.band != BAND_LAYERS) {              // both layers in one launch (A/B: BSRNN_BAND_PAIR=0)
            OvlConsumer oc = {nullptr, 0, 0, nullptr, 0, 2};
            const bool cons = p.ovl && blk;
            if (cons)                             // beside the first time-axis launch: tiles in the order their frames leave it
                oc = OvlConsumer{c->d_ovl + OVL_HEAD, p.T, c->overlap_sabotage ? 200000 : OVL_SPIN_LIMIT, p.ovl->band_order, p.ovl_base, f.seqs == 8 ? 3 : 2};
            launch_band_pair(zi, p.HB0, p.HB1, c->bandW16[blk][0], c->bandB[blk][0], c->bandW16[blk][1], c->bandB[blk][1], M, K, c->d_range, s,
                             parts ? c->bandFc16[blk] : nullptr, parts ? c->bandFcB[blk] : nullptr, p.band_flags, cons ? &oc : nullptr, nullptr, 0,
                             p.ovl ? p.band_done[blk] : nullptr, f.band_tiles);
            break;
        }
        launch_band_lstm(zi, p.HB0, c->bandW[blk][0], c->bandW16[blk][0], c->bandB[blk][0], M, K, 64, c->d_range, s, f.lstm_f32);
        launch_band_lstm(p.HB0, p.HB1, c->bandW[blk][1], c->bandW16[blk][1], c->bandB[blk][1], M, K, 128, c->d_range, s, f.lstm_f32);
        break;
    }
    case MS_BANDFC0: case MS_BANDFC1: {
        const int blk = stage == MS_BANDFC1;
        if (f.band == BAND_SMALL || f.band == BAND_PAIR_PARTS) break;     // done inside the band launch / inside the launches around it
        StageScope sc(c, ST_BAND_FC, s);
        gemm_slot(c, f.gemv, BLK_FC0 + 2 * blk, p.HB1, 2 * HID, p.Z1, HID, p.Z0, HID, nullptr, 0, nullptr, M * K, EPI_RES, s);
        break;
    }
    case MS_TIME0: case MS_TIME1: {   // TimewiseLSTM: N = C*K sequences of length T, causal, state carry   bsrnn.py:106-128
        const int blk = stage == MS_TIME1;
        StageScope sc(c, ST_TIME_LSTM, s);
        // time_fc: the launch also computes the block's fc + residual (out = fc(h1) + Z1 -> Z0); otherwise it writes h1.  Parts flow: it adds
        // the band block's fc shares (HB1) to its input, block 0 reads Z0 and writes Z1; beside the band / mask launch that waits for it, it publishes
        const bool first_of_parts = f.band == BAND_PAIR_PARTS && !blk;
        OvlProducer op = {nullptr, nullptr, 0};
        if (p.ovl) op = OvlProducer{c->d_ovl + blk * c->ovl_stride, c->overlap_sabotage ? nullptr : c->d_ovl + blk * c->ovl_stride + OVL_HEAD, p.ovl_base};
        launch_time_lstm(first_of_parts ? p.Z0 : p.Z1, first_of_parts ? p.Z1 : (f.time_fc ? p.Z0 : p.H1), c->timeW[blk], c->timeW16[blk], c->timeB[blk],
                         p.state_in ? p.state_in + blk * p.state_slab : nullptr, p.state_out ? p.state_out + blk * p.state_slab : nullptr,
                         p.C, p.T, K, c->d_range, s, f.lstm_f32, f.seqs, f.time_fc ? c->timeFc16[blk] : nullptr, f.time_fc ? c->timeFcB[blk] : nullptr,
                         f.band == BAND_PAIR_PARTS ? p.HB1 : nullptr, p.ovl ? &op : nullptr, p.row_frames);
        break;
    }
    case MS_TIMEFC0: case MS_TIMEFC1: {
        const int blk = stage == MS_TIMEFC1;
        if (f.time_fc) break;                     // done inside the time-axis launch
        StageScope sc(c, ST_TIME_FC, s);
        gemm_slot(c, f.gemv, BLK_FC1 + 2 * blk, p.H1, HID, p.Z0, HID, p.Z1, HID, nullptr, 0, nullptr, M * K, EPI_RES, s);
        break;
    }
    case MS_MASK: {   // bandFCs_back (3) + bandFCs_back_post (2) + skip + x*mask   bsrnn.py:420-443
        StageScope sc(c, ST_MASK, s);
        if (f.chains) {
            ChainLaunch g;
            if (!chain_launch(c, p, CHAIN_MASK, g)) break;
            g.Xin = p.Z0; g.ldx = KH; g.Xmul = p.Xf; g.ldm = c->LDP;
            g.Y = p.Yf; g.ldy = c->LDP; g.tap = p.tap; g.ldt = c->LDP;
            if (p.ovl) {                          // beside the second time-axis launch: the earliest-ready heavy workgroups first
                g.tasks = p.ovl->mask_tasks; g.n_tasks = p.ovl->n_mask;
                g.ovl_prog = c->d_ovl + c->ovl_stride + OVL_HEAD; g.ovl_T = p.T; g.ovl_K = K;
                g.ovl_spin = c->overlap_sabotage ? 200000 : OVL_SPIN_LIMIT;
                g.ovl_base = p.ovl_base; g.ovl_wg_shift = f.seqs == 8 ? 3 : 2;
            }
            launch_mlp_chain(g, CHAIN_MASK, s);
            break;
        }
        gemm_slot(c, f.gemv, BACK0, p.Z0, KH, p.A1, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, BACK2, p.A1, c->LDA, p.A2, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, BACK4, p.A2, c->LDA, p.A1, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, POST0, p.A1, c->LDA, p.A2, c->LDA, nullptr, 0, nullptr, 0, nullptr, M, EPI_LEAKY, s);
        gemm_slot(c, f.gemv, POST2, p.A2, c->LDA, p.Yf, c->LDP, p.P, c->LDP, p.Xf, c->LDP, p.tap, M, EPI_MASK, s);
        break;
    }
    case MS_ISTFT:
        if (p.wave_out) {
            StageScope sc(c, ST_ISTFT, s);
            if (p.lens) launch_istft_ragged(c->tb, p.Yf, p.wave_out, p.out_stride, p.lens, p.C, p.T, s);
            else launch_istft(c->tb, p.Yf, p.wave_out, p.C, p.T, s);
        }
        break;
    }
}

// ---- overlapped dual path (whether a call runs it: plan_call) --------------------------------------------------------------------
static void free_ovl_tables(bsrnn_ctx* c)
{
    for (auto& kv : c->ovl_tables) { (void)hipFree(kv.second.mask_tasks); (void)hipFree(kv.second.band_order); }
    c->ovl_tables.clear();
}
// Progress words and the consumers' dispatch orders for a call of C rows x T frames planned as f (made outside any capture, like the task
// tables, and before the call's first launch).
int ensure_ovl(bsrnn_ctx* c, const Flow& f, int C, int T)
{
    if (!f.overlap) return 0;
    int rc = ensure_streams(c, 1);
    if (rc) return rc;
    if (!c->ev_ovl_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_ovl_fork, hipEventDisableTiming | hipEventDisableSystemFence));      // (device-side ordering only: no system-scope release on the record)
    if (!c->ev_ovl_join) HIP_TRY(hipEventCreateWithFlags(&c->ev_ovl_join, hipEventDisableTiming | hipEventDisableSystemFence));
    if (!c->ev_ovl_mid) HIP_TRY(hipEventCreateWithFlags(&c->ev_ovl_mid, hipEventDisableTiming | hipEventDisableSystemFence));
    const int stride = ovl_stride(f.nwg);
    if (stride > c->ovl_stride) {
        if (c->d_ovl) { c->retired.push_back(c->d_ovl); c->d_ovl = nullptr; }      // (retired like the workspace, see ensure_ws)
        ++g_dbg[DBG_ALLOC];
        HIP_TRY(hipMalloc((void**)&c->d_ovl, (size_t)2 * stride * sizeof(int)));
        HIP_TRY(hipMemset(c->d_ovl, 0, (size_t)2 * stride * sizeof(int)));
        c->ovl_stride = stride;
        c->ovl_resident_total[0] = c->ovl_resident_total[1] = 0;       // (fresh counters; the epochs go on: fresh words are below every base)
        ++c->gen;
    }
    const auto key = std::make_pair(C, T);
    if (c->ovl_tables.find(key) != c->ovl_tables.end()) return 0;
    if (c->ovl_tables.size() >= c->ovl_cap) { HIP_TRY(hipDeviceSynchronize()); free_ovl_tables(c); ++c->gen; }
    const OvlOrders o = ovl_orders(C * T, T, f.nwg, device_cus(), c->h_chain[CHAIN_MASK]);
    bsrnn_ctx::OvlTable tb;
    tb.n_mask = (int)o.mask_tasks.size(); tb.n_ord = (int)o.band_order.size();
    hipError_t e = upload_table(&tb.mask_tasks, o.mask_tasks.data(), o.mask_tasks.size() * sizeof(int2), sizeof(int2));
    if (e == hipSuccess && (e = upload_table(&tb.band_order, o.band_order.data(), o.band_order.size() * sizeof(int))) != hipSuccess) (void)hipFree(tb.mask_tasks);
    if (e != hipSuccess) return fail(BSRNN_EHIP, "overlap tables: %s", hipGetErrorString(e));
    c->ovl_tables.emplace(key, tb);
    return 0;
}

// The stages of one part with the dual path overlapped (kernels.h): caller's stream A, the context's auxiliary stream B.
//   A: [STFT] BandSplit, zero the progress words, band block 0, TIME 0 ............ gate 1, MASK chain (waits per workgroup), [iSTFT]
//   B:                                        (fork) gate 0, BAND block 1 (waits per tile), TIME 1 ......................... (join)
// gate b = one wave that leaves when every workgroup of time launch b is resident: no consumer workgroup is dispatched before that, so a
// waiting consumer never holds a CU a producer needs; producers wait for nobody.  Same kernels, same arithmetic, other dispatch order:
// bit-identical to the serial flow (tests/test_gpu_overlap.py).
void run_overlapped(bsrnn_ctx* c, Part p, const bsrnn_ctx::OvlTable* tb, int first, int last)
{
    hipStream_t A = p.s, B = c->aux[0];
    p.ovl = tb;
    Part pb = p;
    pb.s = B;
    const int nwg = p.f.nwg;
    // this call's epoch (upper bits of every progress word it publishes or waits for) and the gates' targets (running totals)
    if (++c->ovl_epoch >= c->ovl_epoch_period || c->ovl_resident_total[0] > (1 << 30) || c->ovl_resident_total[1] > (1 << 30)) {   // start again: nothing in flight, every word zero
        (void)hipDeviceSynchronize();
        (void)hipMemset(c->d_ovl, 0, (size_t)2 * c->ovl_stride * sizeof(int));
        c->ovl_epoch = 1; c->ovl_resident_total[0] = c->ovl_resident_total[1] = 0;
    }
    p.ovl_base = pb.ovl_base = c->ovl_epoch << OVL_EPOCH_SHIFT;
    c->ovl_resident_total[0] += nwg;
    c->ovl_resident_total[1] += nwg;
    // hold stream `s` until every workgroup of time launch `blk` of THIS call is resident
    auto gate = [&](int blk, hipStream_t s) { launch_ovl_gate(c->d_ovl + blk * c->ovl_stride, c->ovl_resident_total[blk], c->d_range, OVL_SPIN_LIMIT, s); };
    p.band_done[0] = pb.band_done[0] = c->ev_ovl_fork;
    p.band_done[1] = pb.band_done[1] = c->ev_ovl_mid;
    for (int st = first; st <= MS_BANDSPLIT; ++st) run_stage(c, p, st);
    run_stage(c, p, MS_BAND0);
    // the fork event keeps gate 0 off band 0's dispatch, and gate 1 waits (event) until band 1 has been dispatched completely
    (void)hipStreamWaitEvent(B, c->ev_ovl_fork, 0);              // (signalled by band 0's own dispatch: p.band_done)
    run_stage(c, p, MS_TIME0);
    gate(0, B);
    run_stage(c, pb, MS_BAND1);                                  // (... and the mid event by band 1's)
    run_stage(c, pb, MS_TIME1);
    (void)hipStreamWaitEvent(A, c->ev_ovl_mid, 0);
    gate(1, A);
    run_stage(c, p, MS_MASK);
    // The auxiliary stream is joined on the host where something needs it (finish_call under the default range policy, bsrnn_sync, a stream
    // switch) or by an event for a call that returns LSTM state; a join event in front of the iSTFT cost the caller's stream a 6 us gap.
    if (p.state_out) { (void)hipEventRecord(c->ev_ovl_join, B); (void)hipStreamWaitEvent(A, c->ev_ovl_join, 0); }
    else c->ovl_unjoined = true;
    for (int st = MS_MASK + 1; st <= last; ++st) run_stage(c, p, st);
}
// host-side join of the auxiliary stream with the last overlapped call (see run_overlapped)
int ovl_join_host(bsrnn_ctx* c)
{
    if (c->ovl_unjoined && c->aux[0]) HIP_TRY(hipStreamSynchronize(c->aux[0]));
    c->ovl_unjoined = false;
    return 0;
}
static const bsrnn_ctx::OvlTable* ovl_table(const bsrnn_ctx* c, const Flow& f, int C, int T, hipStream_t s)
{
    if (!f.overlap || !c->d_ovl) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s && hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }      // (the legacy default stream cannot be captured)
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    auto it = c->ovl_tables.find(std::make_pair(C, T));
    return it == c->ovl_tables.end() ? nullptr : &it->second;
}

// The model proper for a single part on one stream.
int run_model(bsrnn_ctx* c, const float* Xf, float* Yf, float* tap, int C, int T,
              const float* state_in, float* state_out, hipStream_t s, const int* row_frames)
{
    Part p = make_part(c, 0, C, T, s);
    p.row_frames = row_frames;
    p.f = plan_call(c, C, T, true, true);
    if (int rc = ensure_ovl(c, p.f, C, T)) return rc;
    p.Xf = Xf; p.Yf = Yf; p.tap = tap;
    p.state_in = state_in; p.state_out = state_out;
    p.state_slab = state_slab_floats(C, c->K);
    const bsrnn_ctx::OvlTable* tb = ovl_table(c, p.f, C, T, s);
    if (tb) run_overlapped(c, p, tb, MS_BANDSPLIT, MS_MASK);
    else
    for (int st = MS_BANDSPLIT; st <= MS_MASK; ++st) run_stage(c, p, st);
    if (c->stage_error) { c->stage_error = false; return fail(BSRNN_ESTATE, "no task table for %d frame rows (internal error)", C * T); }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The guard word the fp16x2 kernels set, read and cleared (the host-mapped word: the caller has waited for the kernels it means).
int take_guard(bsrnn_ctx* c)
{
    if (!c->h_range) return 0;
    const int v = *(volatile int*)c->h_range;
    if (v) *(volatile int*)c->h_range = 0;
    return v;
}
// The guard values that are not about the fp16 range (1): 3 = a time-axis launch gave up waiting on its own workgroup-local counters
// (internal error); 4 = the band-pair launch's partner workgroups did not meet (placement / dispatch order not as assumed); 5 = a consumer
// of the overlapped dual path gave up waiting for the time-axis launch beside it.  4 and 5 switch the context for good to the flow
// without that assumption (same arithmetic: one launch per layer / launch after launch; ++gen re-captures streaming graphs, which contain
// the old flow).  Returns BSRNN_EHIP with the message for 3, 4 and 5 - `who` names the call whose results are invalid -, else 0.
int guard_fallback(bsrnn_ctx* c, int v, const char* who)
{
    if (v == 3) return fail(BSRNN_EHIP, "%s: a time-axis LSTM launch gave up waiting on its own workgroup-local counters (internal error)", who);
    if (v != 4 && v != 5) return 0;
    (v == 4 ? c->band_pair_off : c->overlap_off) = true;
    ++c->gen;
    return fail(BSRNN_EHIP, v == 4 ? "%s: a band-axis launch (both layers in one launch) did not find its partner workgroups on the same XCD in time; "
                                     "its results are invalid - repeat the call (the context now runs one launch per layer)"
                                   : "%s: a consumer workgroup of the overlapped dual path gave up waiting for the time-axis launch beside it; its "
                                     "results are invalid - repeat the call (the context now runs launch after launch)", who);
}
int check_range(bsrnn_ctx* c)
{
    const int v = take_guard(c);
    if (!v) return 0;
    if (int rc = guard_fallback(c, v, "an earlier call (range policy 'deferred')")) return rc;
    return fail(BSRNN_ERANGE, "an earlier call (range policy 'deferred') fed the fp16x2 matrix path an activation beyond +-65504; its "
                              "results are invalid - repeat it under the default policy, rescale the input or set BSRNN_GEMM=f32 BSRNN_LSTM=f32");
}
// The opening of every compute entry point: a context that can compute, on its device.  model: the entry points that run the committed
// model say which of the two it is, need the weights, and report a range violation that an earlier call left behind.
int check_device(bsrnn_ctx* c, bool model)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (c->device < 0 || c->zombie)
        return fail(BSRNN_ESTATE, !model ? "context cannot compute (host-only or destroyed)"
                                         : (c->device < 0 ? "host-only context (device -1): no compute entry points" : "context was destroyed"));
    if (model && !c->committed) return fail(BSRNN_ESTATE, "bsrnn_commit_params() has not been called");
    HIP_TRY(hipSetDevice(c->device));
    return model ? check_range(c) : 0;
}
int check_ready(bsrnn_ctx* c) { return check_device(c, true); }

static thread_local bsrnn_ctx* tl_owner = nullptr;
CallGuard::CallGuard(bsrnn_ctx* c_) : c(c_), ok(true), outer(false)
{
    if (!c || tl_owner == c) return;
    int expect = 0;
    ok = c->busy.compare_exchange_strong(expect, 1);
    if (ok) { outer = true; tl_owner = c; }
}
CallGuard::~CallGuard() { if (outer) { tl_owner = nullptr; c->busy.store(0); } }
int CallGuard::refuse() const { return fail(BSRNN_ESTATE, "context is in use by a call from another host thread (one call at a time per context)"); }
// The context has one workspace: work enqueued by the previous call on ANOTHER stream must have finished before this
// call's kernels may touch it.  Same stream (the normal case): stream order does it, nothing to do here.
int order_after_last(bsrnn_ctx* c, hipStream_t s)
{
    if (c->have_last && c->last_stream != s) { HIP_TRY(hipStreamSynchronize(c->last_stream)); if (int rcj = ovl_join_host(c)) return rcj; }
    c->last_stream = s; c->have_last = true;
    return 0;
}

void destroy_now(bsrnn_ctx* c)
{
    if (c->device < 0) { delete c; return; }
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (auto& r : c->pool) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (int j = 0; j < MAX_PARTS; ++j) {
        if (c->aux[j]) (void)hipStreamDestroy(c->aux[j]);
        if (c->ev_join[j]) (void)hipEventDestroy(c->ev_join[j]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->lf.copy) (void)hipStreamDestroy(c->lf.copy);
    for (int k = 0; k < 2; ++k)
        for (hipEvent_t e : {c->lf.ev_h2d[k], c->lf.ev_comp[k], c->lf.ev_d2h[k]})
            if (e) (void)hipEventDestroy(e);
    if (c->lf.state[0]) (void)hipFree(c->lf.state[0]);
    if (c->lf.d_base) (void)hipFree(c->lf.d_base);
    if (c->lf.h_base) (void)hipHostFree(c->lf.h_base);
    c->rg.release();
    c->er.table.release();
    if (c->er.d_part) (void)hipFree(c->er.d_part);
    if (c->er.h_part) (void)hipHostFree(c->er.h_part);
    if (c->er.d_est) (void)hipFree(c->er.d_est);
    for (auto& t : c->rs_tables) (void)hipFree(t.d);
    if (c->cv.X) (void)hipFree(c->cv.X);
    if (c->cv.Y) (void)hipFree(c->cv.Y);
    if (c->ev_ovl_fork) (void)hipEventDestroy(c->ev_ovl_fork);
    if (c->ev_ovl_join) (void)hipEventDestroy(c->ev_ovl_join);
    free_ovl_tables(c);
    if (c->d_ovl) (void)hipFree(c->d_ovl);
    if (c->ev_ovl_mid) (void)hipEventDestroy(c->ev_ovl_mid);
    if (c->d_ws) (void)hipFree(c->d_ws);
    if (c->d_tap) (void)hipFree(c->d_tap);
    if (c->d_arena) (void)hipFree(c->d_arena);
    if (c->d_jobs) (void)hipFree(c->d_jobs);
    if (c->d_tiles) (void)hipFree(c->d_tiles);
    for (int ch = 0; ch < 2; ++ch)
        if (c->d_chain[ch]) (void)hipFree(c->d_chain[ch]);
    free_chain_tasks(c);
    if (c->d_tables) (void)hipFree(c->d_tables);
    if (c->d_cs_tables) (void)hipFree(c->d_cs_tables);
    if (c->d_train_ws) (void)hipFree(c->d_train_ws);
    for (float* p : c->train_ws_retired) (void)hipFree(p);
    for (void* p : c->retired) (void)hipFree(p);
    if (c->d_colmap) (void)hipFree(c->d_colmap);
    if (c->h_range) (void)hipHostFree(c->h_range);
    delete c;
}
// Scratch of the training entry points: one grow-only buffer per context.  Calls on a context are serialised (ENTER_CALL) and a
// stream switch waits for the previous stream, so reuse in stream order is safe; growing synchronises the device once.
float* train_scratch(bsrnn_ctx* c, size_t floats)
{
    if (floats <= c->train_ws_floats) return c->d_train_ws;
    // Grow: the old buffer is RETIRED, not freed.  Kernel nodes of a captured training iteration hold its address; a later, larger
    // clip (its eager warm-up or an eager fall-back clip) must not turn those graphs into writers of freed memory.  A retired
    // buffer stays valid scratch for the graphs that know it (they are replayed one at a time, in stream order, like every call).
    float* fresh = nullptr;
    const size_t want = floats + floats / 4;
    if (hipMalloc((void**)&fresh, want * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (c->d_train_ws) c->train_ws_retired.push_back(c->d_train_ws);
    c->d_train_ws = fresh;
    c->train_ws_floats = want;
    return c->d_train_ws;
}

}  // namespace bsrnn::host

// =========================================================================== ABI
extern "C" {

int bsrnn_abi_version(void) { return BSRNN_ABI_VERSION; }
const char* bsrnn_last_error(void) { return g_err; }
const char* bsrnn_compute_mode(void)
{
    static char buf[64];
    const int g = gemm_mode(), l = lstm_mode();
    snprintf(buf, sizeof buf, "gemm=%s lstm=%s", g == GEMM_F32 ? "f32" : (g == GEMM_FP16X2 ? "fp16x2" : (g == GEMM_BF16 ? "bf16" : "fp16")),
             l == LSTM_F32 ? "f32" : "fp16x2");
    return buf;
}

int bsrnn_create(int device, const int32_t* widths, int32_t n_bands, bsrnn_ctx** out)
{
    if (!out || !widths || n_bands < 1 || n_bands > 256) return fail(BSRNN_EARG, "bad band table");
    int sum = 0;
    for (int i = 0; i < n_bands; ++i) {
        if (widths[i] < 0) return fail(BSRNN_EARG, "negative band width");
        sum += widths[i];
    }
    if (sum != NBINS) return fail(BSRNN_EARG, "band widths sum to %d, expected %d", sum, NBINS);
    if (device != -1) {
        int ndev = 0;
        HIP_TRY(hipGetDeviceCount(&ndev));
        if (device < 0 || device >= ndev) return fail(BSRNN_EARG, "device %d out of range (%d devices)", device, ndev);
        HIP_TRY(hipSetDevice(device));
    }
    bsrnn_ctx* c = new bsrnn_ctx();
    c->device = device;
    c->K = n_bands;
    c->widths.assign(widths, widths + n_bands);
    int pos = 0;
    for (int i = 0; i < n_bands; ++i) { c->off.push_back(pos); pos += widths[i]; }
    const BandColumns bc = band_columns(c->widths);
    c->aoff = bc.aoff; c->poff = bc.poff; c->LDA = bc.LDA; c->LDP = bc.LDP;
    build_inventory(c);
    memset(c->acc_ms, 0, sizeof c->acc_ms);
    memset(c->acc_n, 0, sizeof c->acc_n);
    if (device == -1) { *out = c; return 0; }     // host-only: inventory, set / get, weight-file validation
    {   // range-guard word: pinned host memory the fp16x2 kernels can set and the host can read without a sync
        hipError_t e = hipHostMalloc((void**)&c->h_range, sizeof(int), hipHostMallocMapped);
        if (e == hipSuccess) { *c->h_range = 0; e = hipHostGetDevicePointer((void**)&c->d_range, c->h_range, 0); }
        if (e != hipSuccess) { c->h_range = nullptr; c->d_range = nullptr; (void)hipGetLastError(); }
    }
    if (const char* e = getenv("BSRNN_OVERLAP")) {
        c->overlap_env = strcmp(e, "0") != 0; c->overlap_sabotage = !strcmp(e, "timeout");
    }
    if (const char* e = getenv("BSRNN_OVL_EPOCHS")) c->ovl_epoch_period = std::max(2, std::min(1 << 18, atoi(e)));

    // FFT tables in double precision
    std::vector<float> t(2 * 1024 + 2 * 1025 + 2048 + 1024 + 1024 + 16);
    size_t o = 0;
    const double PI = 3.14159265358979323846;
    size_t o_tw1 = o;
    for (int k = 0; k < 1024; ++k) { t[o++] = (float)cos(2 * PI * k / 1024); t[o++] = (float)(-sin(2 * PI * k / 1024)); }
    size_t o_tw2 = o;
    for (int k = 0; k <= 1024; ++k) { t[o++] = (float)cos(2 * PI * k / 2048); t[o++] = (float)(-sin(2 * PI * k / 2048)); }
    o = (o + 3) & ~size_t(3);
    size_t o_hann = o;
    std::vector<float> w(2048);
    for (int i = 0; i < 2048; ++i) { w[i] = (float)(0.5 - 0.5 * cos(2 * PI * i / 2048)); t[o++] = w[i]; }
    size_t o_env = o;
    for (int i = 0; i < 1024; ++i) {     // torch.istft envelope: overlap-add of window^2 (float), inverted
        const float e = w[i] * w[i] + w[i + 1024] * w[i + 1024];
        t[o++] = 1.0f / e;
    }
    size_t o_ws = o;
    for (int i = 0; i < 1024; ++i) t[o++] = 1.0f / (w[i] + w[i + 1024]);
    hipError_t e = hipMalloc((void**)&c->d_tables, o * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(c->d_tables, t.data(), o * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { delete c; return fail(BSRNN_EHIP, "table upload: %s", hipGetErrorString(e)); }
    c->tb.tw1024 = (const float2*)(c->d_tables + o_tw1);
    c->tb.tw2048 = (const float2*)(c->d_tables + o_tw2);
    c->tb.hann = c->d_tables + o_hann;
    c->tb.inv_env = c->d_tables + o_env;
    c->tb.inv_wsum = c->d_tables + o_ws;
    {   // bin -> column of its real part in the band-padded spectrum layout
        std::vector<int> cm(NBINS);
        for (int i = 0; i < n_bands; ++i)
            for (int k = 0; k < widths[i]; ++k) cm[c->off[i] + k] = c->poff[i] + 2 * k;
        e = hipMalloc((void**)&c->d_colmap, NBINS * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(c->d_colmap, cm.data(), NBINS * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) { delete c; return fail(BSRNN_EHIP, "table upload: %s", hipGetErrorString(e)); }
        c->tb.colmap = c->d_colmap;
        c->tb.ld = c->LDP;
    }
    *out = c;
    return 0;
}

void bsrnn_destroy(bsrnn_ctx* c)
{
    if (!c) return;
    // streams hold a pointer to their context (and a captured graph holds the context's buffers): with streams alive the
    // context only stops accepting calls here and is freed when the last of them is destroyed
    if (c->live_streams > 0) { c->zombie = true; return; }
    destroy_now(c);
}

int bsrnn_n_bands(const bsrnn_ctx* c) { return c ? c->K : -1; }
int bsrnn_mlp_fused(const bsrnn_ctx* c) { return c ? (c->fused ? 1 : 0) : -1; }
int bsrnn_chain_geometry(const bsrnn_ctx* c, int32_t chain, int32_t band, int32_t out[6])
{
    if (!c || !out || (chain != CHAIN_SPLIT && chain != CHAIN_MASK) || band < 0 || band >= c->K)
        return fail(BSRNN_EARG, "bsrnn_chain_geometry: bad arguments");
    if (c->device < 0 || !c->committed) return fail(BSRNN_ESTATE, "bsrnn_chain_geometry: no committed device context");
    const int v = !c->fused ? -1 : 0;
    for (int i = 0; i < 6; ++i) out[i] = v;
    if (!c->fused || c->widths[band] == 0) return 0;
    for (const ChainDesc& d : c->h_chain[chain]) {
        if (d.constant || d.z_off != band * HID) continue;
        chain_geometry_answer(d, out);
        return 0;
    }
    return fail(BSRNN_ESTATE, "bsrnn_chain_geometry: band %d has no descriptor in chain %d", band, chain);
}
int bsrnn_device(const bsrnn_ctx* c) { return c ? c->device : -1; }
int bsrnn_debug_peek(bsrnn_ctx* c, int32_t which, float* host_out, int64_t nfloats)
{
    if (!c || !host_out || nfloats < 0 || which < 0 || which > 4) return fail(BSRNN_EARG, "bsrnn_debug_peek: bad arguments");
    if (c->device < 0 || !c->d_ws) return fail(BSRNN_ESTATE, "bsrnn_debug_peek: no workspace yet");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t KH = (size_t)c->K * HID;
    const float* src[5] = {c->Z0, c->Z1, c->HB1, c->P, c->Yf};
    const size_t cap[5] = {c->cap_rows * KH, c->cap_rows * KH, c->cap_rows * KH * 2, c->cap_rows * c->LDP, c->cap_rows * c->LDP};
    if ((size_t)nfloats > cap[which]) return fail(BSRNN_EARG, "bsrnn_debug_peek: the buffer holds %zu floats", cap[which]);
    HIP_TRY(hipMemcpy(host_out, src[which], (size_t)nfloats * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}
long long bsrnn_debug_counter(int32_t which) { return which >= 0 && which < 5 ? g_dbg[which].load() : -1; }
int bsrnn_overlap_state(const bsrnn_ctx* c) { return !c ? -1 : (c->overlap_off ? 2 : (c->overlap_env ? 1 : 0)); }
int bsrnn_set_range_policy(bsrnn_ctx* c, int32_t policy)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (policy != BSRNN_RANGE_EXACT && policy != BSRNN_RANGE_DEFERRED) return fail(BSRNN_EARG, "bsrnn_set_range_policy: unknown policy %d", policy);
    c->range_policy = policy;
    return 0;
}
int bsrnn_get_range_policy(const bsrnn_ctx* c) { return c ? c->range_policy : -1; }
int bsrnn_param_count(const bsrnn_ctx* c) { return c ? (int)c->params.size() : -1; }

int bsrnn_param_info(const bsrnn_ctx* c, int32_t i, const char** key, int64_t* d0, int64_t* d1, int32_t* ndim)
{
    if (!c || i < 0 || i >= (int)c->params.size()) return fail(BSRNN_EARG, "param index out of range");
    const Param& p = c->params[i];
    if (key) *key = p.key.c_str();
    if (d0) *d0 = p.d0;
    if (d1) *d1 = p.d1;
    if (ndim) *ndim = p.ndim;
    return 0;
}

int bsrnn_set_param(bsrnn_ctx* c, const char* key, const float* host, int64_t numel)
{
    if (!c || !key) return fail(BSRNN_EARG, "null argument");
    auto it = c->index.find(key);
    if (it == c->index.end()) return fail(BSRNN_ENOKEY, "unexpected key '%s'", key);
    Param& p = c->params[it->second];
    if (numel != p.numel()) return fail(BSRNN_EARG, "size mismatch for %s: got %lld, expected %lld", key, (long long)numel, (long long)p.numel());
    if (numel > 0 && !host) return fail(BSRNN_EARG, "null data for %s", key);
    p.data.assign(host, host + numel);
    p.set = true;
    c->committed = false;
    return 0;
}

int bsrnn_get_param(const bsrnn_ctx* c, const char* key, float* out, int64_t numel)
{
    if (!c || !key) return fail(BSRNN_EARG, "null argument");
    auto it = c->index.find(key);
    if (it == c->index.end()) return fail(BSRNN_ENOKEY, "unexpected key '%s'", key);
    const Param& p = c->params[it->second];
    if (!p.set) return fail(BSRNN_ESTATE, "%s was never set", key);
    if (numel != p.numel()) return fail(BSRNN_EARG, "size mismatch for %s", key);
    if (numel) memcpy(out, p.data.data(), numel * sizeof(float));
    return 0;
}

int bsrnn_commit_params(bsrnn_ctx* c)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    for (const Param& p : c->params)
        if (!p.set) return fail(BSRNN_ESTATE, "missing key '%s'", p.key.c_str());
    if (c->device < 0) return 0;          // host-only context: the inventory is complete, there is nothing to upload
    CallGuard guard_(c);
    if (!guard_.ok) return guard_.refuse();
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    ++c->gen;                             // the arena is rebuilt: captured streaming graphs hold pointers into the old one

    // BSRNN_MLP and the two class knobs are read at every commit, the ragged split and the GEMM mode once per process
    static const bool rag_on = [] { const char* e = getenv("BSRNN_CHAIN_RAG"); return !(e && !strcmp(e, "0")); }();
    const char* mlp = getenv("BSRNN_MLP");
    const CommitKnobs knobs = {gemm_mode(), mlp && !strcmp(mlp, "layers"), getenv("BSRNN_CHAIN_NO48") != nullptr, getenv("BSRNN_CHAIN_NO80") != nullptr, rag_on};
    const WeightImage im = build_weight_image([c](const std::string& key) -> const std::vector<float>& { return c->params[c->index.at(key)].data; },
                                              c->widths, c->aoff, c->poff, knobs);
    c->slots = im.slots;

    // upload: the arena first, then the descriptors with the arena's device address added to their offsets
    if (c->d_arena) { HIP_TRY(hipFree(c->d_arena)); c->d_arena = nullptr; }
    if (c->d_jobs) { HIP_TRY(hipFree(c->d_jobs)); c->d_jobs = nullptr; }
    if (c->d_tiles) { HIP_TRY(hipFree(c->d_tiles)); c->d_tiles = nullptr; }
    HIP_TRY(hipMalloc((void**)&c->d_arena, (im.arena.size() + 4) * sizeof(float)));
    HIP_TRY(hipMemcpy(c->d_arena, im.arena.data(), im.arena.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<GemmJob> jobs;
    for (const JobRec& r : im.jobs) {
        jobs.push_back(r.j);
        jobs.back().W = c->d_arena + r.w; jobs.back().bias = c->d_arena + r.b; jobs.back().Wp = c->d_arena + r.wp;
    }
    HIP_TRY(hipMalloc((void**)&c->d_jobs, jobs.size() * sizeof(GemmJob)));
    HIP_TRY(hipMemcpy(c->d_jobs, jobs.data(), jobs.size() * sizeof(GemmJob), hipMemcpyHostToDevice));
    static_assert(sizeof(GemmTile) == sizeof(int2) && alignof(GemmTile) <= alignof(int2), "the kernels read a GemmTile as an int2");
    HIP_TRY(hipMalloc((void**)&c->d_tiles, im.tiles.size() * sizeof(int2)));
    HIP_TRY(hipMemcpy(c->d_tiles, im.tiles.data(), im.tiles.size() * sizeof(int2), hipMemcpyHostToDevice));
    c->fused = false;
    free_chain_tasks(c);
    for (int ch = 0; ch < 2; ++ch) {
        c->h_chain[ch].clear();
        if (c->d_chain[ch]) { HIP_TRY(hipFree(c->d_chain[ch])); c->d_chain[ch] = nullptr; }
        if (!im.fused) continue;
        std::vector<ChainDesc> descs;
        for (const ChainRec& r : im.chains[ch]) {
            descs.push_back(r.d);
            descs.back().wstream = c->d_arena + r.w; descs.back().bias = c->d_arena + r.b;
        }
        HIP_TRY(hipMalloc((void**)&c->d_chain[ch], descs.size() * sizeof(ChainDesc)));
        HIP_TRY(hipMemcpy(c->d_chain[ch], descs.data(), descs.size() * sizeof(ChainDesc), hipMemcpyHostToDevice));
        c->h_chain[ch] = descs;
    }
    c->fused = im.fused;
    for (int blk = 0; blk < 2; ++blk) {
        const BlockSegs& s = im.blk[blk];
        const struct { const float** member; size_t off; } segs[] = {
            {&c->bandW[blk][0], s.bandW[0]}, {&c->bandW[blk][1], s.bandW[1]}, {&c->bandB[blk][0], s.bandB[0]}, {&c->bandB[blk][1], s.bandB[1]},
            {&c->bandW16[blk][0], s.bandW16[0]}, {&c->bandW16[blk][1], s.bandW16[1]}, {&c->bandFc16[blk], s.bandFc16}, {&c->bandFcB[blk], s.bandFcB},
            {&c->timeW[blk], s.timeW}, {&c->timeB[blk], s.timeB}, {&c->timeW16[blk], s.timeW16}, {&c->timeFc16[blk], s.timeFc16}, {&c->timeFcB[blk], s.timeFcB}};
        for (const auto& sg : segs) *sg.member = c->d_arena + sg.off;
    }
    c->committed = true;
    return 0;
}

int bsrnn_load_weights_file(bsrnn_ctx* c, const char* path)
{
    if (!c || !path) return fail(BSRNN_EARG, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(BSRNN_EIO, "cannot open %s", path);
    auto bad = [&](const char* why) { fclose(f); return fail(BSRNN_EIO, "%s: %s", path, why); };
    // Nothing in the file is trusted: every tensor is looked up in the inventory FIRST and must have exactly the
    // inventory's rank and dimensions (not just the element count: a transposed matrix has the same count) before a byte
    // of it is read, so sizes never come from the file; nothing may throw across the C ABI (the LADSPA host would terminate).
    try {
        char magic[8];
        uint32_t nb = 0, nt = 0;
        if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "BSRNNW01", 8)) return bad("bad magic");
        if (fread(&nb, 4, 1, f) != 1 || (int)nb != c->K) return bad("band count differs from the context's table");
        for (uint32_t i = 0; i < nb; ++i) {
            uint32_t w;
            if (fread(&w, 4, 1, f) != 1 || (int)w != c->widths[i]) return bad("band table differs from the context's table");
        }
        if (fread(&nt, 4, 1, f) != 1) return bad("truncated");
        if (nt > c->params.size()) return bad("more tensors than the model has parameters");
        std::vector<float> buf;
        std::string key;
        for (uint32_t t = 0; t < nt; ++t) {
            uint32_t kl = 0, nd = 0;
            if (fread(&kl, 4, 1, f) != 1 || kl > 256) return bad("bad key length");
            key.resize(kl);
            if (kl && fread(&key[0], 1, kl, f) != kl) return bad("truncated key");
            auto it = c->index.find(key);
            if (it == c->index.end()) { fclose(f); return fail(BSRNN_ENOKEY, "%s: unexpected key '%s'", path, key.c_str()); }
            const Param& p = c->params[it->second];
            if (fread(&nd, 4, 1, f) != 1 || (int)nd != p.ndim) return bad(("rank of '" + key + "' differs from the model's").c_str());
            uint64_t dims[2] = {0, 0};
            for (uint32_t d = 0; d < nd; ++d)
                if (fread(&dims[d], 8, 1, f) != 1) return bad("truncated dims");
            if (dims[0] != (uint64_t)p.d0 || (nd == 2 && dims[1] != (uint64_t)p.d1))
                return bad(("shape of '" + key + "' differs from the model's").c_str());
            const size_t n = (size_t)p.numel();
            buf.resize(n);
            if (n && fread(buf.data(), 4, n, f) != n) return bad("truncated data");
            int rc = bsrnn_set_param(c, key.c_str(), buf.data(), (int64_t)n);
            if (rc) { fclose(f); return rc; }
        }
    } catch (...) {
        return bad("out of memory or malformed file");
    }
    fclose(f);
    return bsrnn_commit_params(c);
}

// --------------------------------------------------------------------------- I/O signature (the exported ONNX file's)
int bsrnn_io_count(void) { return 4; }
int bsrnn_io_info(const bsrnn_ctx* c, int32_t index, int32_t C, const char** name, int32_t* is_input, int64_t dims[4], int32_t* ndim)
{
    static const char* const kNames[4] = {"x.0", "state.0", "y.0", "new_state.0"};      // infer-streaming.py:74 (torch.onnx.export naming)
    if (!c || index < 0 || index >= 4 || C < 1 || !dims || !ndim) return fail(BSRNN_EARG, "bsrnn_io_info: bad arguments");
    if (name) *name = kNames[index];
    if (is_input) *is_input = index < 2;
    if (index & 1) { dims[0] = 4; dims[1] = 2; dims[2] = (int64_t)C * c->K; dims[3] = HID; *ndim = 4; }
    else { dims[0] = C; dims[1] = F2; dims[2] = dims[3] = 0; *ndim = 2; }
    return 0;
}

// --------------------------------------------------------------------------- model entry points
int bsrnn_forward(bsrnn_ctx* c, const float* x, float* y, float* mask, int32_t C, int32_t T, void* stream)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if (!x || !y || C < 1 || T < 1) return fail(BSRNN_EARG, "bsrnn_forward: bad arguments (C=%d, T=%d)", C, T);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const size_t M = (size_t)C * T;
    if ((rc = ensure_ws(c, M)) || (rc = ensure_tasks(c, (int)M))) return rc;
    if (mask && (rc = ensure_tap(c, M))) return rc;
    // The re-run (finish_call) starts from the frame-major copy Xf of the first run, which nothing in run_model writes: y and mask
    // may overlap x (an in-place call) and the re-run still sees the caller's input.
    auto run = [&](bool layout) -> int {
        if (layout) { StageScope sc(c, ST_LAYOUT, s); launch_to_frame_major(c->tb, x, c->Xf, C, T, s); }
        if (int rc2 = run_model(c, c->Xf, c->Yf, mask ? c->d_tap : nullptr, C, T, nullptr, nullptr, s)) return rc2;
        {
            StageScope sc(c, ST_LAYOUT, s);
            launch_from_frame_major(c->tb, c->Yf, y, C, T, s);
            if (mask) launch_from_frame_major(c->tb, c->d_tap, mask, C, T, s);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = run(true))) return rc;
    return finish_call(c, s, [&]() -> int { return run(false); });
}

int bsrnn_forward_chunk(bsrnn_ctx* c, const float* x, const float* state_in, float* y, float* state_out,
                        int32_t C, int32_t L, void* stream)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if (!x || !y || !state_in || !state_out || C < 1 || L < 1) return fail(BSRNN_EARG, "bsrnn_forward_chunk: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const size_t M = (size_t)C * L;
    if ((rc = ensure_ws(c, M)) || (rc = ensure_tasks(c, (int)M))) return rc;
    // The re-run reads state_in again (and x through its frame-major copy Xf, as bsrnn_forward): no output may overlap state_in.
    const size_t ns = state_floats(C, c->K) * sizeof(float), ny = (size_t)C * F2 * L * sizeof(float);
    if (c->range_policy == BSRNN_RANGE_EXACT && (ranges_overlap(state_in, ns, state_out, ns) || ranges_overlap(state_in, ns, y, ny)))
        return fail(BSRNN_EARG, "bsrnn_forward_chunk: state_out and y must not overlap state_in (a call that leaves the fp16 range is run again from state_in)");
    auto run = [&](bool layout) -> int {
        if (layout) { StageScope sc(c, ST_LAYOUT, s); launch_to_frame_major(c->tb, x, c->Xf, C, L, s); }
        if (int rc2 = run_model(c, c->Xf, c->Yf, nullptr, C, L, state_in, state_out, s)) return rc2;
        { StageScope sc(c, ST_LAYOUT, s); launch_from_frame_major(c->tb, c->Yf, y, C, L, s); }
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = run(true))) return rc;
    return finish_call(c, s, [&]() -> int { return run(false); });
}

int bsrnn_forward_recurrent(bsrnn_ctx* c, const float* x, const float* state_in, float* y, float* state_out,
                            int32_t C, void* stream)
{
    return bsrnn_forward_chunk(c, x, state_in, y, state_out, C, 1, stream);
}

int bsrnn_dual_path(bsrnn_ctx* c, const float* z, float* z_out, const float* state_in, float* state_out,
                    int32_t C, int32_t T, void* stream)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if (!z || !z_out || C < 1 || T < 1) return fail(BSRNN_EARG, "bsrnn_dual_path: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int M = C * T, K = c->K;
    if ((rc = ensure_ws(c, M))) return rc;
    const size_t nz = (size_t)M * K * HID;
    // The re-run copies z in again and reads state_in again: neither may overlap an output of the call.
    const size_t bz = nz * sizeof(float), bs = state_floats(C, K) * sizeof(float);
    if (c->range_policy == BSRNN_RANGE_EXACT &&
        (ranges_overlap(z, bz, z_out, bz) || ranges_overlap(z, bz, state_out, bs) ||
         ranges_overlap(state_in, bs, z_out, bz) || ranges_overlap(state_in, bs, state_out, bs)))
        return fail(BSRNN_EARG, "bsrnn_dual_path: z_out and state_out must not overlap z or state_in (a call that leaves the fp16 range is run again from them)");
    // the recurrent stages of run_stage on one part (never on the GEMV kernels)
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(c->Z0, z, nz * sizeof(float), hipMemcpyDeviceToDevice, s));
        Part p = make_part(c, 0, C, T, s);
        p.f = plan_call(c, C, T, false, false);
        p.state_in = state_in; p.state_out = state_out;
        p.state_slab = state_slab_floats(C, K);
        for (int st = MS_BAND0; st <= MS_TIMEFC1; ++st) run_stage(c, p, st);
        HIP_TRY(hipMemcpyAsync(z_out, c->Z0, nz * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = run())) return rc;
    return finish_call(c, s, run);
}

// --------------------------------------------------------------------------- training step, part 1: recurrent layers
// nn.LSTM of NormRNNResidual (bsrnn.py:66-72) forward with saves and backward through time (lstm_train.hip); what
// loss.backward() runs for these layers in train.py:97-115.  Operands are the caller's device buffers (torch layouts);
// nothing of the committed inference weights is used.

static int train_args_ok(bsrnn_ctx* c, int32_t N, int32_t L, int32_t IN, int32_t ndir, const char* who)
{
    if (int rc0 = check_device(c)) return rc0;
    if (N < 1 || L < 1 || (IN != HID && IN != 2 * HID) || ndir < 1 || ndir > 2 || (int64_t)N * L > (int64_t)1 << 30)
        return fail(BSRNN_EARG, "%s: need N, L >= 1, IN = 64 | 128, ndir = 1 | 2 (got N=%d L=%d IN=%d ndir=%d)", who, N, L, IN, ndir);
    return 0;
}

int bsrnn_lstm_train_forward(bsrnn_ctx* c, const float* x, const float* w_ih, const float* w_hh, const float* bias, float* h,
                             float* gates, float* cells, int32_t N, int32_t L, int32_t IN, int32_t ndir, void* stream)
{
    int rc = train_args_ok(c, N, L, IN, ndir, "bsrnn_lstm_train_forward");
    if (rc) return rc;
    if (!x || !w_ih || !w_hh || !bias || !h || !gates || !cells) return fail(BSRNN_EARG, "bsrnn_lstm_train_forward: null argument");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    launch_lstm_train_forward(x, w_ih, w_hh, bias, h, gates, cells, N, L, IN, ndir, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_lstm_train_backward(bsrnn_ctx* c, const float* x, const float* h, const float* gates, const float* cells, const float* dh,
                              const float* w_ih, const float* w_hh, float* dx, float* dw_ih, float* dw_hh, float* db,
                              int32_t N, int32_t L, int32_t IN, int32_t ndir, void* stream)
{
    int rc = train_args_ok(c, N, L, IN, ndir, "bsrnn_lstm_train_backward");
    if (rc) return rc;
    if (!x || !h || !gates || !cells || !dh || !w_ih || !w_hh || !dw_ih || !dw_hh || !db)
        return fail(BSRNN_EARG, "bsrnn_lstm_train_backward: null argument (only dx may be null)");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    // workspace in stream order: gate gradients of every (sequence, step, direction) + the partial sums of the reductions
    const size_t n_dg = (size_t)N * L * ndir * 256, n_scr = lstm_train_scratch_floats(N, L, IN, ndir);
    float* ws = train_scratch(c, n_dg + n_scr);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_lstm_train_backward: out of device memory (%zu MB of workspace)", (n_dg + n_scr) * sizeof(float) >> 20);
    launch_lstm_train_backward(x, h, gates, cells, dh, w_ih, w_hh, ws, ws + n_dg, dx, dw_ih, dw_hh, db, N, L, IN, ndir, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_train_reduction_layout(int32_t M, int32_t N1, int32_t N2, int32_t out[2])
{
    if (!out || M < 1 || M > (1 << 30) || N1 < 1 || N1 > 65536 || N2 < 1 || N2 > 65536)
        return fail(BSRNN_EARG, "bsrnn_train_reduction_layout: bad arguments (M=%d N1=%d N2=%d)", M, N1, N2);
    int o[2];
    train_reduction_layout(M, N1, N2, o);
    out[0] = o[0]; out[1] = o[1];
    return 0;
}

int bsrnn_adamw_step(bsrnn_ctx* c, float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                     float eps, float weight_decay, int32_t step, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!p || !g || !m || !v || n < 0 || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(BSRNN_EARG, "bsrnn_adamw_step: bad arguments (n=%lld step=%d)", (long long)n, step);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    launch_adamw(p, g, m, v, (size_t)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), s);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int adamw_multi(bsrnn_ctx* c, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* sizes,
                       int32_t n_tensors, float lr, double beta1, double beta2, float eps, float weight_decay, int32_t step, float* state,
                       void* stream, const char* who)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!p || !g || !m || !v || !sizes || n_tensors < 1 || (!state && step < 1) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return fail(BSRNN_EARG, "%s: bad arguments (n_tensors=%d step=%d)", who, n_tensors, step);
    for (int i = 0; i < n_tensors; ++i)
        if (!p[i] || !g[i] || !m[i] || !v[i] || sizes[i] < 0) return fail(BSRNN_EARG, "%s: tensor %d: null pointer or negative size", who, i);
    for (int i = 0; i < n_tensors; ++i)
        if (sizes[i] >= ((int64_t)1 << 31) - 1024) return fail(BSRNN_EARG, "%s: tensor %d has %lld elements (limit 2^31)", who, i, (long long)sizes[i]);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    double bc1 = 1.0, bc2 = 1.0;
    if (state) launch_adamw_tick(state, beta1, beta2, s);
    else { bc1 = 1.0 - pow(beta1, step); bc2 = 1.0 - pow(beta2, step); }
    for (int i0 = 0; i0 < n_tensors; i0 += ADAM_GROUP) {
        AdamGroup a;
        a.count = std::min(ADAM_GROUP, n_tensors - i0);
        a.first_block[0] = 0;
        for (int j = 0; j < a.count; ++j) {
            a.p[j] = p[i0 + j]; a.g[j] = g[i0 + j]; a.m[j] = m[i0 + j]; a.v[j] = v[i0 + j];
            a.n[j] = (int)sizes[i0 + j];
            a.first_block[j + 1] = a.first_block[j] + (a.n[j] + 1023) / 1024;
        }
        launch_adamw_group(a, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), s, state);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_adamw_step_multi(bsrnn_ctx* c, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* sizes,
                           int32_t n_tensors, float lr, double beta1, double beta2, float eps, float weight_decay, int32_t step, void* stream)
{
    return adamw_multi(c, p, g, m, v, sizes, n_tensors, lr, beta1, beta2, eps, weight_decay, step, nullptr, stream, "bsrnn_adamw_step_multi");
}

int bsrnn_adamw_step_multi_dev(bsrnn_ctx* c, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* sizes,
                               int32_t n_tensors, float* state_dev, double beta1, double beta2, float eps, float weight_decay, void* stream)
{
    if (!state_dev) return fail(BSRNN_EARG, "bsrnn_adamw_step_multi_dev: null optimizer state");
    return adamw_multi(c, p, g, m, v, sizes, n_tensors, 0.f, beta1, beta2, eps, weight_decay, 0, state_dev, stream, "bsrnn_adamw_step_multi_dev");
}

int bsrnn_linear_train_forward(bsrnn_ctx* c, const float* x, int32_t ldx, const float* w, const float* b, float* y, int32_t ldy,
                               int32_t M, int32_t K, int32_t N, int32_t leaky, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!x || !w || !b || !y || M < 1 || K < 1 || N < 1 || ldx < K || ldy < N)
        return fail(BSRNN_EARG, "bsrnn_linear_train_forward: bad arguments (M=%d K=%d N=%d ldx=%d ldy=%d)", M, K, N, ldx, ldy);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    launch_linear_train_forward(x, ldx, w, b, y, ldy, M, K, N, leaky != 0, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_linear_train_backward(bsrnn_ctx* c, const float* x, int32_t ldx, const float* w, const float* y, int32_t ldy,
                                const float* dy, int32_t lddy, float* dx, int32_t lddx, float* dw, float* db,
                                int32_t M, int32_t K, int32_t N, int32_t leaky, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!x || !w || !dy || !dw || !db || (leaky && !y) || M < 1 || K < 1 || N < 1 || ldx < K || lddy < N || (leaky && ldy < N) || (dx && lddx < K))
        return fail(BSRNN_EARG, "bsrnn_linear_train_backward: bad arguments (M=%d K=%d N=%d)", M, K, N);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const size_t n_scr = linear_train_scratch_floats(M, K, N, leaky != 0);
    float* ws = train_scratch(c, n_scr);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_linear_train_backward: out of device memory (%zu MB of workspace)", n_scr * sizeof(float) >> 20);
    launch_linear_train_backward(x, ldx, w, y, ldy, dy, lddy, dx, lddx, dw, db, ws, M, K, N, leaky != 0, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The same Linear layer of several bands (or any layers that share the row count M) in grouped launches: arrays [n] per field.
int bsrnn_linear_group_train_forward(bsrnn_ctx* c, int32_t n, const float* const* x, const int32_t* ldx, const float* const* w,
                                     const float* const* b, float* const* y, const int32_t* ldy, const int32_t* K, const int32_t* N,
                                     int32_t M, int32_t leaky, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (n < 1 || n > 4096 || !x || !ldx || !w || !b || !y || !ldy || !K || !N || M < 1) return fail(BSRNN_EARG, "bsrnn_linear_group_train_forward: bad arguments");
    std::vector<LinearJob> jobs((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!x[i] || !w[i] || !b[i] || !y[i] || K[i] < 1 || N[i] < 1 || ldx[i] < K[i] || ldy[i] < N[i])
            return fail(BSRNN_EARG, "bsrnn_linear_group_train_forward: job %d: bad arguments (K=%d N=%d ldx=%d ldy=%d)", i, K[i], N[i], ldx[i], ldy[i]);
        LinearJob& j = jobs[i];
        memset(&j, 0, sizeof j);
        j.x = x[i]; j.ldx = ldx[i]; j.w = w[i]; j.b = b[i]; j.y = y[i]; j.ldy = ldy[i]; j.K = K[i]; j.N = N[i];
    }
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    launch_linear_group_forward(jobs.data(), n, M, leaky != 0, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_linear_group_train_backward(bsrnn_ctx* c, int32_t n, const float* const* x, const int32_t* ldx, const float* const* w,
                                      const float* const* y, const int32_t* ldy, const float* const* dy, const int32_t* lddy,
                                      float* const* dx, const int32_t* lddx, float* const* dw, float* const* db,
                                      const int32_t* K, const int32_t* N, int32_t M, int32_t leaky, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (n < 1 || n > 4096 || !x || !ldx || !w || !dy || !lddy || !dx || !lddx || !dw || !db || !K || !N || M < 1 || (leaky && (!y || !ldy)))
        return fail(BSRNN_EARG, "bsrnn_linear_group_train_backward: bad arguments");
    std::vector<LinearJob> jobs((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (!x[i] || !w[i] || !dy[i] || !dw[i] || !db[i] || K[i] < 1 || N[i] < 1 || ldx[i] < K[i] || lddy[i] < N[i] || (dx[i] && lddx[i] < K[i]) ||
            (leaky && (!y[i] || ldy[i] < N[i])))
            return fail(BSRNN_EARG, "bsrnn_linear_group_train_backward: job %d: bad arguments (K=%d N=%d)", i, K[i], N[i]);
        LinearJob& j = jobs[i];
        memset(&j, 0, sizeof j);
        j.x = x[i]; j.ldx = ldx[i]; j.w = w[i]; j.y = leaky ? const_cast<float*>(y[i]) : nullptr; j.ldy = leaky ? ldy[i] : 0;
        j.dy = dy[i]; j.lddy = lddy[i]; j.dx = dx[i]; j.lddx = lddx[i]; j.dw = dw[i]; j.db = db[i]; j.K = K[i]; j.N = N[i];
    }
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const size_t n_scr = linear_group_scratch_floats(jobs.data(), n, M, leaky != 0);
    float* ws = train_scratch(c, n_scr);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_linear_group_train_backward: out of device memory (%zu MB of workspace)", n_scr * sizeof(float) >> 20);
    launch_linear_group_backward(jobs.data(), n, M, leaky != 0, ws, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// --------------------------------------------------------------------------- STFT sandwich
int bsrnn_stft(bsrnn_ctx* c, const float* wave, float* x, int32_t R, int64_t n, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!wave || !x || R < 1 || n <= NFFT / 2) return fail(BSRNN_EARG, "bsrnn_stft: need n > 1024 samples (reflect padding), got %lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int T = 1 + (int)(n / HOPS);
    int rc = ensure_ws(c, (size_t)R * T);
    if (rc) return rc;
    { StageScope sc(c, ST_STFT, s); launch_stft(c->tb, wave, c->Xf, R, n, T, s); }
    { StageScope sc(c, ST_LAYOUT, s); launch_from_frame_major(c->tb, c->Xf, x, R, T, s); }
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_istft(bsrnn_ctx* c, const float* y, float* wave_out, int32_t R, int32_t T, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!y || !wave_out || R < 1 || T < 2) return fail(BSRNN_EARG, "bsrnn_istft: need T >= 2 frames");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    int rc = ensure_ws(c, (size_t)R * T);
    if (rc) return rc;
    { StageScope sc(c, ST_LAYOUT, s); launch_to_frame_major(c->tb, y, c->Yf, R, T, s); }
    {
        StageScope sc(c, ST_ISTFT, s);
        launch_istft(c->tb, c->Yf, wave_out, R, T, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_istft_backward(bsrnn_ctx* c, const float* dwave, float* dy, int32_t R, int32_t T, void* stream)
{
    if (int rc0 = check_device(c)) return rc0;
    if (!dwave || !dy || R < 1 || T < 2) return fail(BSRNN_EARG, "bsrnn_istft_backward: need T >= 2 frames");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    int rc = ensure_ws(c, (size_t)R * T);
    if (rc) return rc;
    float* ws = train_scratch(c, (size_t)R * (T - 1) * HOPS);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_istft_backward: out of device memory");
    launch_istft_backward(c->tb, dwave, ws, c->Yf, R, T, s);
    launch_from_frame_major(c->tb, c->Yf, dy, R, T, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_separate(bsrnn_ctx* c, const float* wave, float* wave_out, int32_t R, int64_t n, void* stream)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if (!wave || !wave_out || R < 1 || n <= NFFT / 2) return fail(BSRNN_EARG, "bsrnn_separate: need n > 1024 samples, got %lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int T = 1 + (int)(n / HOPS);
    if ((rc = ensure_ws(c, (size_t)R * T))) return rc;
    const int64_t out_len = (int64_t)(T - 1) * HOPS;
    // the re-run (finish_call) reads the waveform again; concurrent row blocks write their outputs while others still read
    if (c->range_policy == BSRNN_RANGE_EXACT &&
        ranges_overlap(wave, (size_t)R * n * sizeof(float), wave_out, (size_t)R * out_len * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_separate: wave_out must not overlap wave (a call that leaves the fp16 range is run again from wave)");

    // The batch as concurrent row blocks on separate streams (how many, and which rows: row_block_count, plan_host.h).
    // Part j starts one stage behind part j-1 so that they sit in different stages.
    const Flow whole = plan_call(c, R, T, false, true);
    const int parts = row_block_count(R, T, whole.nwg, device_cus());
    const RowBlocks rb = row_blocks(R, T, parts);
    if (parts > 1 && (rc = ensure_streams(c, parts))) return rc;
    Part pt[MAX_PARTS];
    // task tables of every row block of this call, made before any launch: one call never evicts a table it needs itself
    if ((rc = ensure_tasks(c, rb.ms, parts))) return rc;
    if (parts == 1 && (rc = ensure_ovl(c, whole, R, T))) return rc;
    for (int j = 0; j < parts; ++j) {
        const int r0 = rb.r0[j];
        pt[j] = make_part(c, r0, rb.r0[j + 1] - r0, T, parts > 1 ? c->aux[j] : s, j);
        if (j && row_blocks_share_flags(rb, T, j))
            return fail(BSRNN_ESTATE, "row blocks %d and %d would share a hand-over flag pair (internal error)", j - 1, j);
        pt[j].wave = wave + (size_t)r0 * n; pt[j].n = n;
        pt[j].wave_out = wave_out + (size_t)r0 * out_len;
    }
    auto run = [&]() -> int {
        for (int j = 0; j < parts; ++j) pt[j].f = plan_call(c, pt[j].C, T, false, parts == 1);
        if (parts > 1) {
            HIP_TRY(hipEventRecord(c->ev_fork, s));
            for (int j = 0; j < parts; ++j) HIP_TRY(hipStreamWaitEvent(c->aux[j], c->ev_fork, 0));
        }
        const bsrnn_ctx::OvlTable* tb = parts == 1 ? ovl_table(c, pt[0].f, R, T, s) : nullptr;
        if (tb) run_overlapped(c, pt[0], tb, MS_STFT, MS_ISTFT);      // the dual path overlapped on the context's auxiliary stream
        for (int step = 0; !tb && step < MS_COUNT + parts - 1; ++step)
            for (int j = 0; j < parts; ++j) {
                const int st = step - j;
                if (st >= 0 && st < MS_COUNT) run_stage(c, pt[j], st);
            }
        if (parts > 1)
            for (int j = 0; j < parts; ++j) {
                HIP_TRY(hipEventRecord(c->ev_join[j], c->aux[j]));
                HIP_TRY(hipStreamWaitEvent(s, c->ev_join[j], 0));
            }
        if (c->stage_error) { c->stage_error = false; return fail(BSRNN_ESTATE, "no task table for a row block of this call (internal error)"); }
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = run())) return rc;
    return finish_call(c, s, run);
}

// --------------------------------------------------------------------------- ragged batches: rows of different lengths in one call
// The model is causal along time, its band-axis blocks see one frame at a time and rows are independent: frames t < T_r of row r do not
// depend on what frames t >= T_r of that row, or any other row, hold.  So the call is bsrnn_separate on the rectangle R x Tmax with the two
// DSP ends told the rows' lengths (fft.hip: the padded frames go in as zero rows, the padded hops come out as zeros); every stage between
// them runs as for a rectangular call, the overlapped dual path included.

// What every ragged entry point refuses about its rows' lengths (q = ragged_shape(lens, R, stride)) and its clips (q = clip_shape(...)),
// under the caller's name.  seg_frames: the long form counts the frame rows of one segment.
static int ragged_shape_refuse(const char* who, const RaggedShape& q, int R, int64_t stride, int seg_frames = 0)
{
    if (q.why == RAGGED_SHORT) return fail(BSRNN_EARG, "%s: row %d has %lld samples, need more than 1024 (reflect padding)", who, q.bad_row, (long long)q.bad_len);
    if (q.why == RAGGED_LONG) return fail(BSRNN_EARG, "%s: row %d has %lld samples, more than the row stride of %lld", who, q.bad_row, (long long)q.bad_len, (long long)stride);
    const int64_t frames = seg_frames ? std::min<int64_t>(seg_frames, q.Tmax) : q.Tmax;
    if (ragged_too_many(R, frames))
        return fail(BSRNN_EARG, "%s: %d rows x %lld frames is too many frame rows for one %s", who, R, (long long)frames, seg_frames ? "segment" : "call");
    return 0;
}
static int clip_shape_refuse(const char* who, const ClipShape& q, int64_t stride)
{
    if (q.why == CLIPS_ROWS) return fail(BSRNN_EARG, "%s: clip %d has %lld rows, need at least 1", who, q.bad_clip, (long long)q.bad_value);
    if (q.why == CLIPS_SHORT) return fail(BSRNN_EARG, "%s: clip %d has %lld samples, need more than 1024 (reflect padding)", who, q.bad_clip, (long long)q.bad_value);
    if (q.why == CLIPS_LONG) return fail(BSRNN_EARG, "%s: clip %d has %lld samples, more than the row stride of %lld", who, q.bad_clip, (long long)q.bad_value, (long long)stride);
    if (q.why == CLIPS_MANY) return fail(BSRNN_EARG, "%s: %lld rows x %lld frames is too many frame rows for one call", who, (long long)q.R, (long long)q.Tmax);
    return 0;
}

// This call's block for R rows of M = R * Tmax frame rows, copied in on stream s; where its parts are on the device.
static int ragged_upload(bsrnn_ctx* c, const int64_t* lens, int R, int M, hipStream_t s, Part& p)
{
    std::vector<ChainTask> tk[2];
    const size_t b_lens = (size_t)R * sizeof(int64_t);
    size_t off[2], bytes = b_lens;
    for (int ch = 0; ch < 2; ++ch) {
        if (c->fused) build_chain_tasks(c->h_chain[ch], M, tk[ch]);
        off[ch] = bytes;
        bytes += (tk[ch].size() + 1) * sizeof(int2);                  // (one entry of slack, as upload_table's)
    }
    const int rc = c->rg.upload(bytes, s, [&](char* h) {
        memcpy(h, lens, b_lens);
        for (int ch = 0; ch < 2; ++ch) {
            memcpy(h + off[ch], tk[ch].data(), tk[ch].size() * sizeof(int2));
            memset(h + off[ch] + tk[ch].size() * sizeof(int2), 0, sizeof(int2));
        }
    });
    if (rc) return rc;
    const char* d = c->rg.d;
    p.lens = reinterpret_cast<const int64_t*>(d);
    for (int ch = 0; ch < 2; ++ch) {
        p.tasks[ch] = c->fused ? reinterpret_cast<const int2*>(d + off[ch]) : nullptr;
        p.n_tasks[ch] = (int)tk[ch].size();
    }
    return 0;
}
// The lengths alone, for the calls that run no model stage (the ragged DSP and loss calls of a training step need no chain task tables)
static int ragged_upload_lens(bsrnn_ctx* c, const int64_t* lens, int R, hipStream_t s, const int64_t** d_lens)
{
    const size_t b_lens = (size_t)R * sizeof(int64_t);
    if (int rc = c->rg.upload(b_lens, s, [&](char* h) { memcpy(h, lens, b_lens); })) return rc;
    *d_lens = reinterpret_cast<const int64_t*>(c->rg.d);
    return 0;
}

int bsrnn_separate_ragged(bsrnn_ctx* c, const float* wave, int64_t wave_stride, const int64_t* lens_host, float* wave_out, int32_t R, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!wave || !lens_host || !wave_out || R < 1)
        return fail(BSRNN_EARG, "bsrnn_separate_ragged: need a waveform, R lengths, an output buffer and R >= 1, got R = %d", R);
    const RaggedShape q = ragged_shape(lens_host, R, wave_stride);
    if (int rc0 = ragged_shape_refuse("bsrnn_separate_ragged", q, R, wave_stride)) return rc0;
    // the re-run (finish_call) reads the waveform again
    if (c->range_policy == BSRNN_RANGE_EXACT &&
        ranges_overlap(wave, (size_t)R * wave_stride * sizeof(float), wave_out, (size_t)R * q.out_stride * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_separate_ragged: wave_out must not overlap wave (a call that leaves the fp16 range is run again from wave)");
    int rc = check_ready(c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int T = (int)q.Tmax;
    if ((rc = ensure_ws(c, (size_t)R * T))) return rc;
    if ((rc = ensure_ovl(c, plan_call(c, R, T, false, true), R, T))) return rc;
    // one row block (the two concurrent row blocks of bsrnn_separate for R >= 128 are not reproduced, as in bsrnn_separate_long)
    Part p = make_part(c, 0, R, T, s);
    p.wave = wave; p.wave_stride = wave_stride;
    p.wave_out = wave_out; p.out_stride = q.out_stride;
    if ((rc = ragged_upload(c, lens_host, R, R * T, s, p))) return rc;
    // a re-run sees the same lengths: the block on the device is not touched before the next call
    auto run = [&]() -> int {
        p.f = plan_call(c, R, T, false, true);
        const bsrnn_ctx::OvlTable* tb = ovl_table(c, p.f, R, T, s);
        if (tb) run_overlapped(c, p, tb, MS_STFT, MS_ISTFT);
        else
            for (int st = 0; st < MS_COUNT; ++st) run_stage(c, p, st);
        if (c->stage_error) { c->stage_error = false; return fail(BSRNN_ESTATE, "no task table for this call (internal error)"); }
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = run())) return rc;
    return finish_call(c, s, run);
}

// --------------------------------------------------------------------------- ragged training step: the DSP ends and the loss told the lengths
// The clips of one optimizer step as one rectangle R x Tmax through the training kernels: x = 0 in the padded frames and y = x * mask, so
// those frames carry neither value nor gradient, and between the two DSP ends the step runs as for a rectangular batch.  What knows the
// lengths: the ragged analysis and synthesis at the [R, 2050, Tmax] boundary autograd works on, the synthesis' transpose, and the loss, whose
// means and gradients are per clip.  None of these calls waits for the device; each uploads its lengths (the loss calls their clip table)
// through the context's block, in stream order.
static_assert(TV_LOSS == BSRNN_TV_LOSS && TV_L1_TIME == BSRNN_TV_L1_TIME && TV_L1_RE == BSRNN_TV_L1_RE && TV_L1_IM == BSRNN_TV_L1_IM &&
              TV_SDR == BSRNN_TV_SDR && TV_COUNT == BSRNN_N_TRAIN_VALUES, "train_ragged_host.h");

// The argument checks the three DSP calls share (stride: what a length may not exceed; INT64_MAX where rows have no input stride)
static int ragged_dsp_check(const char* who, const bsrnn_ctx* c, bool have_buffers, const int64_t* lens, int R, int64_t stride, RaggedShape& q)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!have_buffers || !lens || R < 1) return fail(BSRNN_EARG, "%s: need both buffers, R lengths and R >= 1, got R = %d", who, R);
    q = ragged_shape(lens, R, stride);
    return ragged_shape_refuse(who, q, R, stride);
}

int bsrnn_stft_ragged(bsrnn_ctx* c, const float* wave, int64_t wave_stride, const int64_t* lens_host, float* x, int32_t R, void* stream)
{
    RaggedShape q;
    if (int rc0 = ragged_dsp_check("bsrnn_stft_ragged", c, wave && x, lens_host, R, wave_stride, q)) return rc0;
    if (int rc0 = check_device(c)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int T = (int)q.Tmax;
    if (int rc = ensure_ws(c, (size_t)R * T)) return rc;
    const int64_t* d_lens = nullptr;
    if (int rc = ragged_upload_lens(c, lens_host, R, s, &d_lens)) return rc;
    { StageScope sc(c, ST_STFT, s); launch_stft_ragged(c->tb, wave, wave_stride, d_lens, c->Xf, R, T, s); }
    { StageScope sc(c, ST_LAYOUT, s); launch_from_frame_major(c->tb, c->Xf, x, R, T, s); }
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_istft_ragged(bsrnn_ctx* c, const float* y, const int64_t* lens_host, float* wave_out, int32_t R, void* stream)
{
    RaggedShape q;
    if (int rc0 = ragged_dsp_check("bsrnn_istft_ragged", c, y && wave_out, lens_host, R, INT64_MAX, q)) return rc0;
    if (int rc0 = check_device(c)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int T = (int)q.Tmax;
    if (int rc = ensure_ws(c, (size_t)R * T)) return rc;
    const int64_t* d_lens = nullptr;
    if (int rc = ragged_upload_lens(c, lens_host, R, s, &d_lens)) return rc;
    { StageScope sc(c, ST_LAYOUT, s); launch_to_frame_major(c->tb, y, c->Yf, R, T, s); }
    { StageScope sc(c, ST_ISTFT, s); launch_istft_ragged(c->tb, c->Yf, wave_out, q.out_stride, d_lens, R, T, s); }
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_istft_ragged_backward(bsrnn_ctx* c, const float* dwave, const int64_t* lens_host, float* dy, int32_t R, void* stream)
{
    RaggedShape q;
    if (int rc0 = ragged_dsp_check("bsrnn_istft_ragged_backward", c, dwave && dy, lens_host, R, INT64_MAX, q)) return rc0;
    if (int rc0 = check_device(c)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int T = (int)q.Tmax;
    if (int rc = ensure_ws(c, (size_t)R * T)) return rc;
    float* ws = train_scratch(c, (size_t)R * q.out_stride);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_istft_ragged_backward: out of device memory");
    const int64_t* d_lens = nullptr;
    if (int rc = ragged_upload_lens(c, lens_host, R, s, &d_lens)) return rc;
    launch_istft_ragged_backward(c->tb, dwave, ws, c->Yf, d_lens, R, T, s);
    launch_from_frame_major(c->tb, c->Yf, dy, R, T, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The clip table of the two loss calls, checked and uploaded: [R int64 row lengths | n_clips TrainClip | R int32 row -> clip]
struct TrainTableDev { const int64_t* lens; const TrainClip* clips; const int32_t* row_clip; };
static int train_table_check(const char* who, const bsrnn_ctx* c, bool have_buffers, const int64_t* clip_lens, const int32_t* clip_rows, int n_clips,
                             int64_t wave_stride, TrainClipTable& t)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!have_buffers || !clip_lens || n_clips < 1)
        return fail(BSRNN_EARG, "%s: need every tensor, the clips' lengths and n_clips >= 1, got n_clips = %d", who, n_clips);
    t = train_clip_table(clip_lens, clip_rows, n_clips, wave_stride);
    return clip_shape_refuse(who, t.shape, wave_stride);
}
static int train_table_upload(bsrnn_ctx* c, const TrainClipTable& t, hipStream_t s, TrainTableDev& dv)
{
    const int64_t R = t.shape.R;
    const int n_clips = (int)t.clips.size();
    const int rc = c->rg.upload(train_table_bytes(R, n_clips), s, [&](char* h) {
        memcpy(h, t.row_lens.data(), (size_t)R * sizeof(int64_t));
        memcpy(h + train_table_clips_at(R), t.clips.data(), (size_t)n_clips * sizeof(TrainClip));
        memcpy(h + train_table_map_at(R, n_clips), t.row_clip.data(), (size_t)R * sizeof(int32_t));
    });
    if (rc) return rc;
    const char* d = c->rg.d;
    dv.lens = reinterpret_cast<const int64_t*>(d);
    dv.clips = reinterpret_cast<const TrainClip*>(d + train_table_clips_at(R));
    dv.row_clip = reinterpret_cast<const int32_t*>(d + train_table_map_at(R, n_clips));
    return 0;
}

int bsrnn_train_loss_ragged(bsrnn_ctx* c, const float* y, const float* sfreq, const float* xtime, const float* speech, int64_t wave_stride,
                            const int64_t* clip_lens_host, const int32_t* clip_rows_host, int32_t n_clips, double* values, double* row_sums,
                            void* stream)
{
    TrainClipTable t;
    if (int rc0 = train_table_check("bsrnn_train_loss_ragged", c, y && sfreq && xtime && speech && values && row_sums, clip_lens_host, clip_rows_host,
                                    n_clips, wave_stride, t))
        return rc0;
    if (int rc0 = check_device(c)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int R = (int)t.shape.R, T = (int)t.shape.Tmax;
    const size_t n_part = train_loss_partials(R, T);
    float* ws = train_scratch(c, 2 * n_part);                           // (doubles)
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_train_loss_ragged: out of device memory");
    TrainTableDev dv;
    if (int rc = train_table_upload(c, t, s, dv)) return rc;
    launch_train_loss_ragged(y, sfreq, xtime, speech, dv.lens, dv.clips, n_clips, R, T, wave_stride, reinterpret_cast<double*>(ws), values, row_sums, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_train_loss_ragged_backward(bsrnn_ctx* c, const float* y, const float* sfreq, const float* xtime, const float* speech, int64_t wave_stride,
                                     const int64_t* clip_lens_host, const int32_t* clip_rows_host, int32_t n_clips, const double* row_sums,
                                     const float* gclip, float* dy, float* dxtime, void* stream)
{
    TrainClipTable t;
    if (int rc0 = train_table_check("bsrnn_train_loss_ragged_backward", c, y && sfreq && xtime && speech && row_sums && gclip && dy && dxtime,
                                    clip_lens_host, clip_rows_host, n_clips, wave_stride, t))
        return rc0;
    if (int rc0 = check_device(c)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    TrainTableDev dv;
    if (int rc = train_table_upload(c, t, s, dv)) return rc;
    launch_train_loss_ragged_backward(y, sfreq, xtime, speech, dv.lens, dv.clips, dv.row_clip, gclip, row_sums, (int)t.shape.R, (int)t.shape.Tmax,
                                      wave_stride, dy, dxtime, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// --------------------------------------------------------------------------- long-form separation: the sandwich in segments
// A clip of T frames as consecutive segments of `seg` frames (the last one shorter): segment STFT -> run_model on R * L frame rows with
// the time-axis LSTM state carried (the model is causal along time; the band-axis blocks see one frame at a time) -> segment iSTFT with
// the overlap-add tail carried.  Workspace, task tables and carry are those of one segment.

static int ensure_long_carry(bsrnn_ctx* c, int R)
{
    bsrnn_ctx::LongForm& lf = c->lf;
    if (R <= lf.rows) return 0;
    const size_t nstate = state_floats(R, c->K), ncarry = (size_t)R * HOPS;
    float* p = nullptr;
    ++g_dbg[DBG_ALLOC];
    HIP_TRY(hipMalloc((void**)&p, 2 * (nstate + ncarry) * sizeof(float)));
    if (lf.state[0]) c->retired.push_back(lf.state[0]);           // (work of an earlier call may still read it: retired like the workspace)
    for (int k = 0; k < 2; ++k) { lf.state[k] = p; p += nstate; }
    for (int k = 0; k < 2; ++k) { lf.carry[k] = p; p += ncarry; }
    lf.rows = R;
    return 0;
}

// Staging of the host-buffer entry point for R rows and segments of `seg` frames (window and block sizes: plan_host.h); the caller has
// nothing of its own in flight on them (the entry point is synchronous).
static int ensure_long_staging(bsrnn_ctx* c, int R, int seg)
{
    bsrnn_ctx::LongForm& lf = c->lf;
    if (!lf.copy) { ++g_dbg[DBG_ALLOC]; HIP_TRY(hipStreamCreateWithFlags(&lf.copy, hipStreamNonBlocking)); }
    for (int k = 0; k < 2; ++k)
        for (hipEvent_t* e : {&lf.ev_h2d[k], &lf.ev_comp[k], &lf.ev_d2h[k]})
            if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    const size_t in = (size_t)R * staging_window_floats(seg), out = (size_t)R * staging_block_floats(seg);
    if (in <= lf.in_floats && out <= lf.out_floats) return 0;
    const size_t in_new = std::max(in, lf.in_floats), out_new = std::max(out, lf.out_floats);
    HIP_TRY(hipStreamSynchronize(lf.copy));
    if (lf.d_base) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(lf.d_base); (void)hipHostFree(lf.h_base); lf.d_base = lf.h_base = nullptr; lf.in_floats = lf.out_floats = 0; }
    const size_t bytes = 2 * (in_new + out_new) * sizeof(float);
    g_dbg[DBG_ALLOC] += 2;
    HIP_TRY(hipHostMalloc((void**)&lf.h_base, bytes, hipHostMallocDefault));
    hipError_t e = hipMalloc((void**)&lf.d_base, bytes);
    if (e != hipSuccess) { (void)hipHostFree(lf.h_base); lf.h_base = lf.d_base = nullptr; return fail(BSRNN_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
    for (int k = 0; k < 2; ++k) {
        lf.h_in[k] = lf.h_base + k * in_new; lf.d_in[k] = lf.d_base + k * in_new;
        lf.h_out[k] = lf.h_base + 2 * in_new + k * out_new; lf.d_out[k] = lf.d_base + 2 * in_new + k * out_new;
    }
    lf.in_floats = in_new; lf.out_floats = out_new;
    return 0;
}

// One segment from carry set p into set 1 - p (does not decide which set the next one reads: the caller does, once the segment is final).
// src / stride / base as launch_stft_segment's, out / out_stride as launch_istft_segment's.
static int long_segment_run(bsrnn_ctx* c, const float* src, int64_t stride, int64_t base, float* out, int64_t out_stride, int R, int64_t n, int ta,
                            int te, int p, hipStream_t s)
{
    bsrnn_ctx::LongForm& lf = c->lf;
    { StageScope sc(c, ST_STFT, s); launch_stft_segment(c->tb, src, stride, base, c->Xf, R, n, ta, te, s); }
    if (int rc = run_model(c, c->Xf, c->Yf, nullptr, R, te - ta, lf.state[p], lf.state[p ^ 1], s)) return rc;
    { StageScope sc(c, ST_ISTFT, s); launch_istft_segment(c->tb, c->Yf, out, out_stride, ta ? lf.carry[p] : nullptr, lf.carry[p ^ 1], R, te - ta, s); }
    HIP_TRY(hipGetLastError());
    return 0;
}

// All segments of a clip on stream s.  host = false: wave / wave_out are the whole clip and the whole result on the device.  host = true:
// they are host memory; segment i goes through staging block i & 1 (ensure_long_staging), its window copied in and its hops copied out on the
// copy stream beside the kernels of its neighbours:
//   host:  stage window i+1 (when H2D i-1 has left the pinned window), take block i-1 (when D2H i-1 is there)  - while segment i computes
//   copy:  H2D i+1 (after segment i-1, which read that mirror, is final) | D2H i (after segment i is final)
//   s:     segment i after H2D i, and after D2H i-2 (which read the mirror segment i writes)
// Same kernels, same order, same cut either way.
static int long_segments(bsrnn_ctx* c, const float* wave, float* wave_out, int R, int64_t n, int T, int seg, hipStream_t s, bool host)
{
    bsrnn_ctx::LongForm& lf = c->lf;
    const int nseg = (T + seg - 1) / seg;
    const int64_t out_len = (int64_t)(T - 1) * HOPS;
    auto stage_in = [&](int i) -> int {
        const SegmentCut q = segment_cut(n, T, seg, i);
        const int b = i & 1;
        if ((size_t)R * q.wl > lf.in_floats) return fail(BSRNN_ESTATE, "segment window larger than its staging block (internal error)");
        if (i >= 2) { HIP_TRY(hipEventSynchronize(lf.ev_h2d[b])); HIP_TRY(hipStreamWaitEvent(lf.copy, lf.ev_comp[b], 0)); }
        for (int r = 0; r < R; ++r) memcpy(lf.h_in[b] + (size_t)r * q.wl, wave + (size_t)r * n + q.lo, (size_t)q.wl * sizeof(float));
        HIP_TRY(hipMemcpyAsync(lf.d_in[b], lf.h_in[b], (size_t)R * q.wl * sizeof(float), hipMemcpyHostToDevice, lf.copy));
        HIP_TRY(hipEventRecord(lf.ev_h2d[b], lf.copy));
        return 0;
    };
    auto take_out = [&](int i) -> int {
        const SegmentCut q = segment_cut(n, T, seg, i);
        if (!q.nh) return 0;
        HIP_TRY(hipEventSynchronize(lf.ev_d2h[i & 1]));
        const size_t len = (size_t)q.nh * HOPS;
        for (int r = 0; r < R; ++r) memcpy(wave_out + (size_t)r * out_len + (size_t)q.hop0 * HOPS, lf.h_out[i & 1] + r * len, len * sizeof(float));
        return 0;
    };
    int rc;
    HIP_TRY(hipMemsetAsync(lf.state[0], 0, state_floats(R, c->K) * sizeof(float), s));      // the clip starts from zero state (and needs no carry)
    if (host && (rc = stage_in(0))) return rc;
    for (int i = 0; i < nseg; ++i) {
        const SegmentCut q = segment_cut(n, T, seg, i);
        const int b = i & 1;
        const float* src = wave;
        float* out = wave_out + (size_t)q.hop0 * HOPS;
        int64_t stride = n, base = 0, out_stride = out_len;
        if (host) {
            src = lf.d_in[b]; stride = q.wl; base = q.lo; out = lf.d_out[b]; out_stride = (int64_t)q.nh * HOPS;
            HIP_TRY(hipStreamWaitEvent(s, lf.ev_h2d[b], 0));
            if (i >= 2) HIP_TRY(hipStreamWaitEvent(s, lf.ev_d2h[b], 0));
        }
        auto run = [&]() -> int { return long_segment_run(c, src, stride, base, out, out_stride, R, n, q.ta, q.te, b, s); };
        if ((rc = run())) return rc;
        if (host) {
            if (i + 1 < nseg && (rc = stage_in(i + 1))) return rc;
            if (i >= 1 && (rc = take_out(i - 1))) return rc;
        }
        // range policy per segment, as for a block of stream hops: the re-run starts from this segment's untouched state and carry set
        if ((rc = finish_call(c, s, run))) return rc;
        if (host) {
            HIP_TRY(hipEventRecord(lf.ev_comp[b], s));
            HIP_TRY(hipStreamWaitEvent(lf.copy, lf.ev_comp[b], 0));
            if (q.nh) HIP_TRY(hipMemcpyAsync(lf.h_out[b], lf.d_out[b], (size_t)R * q.nh * HOPS * sizeof(float), hipMemcpyDeviceToHost, lf.copy));
            HIP_TRY(hipEventRecord(lf.ev_d2h[b], lf.copy));
        }
    }
    if (host) {
        if ((rc = take_out(nseg - 1))) return rc;
        HIP_TRY(hipStreamSynchronize(lf.copy));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}

// What both entry points need before their first launch: workspace and task tables of the (at most two) segment lengths, the carry sets.
static int long_prepare(bsrnn_ctx* c, int R, int T, int seg, const char* who)
{
    if ((int64_t)R * seg > INT32_MAX / 2) return fail(BSRNN_EARG, "%s: %d rows x %d frames is too many frame rows for one segment", who, R, seg);
    int rc, ms[2];
    if ((rc = ensure_ws(c, (size_t)R * seg))) return rc;
    if ((rc = ensure_tasks(c, ms, long_frame_rows(R, T, seg, ms)))) return rc;
    return ensure_long_carry(c, R);
}
// What both entry points check before anything else (who: the entry point's name).  The overlap is refused whatever the range policy:
// the clip's reflected tail (and every later segment) is read after early hops have been written.
static int long_check(bsrnn_ctx* c, const float* wave, float* wave_out, int R, int64_t n, int seg_frames, const char* who)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!wave || !wave_out || R < 1 || n <= NFFT / 2)
        return fail(BSRNN_EARG, "%s: need two buffers, R >= 1 and n > 1024 samples, got R = %d, n = %lld", who, R, (long long)n);
    if (seg_frames < 1) return fail(BSRNN_EARG, "%s: seg_frames = %d (at least one frame per segment)", who, seg_frames);
    if (int rc = check_ready(c)) return rc;
    const int T = 1 + (int)(n / HOPS);
    if (ranges_overlap(wave, (size_t)R * n * sizeof(float), wave_out, (size_t)R * (T - 1) * HOPS * sizeof(float)))
        return fail(BSRNN_EARG, "%s: wave_out must not overlap wave (later segments read the waveform after earlier hops are written)", who);
    return 0;
}

int bsrnn_separate_long(bsrnn_ctx* c, const float* wave, float* wave_out, int32_t R, int64_t n, int32_t seg_frames, void* stream)
{
    int rc = long_check(c, wave, wave_out, R, n, seg_frames, "bsrnn_separate_long");
    if (rc) return rc;
    const int T = 1 + (int)(n / HOPS);
    if (seg_frames >= T) return bsrnn_separate(c, wave, wave_out, R, n, stream);       // one segment IS the one-shot call: bit-identical by construction
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if ((rc = long_prepare(c, R, T, seg_frames, "bsrnn_separate_long"))) return rc;
    return long_segments(c, wave, wave_out, R, n, T, seg_frames, s, false);
}

int bsrnn_separate_long_host(bsrnn_ctx* c, const float* wave_host, float* wave_out_host, int32_t R, int64_t n, int32_t seg_frames)
{
    int rc = long_check(c, wave_host, wave_out_host, R, n, seg_frames, "bsrnn_separate_long_host");
    if (rc) return rc;
    const int T = 1 + (int)(n / HOPS);
    const size_t out_floats = (size_t)R * (T - 1) * HOPS;
    hipStream_t s = nullptr;
    ENTER_CALL(c, s);
    const int seg = std::min<int>(seg_frames, T);
    if ((int64_t)R * seg > INT32_MAX / 2) return fail(BSRNN_EARG, "bsrnn_separate_long_host: %d rows x %d frames is too many frame rows for one segment", R, seg);
    if ((rc = ensure_long_staging(c, R, seg))) return rc;
    bsrnn_ctx::LongForm& lf = c->lf;
    if (seg_frames >= T) {       // one segment: the one-shot call on the staged clip (R * n <= R * (T + 1) * 1024 floats: it fits a window)
        memcpy(lf.h_in[0], wave_host, (size_t)R * n * sizeof(float));
        HIP_TRY(hipMemcpyAsync(lf.d_in[0], lf.h_in[0], (size_t)R * n * sizeof(float), hipMemcpyHostToDevice, s));
        if ((rc = bsrnn_separate(c, lf.d_in[0], lf.d_out[0], R, n, s))) return rc;
        HIP_TRY(hipMemcpyAsync(lf.h_out[0], lf.d_out[0], out_floats * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        memcpy(wave_out_host, lf.h_out[0], out_floats * sizeof(float));
        return 0;
    }
    if ((rc = long_prepare(c, R, T, seg, "bsrnn_separate_long_host"))) return rc;
    return long_segments(c, wave_host, wave_out_host, R, n, T, seg, s, true);
}

// --------------------------------------------------------------------------- ragged long-form: rows of different lengths in segments
// bsrnn_separate_ragged's batch cut like bsrnn_separate_long's clip, and both arguments hold together: the model is causal along time, the
// band-axis blocks and the per-band MLPs see one frame at a time, rows are independent.  Segment i runs the model on the alive prefix of
// the rows (plan_host.h: ragged_long_plan) - a row that has ended is absent from later segments, one inside the prefix is carried as zero
// frames - so the model sees about the real frames, rounded up to a segment per row, from a workspace of R x seg frame rows.  Carry sets as
// long_segments': segment i reads set p and writes set p ^ 1, and p flips when the segment is final.  When the prefix shrinks, the next
// segment's state has another slab pitch: the surviving rows' state and overlap-add tail are packed from the written set into the one the
// finished segment read (launch_long_compact, on the caller's stream), and p does NOT flip - so a segment always reads a set that nothing
// of its own writes, and its range re-run (finish_call) starts from untouched state and carry.
// The segments of such a call on stream s, after its arguments have been checked (T = q.shape.Tmax > seg).  `out` takes the hops segment i
// completes: whole = true, it is the call's result, rows out_stride floats apart, and the segment writes from its first hop on; whole =
// false, it is a buffer of one segment and every segment writes from its start.  any_policy: the range guard is handled per segment whatever
// the context's policy (finish_call).  after(ta, te, Ri, d_lens, seg_out) runs once per segment, when the segment is final - its estimate at
// seg_out (its first hop of row 0), its spectrum in Yf, Xf free - and before the next one starts.
typedef std::function<int(int ta, int te, int Ri, const int64_t* d_lens, const float* seg_out)> AfterSegment;
static int long_ragged_segments(bsrnn_ctx* c, const RaggedLongPlan& q, const float* wave, int64_t wave_stride, const int64_t* lens_host, float* out,
                                int64_t out_stride, bool whole, int R, int seg, hipStream_t s, bool any_policy, const AfterSegment& after)
{
    int rc;
    const int T = (int)q.shape.Tmax, K = c->K;
    // everything the segments need, before the first launch: the workspace of one segment, the task tables and (where a segment's plan
    // overlaps the dual path) the dispatch orders of every distinct shape rows[i] x frames, the carry sets.  The caches' bounds grow so
    // that this call's set fits beside what is there (as bsrnn_stream_reserve's).
    if ((rc = ensure_ws(c, (size_t)R * seg))) return rc;
    std::vector<std::pair<int, int>> shapes;
    for (int i = 0; i < q.nseg; ++i) {
        const std::pair<int, int> sh(q.rows[i], std::min(T, (i + 1) * seg) - i * seg);
        if (std::find(shapes.begin(), shapes.end(), sh) == shapes.end()) shapes.push_back(sh);
    }
    size_t missing = 0, ovl_missing = 0;
    for (int m : q.ms) missing += c->fused && c->chain_tasks.find(m) == c->chain_tasks.end();
    for (const auto& sh : shapes)
        ovl_missing += plan_call(c, sh.first, sh.second, true, true).overlap && c->ovl_tables.find(sh) == c->ovl_tables.end();
    c->task_cap = std::max(c->task_cap, c->chain_tasks.size() + missing);
    c->ovl_cap = std::max(c->ovl_cap, c->ovl_tables.size() + ovl_missing + 1);
    if ((rc = ensure_tasks(c, q.ms.data(), (int)q.ms.size()))) return rc;
    for (const auto& sh : shapes)
        if ((rc = ensure_ovl(c, plan_call(c, sh.first, sh.second, true, true), sh.first, sh.second))) return rc;
    if ((rc = ensure_long_carry(c, R))) return rc;
    // the lengths go up once, in front of the first segment (the block's task tables stay empty: the segments find theirs in the cache)
    Part lp = make_part(c, 0, R, 1, s);
    if ((rc = ragged_upload(c, lens_host, R, 0, s, lp))) return rc;
    const int64_t* d_lens = lp.lens;

    bsrnn_ctx::LongForm& lf = c->lf;
    HIP_TRY(hipMemsetAsync(lf.state[0], 0, state_floats(R, K) * sizeof(float), s));       // every clip starts from zero state (and needs no carry)
    int p = 0;
    for (int i = 0; i < q.nseg; ++i) {
        const int ta = i * seg, te = std::min(T, ta + seg), Ri = q.rows[i];
        float* seg_out = whole ? out + (size_t)std::max(ta - 1, 0) * HOPS : out;
        auto run = [&]() -> int {
            { StageScope sc(c, ST_STFT, s); launch_stft_ragged_segment(c->tb, wave, wave_stride, d_lens, c->Xf, Ri, ta, te, s); }
            if (int rc2 = run_model(c, c->Xf, c->Yf, nullptr, Ri, te - ta, lf.state[p], lf.state[p ^ 1], s)) return rc2;
            {
                StageScope sc(c, ST_ISTFT, s);
                launch_istft_ragged_segment(c->tb, c->Yf, seg_out, out_stride, d_lens, ta ? lf.carry[p] : nullptr, lf.carry[p ^ 1], R, Ri, ta, te, s);
            }
            HIP_TRY(hipGetLastError());
            return 0;
        };
        if ((rc = run())) return rc;
        g_dbg[DBG_LONG_RAGGED_ROWS] += (long long)Ri * (te - ta);
        // range policy per segment, as in long_segments: the re-run starts from this segment's untouched state and carry set
        if ((rc = finish_call(c, s, run, any_policy))) return rc;
        if ((rc = after(ta, te, Ri, d_lens, seg_out))) return rc;
        if (i + 1 < q.nseg && q.rows[i + 1] < Ri) {
            launch_long_compact(lf.state[p ^ 1], lf.state[p], lf.carry[p ^ 1], lf.carry[p], Ri, q.rows[i + 1], K, s);
            HIP_TRY(hipGetLastError());
        } else p ^= 1;
    }
    return 0;
}

int bsrnn_separate_long_ragged(bsrnn_ctx* c, const float* wave, int64_t wave_stride, const int64_t* lens_host, float* wave_out, int32_t R,
                               int32_t seg_frames, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!wave || !lens_host || !wave_out || R < 1)
        return fail(BSRNN_EARG, "bsrnn_separate_long_ragged: need a waveform, R lengths, an output buffer and R >= 1, got R = %d", R);
    if (seg_frames < 1) return fail(BSRNN_EARG, "bsrnn_separate_long_ragged: seg_frames = %d (at least one frame per segment)", seg_frames);
    const RaggedLongPlan q = ragged_long_plan(lens_host, R, wave_stride, seg_frames);
    if (int rc0 = ragged_shape_refuse("bsrnn_separate_long_ragged", q.shape, R, wave_stride, seg_frames)) return rc0;
    // whatever the range policy: later segments read the waveform after earlier hops are written
    const int64_t out_stride = q.shape.out_stride;
    if (ranges_overlap(wave, (size_t)R * wave_stride * sizeof(float), wave_out, (size_t)R * out_stride * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_separate_long_ragged: wave_out must not overlap wave (later segments read the waveform after earlier hops are written)");
    if (seg_frames >= q.shape.Tmax) {                                 // one segment IS the ragged call: bit-identical by construction
        const int rc1 = bsrnn_separate_ragged(c, wave, wave_stride, lens_host, wave_out, R, stream);
        if (!rc1) g_dbg[DBG_LONG_RAGGED_ROWS] += q.frame_rows;
        return rc1;
    }
    int rc = check_ready(c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    return long_ragged_segments(c, q, wave, wave_stride, lens_host, wave_out, out_stride, true, R, seg_frames, s, false,
                                [](int, int, int, const int64_t*, const float*) { return 0; });
}

int64_t bsrnn_workspace_rows(const bsrnn_ctx* c) { return c ? (int64_t)c->cap_rows : 0; }

// --------------------------------------------------------------------------- validation metrics: the eight numbers per clip
// m_dataset.py:182-226 (`infer` + `train_infer` without the discriminator) and infer.py:44-47.  A clip is the unit of the reference's
// metrics (one `sample`: all rows of one file, one length; validate.py and train.py:132-150 average per-clip numbers): the reference's
// `sdr2` sums over the rows of its own clip, which all have one length, and nothing is summed across clips.  The three entry points are
// views of one arithmetic - bsrnn_evaluate: one clip of R rows, a rectangle; bsrnn_evaluate_ragged: clips of different lengths;
// bsrnn_evaluate_long_ragged: the same in segments - and share one tail: the table [row lengths | clips] goes up through er.table, one
// family of metric kernels (metrics.hip) leaves its sums in er.d_part, ONE download, and metrics_host.h turns them into the numbers per
// clip in a fixed order.  No call has a round trip in its middle (alpha of the SI-SDR pass is formed on the device) and a call that fits
// the context's grow-only blocks allocates nothing.
static_assert(CM_LOSS == BSRNN_M_LOSS && CM_SDR == BSRNN_M_SDR && CM_INPUT_SDR == BSRNN_M_INPUT_SDR && CM_SISDR == BSRNN_M_SISDR &&
              CM_L1_TIME == BSRNN_M_L1_TIME && CM_L1_RE == BSRNN_M_L1_RE && CM_L1_IM == BSRNN_M_L1_IM &&
              CM_SEPARATION_DB == BSRNN_M_SEPARATION_DB && CM_COUNT == BSRNN_N_METRICS, "metrics_host.h");

// Where a call's sums lie in er.d_part and its pinned mirror: [time R x slots x 7 | si R x slots x 2, two-pass calls only | freq R x FB x 2 |
// in n_clips x IB], slots = the time grid's workgroups (or accumulator slots) per row
struct EvalSums {
    int slots, FB, IB;
    size_t n_time, n_si, n_freq, n_in;
    EvalSums(int R, int n_clips, int slots_, bool two_pass, int FB_)
        : slots(slots_), FB(FB_), IB(metric_input_sdr_blocks(n_clips)), n_time((size_t)R * slots_ * METRIC_TIME_Q),
          n_si(two_pass ? (size_t)R * slots_ * 2 : 0), n_freq((size_t)R * FB_ * 2), n_in((size_t)n_clips * IB) {}
    size_t total() const { return n_time + n_si + n_freq + n_in; }
    double* time(double* p) const { return p; }
    double* si(double* p) const { return p + n_time; }
    double* freq(double* p) const { return p + n_time + n_si; }
    double* in(double* p) const { return p + n_time + n_si + n_freq; }
};

static std::vector<MetricClip> clip_table(const std::vector<int>& first_row, const int32_t* clip_rows_host, const int64_t* clip_lens_host, int n_clips)
{
    std::vector<MetricClip> clips(n_clips);
    for (int i = 0; i < n_clips; ++i) clips[i] = MetricClip{first_row[i], clip_rows_host ? clip_rows_host[i] : 1, clip_lens_host[i]};
    return clips;
}

// The metric kernels' table of a call, [R int64 row lengths | MetricClip per clip], through er.table in front of the call's kernels.  The
// block on the device is not touched before the next call, so a re-run sees the same table.
struct EvalTable { const int64_t* lens = nullptr; const MetricClip* clips = nullptr; };      // on the device
static int eval_table_upload(bsrnn_ctx* c, const std::vector<int64_t>& row_lens, const std::vector<MetricClip>& clips, hipStream_t s, EvalTable& t)
{
    bsrnn_ctx::EvalRagged& er = c->er;
    const size_t b_lens = row_lens.size() * sizeof(int64_t), b_clips = clips.size() * sizeof(MetricClip);
    if (int rc = er.table.upload(b_lens + b_clips, s, [&](char* h) { memcpy(h, row_lens.data(), b_lens); memcpy(h + b_lens, clips.data(), b_clips); }))
        return rc;
    t.lens = reinterpret_cast<const int64_t*>(er.table.d);
    t.clips = reinterpret_cast<const MetricClip*>(er.table.d + b_lens);
    return 0;
}

// The end of every evaluate call: the one download of the sums, then the numbers per clip (metrics_host.h)
static int eval_finish(bsrnn_ctx* c, hipStream_t s, const EvalSums& q, const std::vector<MetricClip>& clips, double* metrics)
{
    bsrnn_ctx::EvalRagged& er = c->er;
    HIP_TRY(hipMemcpyAsync(er.h_part, er.d_part, q.total() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    clip_metrics_from_partials(clips.data(), (int)clips.size(), q.time(er.h_part), q.n_si ? q.si(er.h_part) : nullptr, q.slots, q.freq(er.h_part),
                               q.FB, q.in(er.h_part), q.IB, metrics);
    return 0;
}

// The context's scratch (bsrnn_ctx::EvalRagged) for a call of these sizes; grow-only
static int eval_ragged_reserve(bsrnn_ctx* c, size_t n_part, size_t n_est)
{
    bsrnn_ctx::EvalRagged& er = c->er;
    if (n_part <= er.part_cap && n_est <= er.est_cap) return 0;
    HIP_TRY(hipDeviceSynchronize());                                  // queued kernels read and write the old blocks
    auto grown = [](size_t n) { return (n + n / 2 + 255) & ~size_t(255); };
    if (n_part > er.part_cap) {
        if (er.d_part) { (void)hipFree(er.d_part); (void)hipHostFree(er.h_part); er.d_part = er.h_part = nullptr; er.part_cap = 0; }
        const size_t cap = grown(n_part);
        g_dbg[DBG_ALLOC] += 2;
        HIP_TRY(hipHostMalloc((void**)&er.h_part, cap * sizeof(double), hipHostMallocDefault));
        const hipError_t e = hipMalloc((void**)&er.d_part, cap * sizeof(double));
        if (e != hipSuccess) { (void)hipHostFree(er.h_part); er.h_part = er.d_part = nullptr; return fail(BSRNN_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
        er.part_cap = cap;
    }
    if (n_est > er.est_cap) {
        if (er.d_est) { (void)hipFree(er.d_est); er.d_est = nullptr; er.est_cap = 0; }
        const size_t cap = grown(n_est);
        ++g_dbg[DBG_ALLOC];
        const hipError_t e = hipMalloc((void**)&er.d_est, cap * sizeof(float));
        if (e != hipSuccess) { er.d_est = nullptr; return fail(BSRNN_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
        er.est_cap = cap;
    }
    return 0;
}

// The rectangle [R][n] as the batch of one clip {0, R, n}: R equal lengths, wave_stride = n, out_stride = n_est.  The separation stays
// bsrnn_separate (it runs the concurrent row blocks for large R); without est_out the estimate lives in er.d_est, which is grow-only and
// goes with the context.
int bsrnn_evaluate(bsrnn_ctx* c, const float* mix, const float* speech, int32_t R, int64_t n, float* est_out,
                   double* metrics, void* stream)
{
    if (!metrics || !speech) return fail(BSRNN_EARG, "bsrnn_evaluate: null argument");
    const int T = 1 + (int)(n / HOPS);
    const int64_t n_est = (int64_t)(T - 1) * HOPS;
    int rc = 0;
    if ((rc = check_ready(c))) return rc;
    if (!mix || R < 1 || n <= NFFT / 2) return fail(BSRNN_EARG, "bsrnn_evaluate: need n > 1024 samples, got %lld", (long long)n);
    // the metrics read mix and speech after the estimate is written, and the re-run below reads them again: whatever the policy
    if (ranges_overlap(est_out, (size_t)R * n_est * sizeof(float), mix, (size_t)R * n * sizeof(float)) ||
        ranges_overlap(est_out, (size_t)R * n_est * sizeof(float), speech, (size_t)R * n * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_evaluate: est_out must not overlap mix or speech (the metrics and a re-run of the call read them after the estimate is written)");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);

    const EvalSums sums(R, 1, metric_time_chunks(n_est), true, std::min(T, 16));
    if ((rc = eval_ragged_reserve(c, sums.total(), est_out ? 0 : (size_t)R * n_est))) return rc;
    bsrnn_ctx::EvalRagged& er = c->er;
    float* est = est_out ? est_out : er.d_est;
    std::vector<int64_t> row_lens(R);
    std::fill(row_lens.begin(), row_lens.end(), n);
    const std::vector<MetricClip> clips{MetricClip{0, R, n}};
    EvalTable tab;
    if ((rc = eval_table_upload(c, row_lens, clips, s, tab))) return rc;

    auto run = [&]() -> int {
        // x_time and the estimate's spectrum (left in Yf, frame-major)                               m_dataset.py:186-195
        if (int rc2 = bsrnn_separate(c, mix, est, R, n, stream)) return rc2;
        // waveform_speech_freq: the clean signal through the same analysis (Xf is free once the mask launch ran)   :196
        launch_stft(c->tb, speech, c->Xf, R, n, T, s);
        launch_metric_time_ragged(est, speech, mix, tab.lens, R, T, n_est, n, sums.time(er.d_part), s);
        launch_metric_sisdr_ragged(est, speech, tab.lens, R, T, n_est, n, sums.time(er.d_part), sums.si(er.d_part), s);
        launch_metric_freq_ragged(c->tb, c->Yf, c->Xf, tab.lens, R, T, sums.freq(er.d_part), sums.FB, s);
        launch_metric_input_sdr_ragged(speech, mix, tab.clips, 1, n, sums.in(er.d_part), sums.IB, s);
        HIP_TRY(hipGetLastError());
        return eval_finish(c, s, sums, clips, metrics);
    };
    // A synchronous entry point: whatever the context's range policy, the guard word is handled before the metrics are returned, as under
    // the default policy (finish_call: a structural fall-back, or the exact-fp32 kernels for an operand that left the fp16 range)
    if ((rc = run())) return rc;
    return finish_call(c, s, run, true);
}

// Flow of the ragged call: bsrnn_separate_ragged(mix) with the per-clip lengths expanded to rows (Yf keeps the estimate's spectrum, padded
// frames zero) -> the clean signal through the ragged analysis into Xf -> the four metric kernels -> the shared finish.
int bsrnn_evaluate_ragged(bsrnn_ctx* c, const float* mix, const float* speech, int64_t wave_stride, const int64_t* clip_lens_host,
                          const int32_t* clip_rows_host, int32_t n_clips, float* est_out, double* metrics, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!mix || !speech || !clip_lens_host || !metrics || n_clips < 1)
        return fail(BSRNN_EARG, "bsrnn_evaluate_ragged: need a mixture, a clean signal, the clips' lengths, room for the metrics and n_clips >= 1, got n_clips = %d", n_clips);
    std::vector<int64_t> row_lens;
    std::vector<int> first_row;
    const ClipShape q = clip_shape(clip_lens_host, clip_rows_host, n_clips, wave_stride, row_lens, first_row);
    if (int rc0 = clip_shape_refuse("bsrnn_evaluate_ragged", q, wave_stride)) return rc0;
    const int R = (int)q.R, T = (int)q.Tmax;
    // the metrics read mix and speech after the estimate is written, and a re-run reads them again: whatever the policy
    if (ranges_overlap(est_out, (size_t)R * q.out_stride * sizeof(float), mix, (size_t)R * wave_stride * sizeof(float)) ||
        ranges_overlap(est_out, (size_t)R * q.out_stride * sizeof(float), speech, (size_t)R * wave_stride * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_evaluate_ragged: est_out must not overlap mix or speech (the metrics and a re-run of the call read them after the estimate is written)");
    int rc = check_ready(c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);

    const EvalSums sums(R, n_clips, metric_time_chunks(q.out_stride), true, std::min(T, 16));
    if ((rc = eval_ragged_reserve(c, sums.total(), est_out ? 0 : (size_t)R * q.out_stride))) return rc;
    bsrnn_ctx::EvalRagged& er = c->er;
    float* est = est_out ? est_out : er.d_est;
    const std::vector<MetricClip> clips = clip_table(first_row, clip_rows_host, clip_lens_host, n_clips);
    EvalTable tab;
    if ((rc = eval_table_upload(c, row_lens, clips, s, tab))) return rc;

    auto run = [&]() -> int {
        // x_time of every row and the estimate's spectrum (left in Yf, frame-major, padded frames zero)      m_dataset.py:186-195
        if (int rc2 = bsrnn_separate_ragged(c, mix, wave_stride, row_lens.data(), est, R, stream)) return rc2;
        // waveform_speech_freq: the clean signal through the same analysis (Xf is free once the mask launch ran)   :196
        launch_stft_ragged(c->tb, speech, wave_stride, tab.lens, c->Xf, R, T, s);
        launch_metric_time_ragged(est, speech, mix, tab.lens, R, T, q.out_stride, wave_stride, sums.time(er.d_part), s);
        launch_metric_sisdr_ragged(est, speech, tab.lens, R, T, q.out_stride, wave_stride, sums.time(er.d_part), sums.si(er.d_part), s);
        launch_metric_freq_ragged(c->tb, c->Yf, c->Xf, tab.lens, R, T, sums.freq(er.d_part), sums.FB, s);
        launch_metric_input_sdr_ragged(speech, mix, tab.clips, n_clips, wave_stride, sums.in(er.d_part), sums.IB, s);
        HIP_TRY(hipGetLastError());
        return eval_finish(c, s, sums, clips, metrics);
    };
    // A synchronous entry point: whatever the context's range policy, the guard word is handled before the metrics are returned, as in
    // bsrnn_evaluate (finish_call: a structural fall-back, or the whole flow again on the exact-fp32 kernels from the same inputs and lengths)
    if ((rc = run())) return rc;
    return finish_call(c, s, run, true);
}

// --------------------------------------------------------------------------- ragged long-form evaluate: the metrics per clip, in segments
// bsrnn_evaluate_ragged's numbers from bsrnn_separate_long_ragged's flow: the same cut, plan, alive prefix and carry sets
// (long_ragged_segments), so the workspace is R x seg frame rows and the model is paid for on about the real frames.  A segment's estimate
// spectrum is gone when the next segment starts, so the sums are formed per segment: when a segment is FINAL (finish_call has returned,
// whatever the range policy - Yf holds its spectrum whichever pass produced it, and its sums are added exactly once) the clean signal
// goes through the segment's analysis into Xf and one launch each adds the segment's time and spectral sums into the call's accumulators
// (metrics.hip: a slot per workgroup, plain additions in stream order).  The SI-SDR needs no second pass over an estimate that no longer
// exists: metrics_host.h, sisdr_sums_from_totals.  INPUT_SDR does not depend on the estimate: bsrnn_evaluate_ragged's launch over the whole
// inputs.  One download at the end.  Nothing is sized by Tmax: accumulators [R][METRIC_SEG_SLOTS][7 + 2] and, when the caller wants no
// estimate, a buffer of ONE segment's hops [R][seg * 1024] that the synthesis writes with that row stride.
int bsrnn_evaluate_long_ragged(bsrnn_ctx* c, const float* mix, const float* speech, int64_t wave_stride, const int64_t* clip_lens_host,
                               const int32_t* clip_rows_host, int32_t n_clips, int32_t seg_frames, float* est_out, double* metrics, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!mix || !speech || !clip_lens_host || !metrics || n_clips < 1)
        return fail(BSRNN_EARG, "bsrnn_evaluate_long_ragged: need a mixture, a clean signal, the clips' lengths, room for the metrics and n_clips >= 1, got n_clips = %d", n_clips);
    if (seg_frames < 1) return fail(BSRNN_EARG, "bsrnn_evaluate_long_ragged: seg_frames = %d (at least one frame per segment)", seg_frames);
    std::vector<int64_t> row_lens;
    std::vector<int> first_row;
    const ClipShape q = clip_shape(clip_lens_host, clip_rows_host, n_clips, wave_stride, row_lens, first_row);
    if (int rc0 = clip_shape_refuse("bsrnn_evaluate_long_ragged", q, wave_stride)) return rc0;
    const int R = (int)q.R, T = (int)q.Tmax;
    const RaggedLongPlan plan = ragged_long_plan(row_lens.data(), R, wave_stride, seg_frames);
    if (int rc0 = ragged_shape_refuse("bsrnn_evaluate_long_ragged", plan.shape, R, wave_stride, seg_frames)) return rc0;
    // whatever the range policy: later segments and the metrics read mix and speech after earlier hops of the estimate are written
    if (ranges_overlap(est_out, (size_t)R * q.out_stride * sizeof(float), mix, (size_t)R * wave_stride * sizeof(float)) ||
        ranges_overlap(est_out, (size_t)R * q.out_stride * sizeof(float), speech, (size_t)R * wave_stride * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_evaluate_long_ragged: est_out must not overlap mix or speech (later segments, the metrics and a re-run read them after the estimate is written)");
    if (seg_frames >= T) {                                            // one segment IS the ragged evaluate: bit-identical by construction
        const int rc1 = bsrnn_evaluate_ragged(c, mix, speech, wave_stride, clip_lens_host, clip_rows_host, n_clips, est_out, metrics, stream);
        if (!rc1) g_dbg[DBG_LONG_RAGGED_ROWS] += plan.frame_rows;
        return rc1;
    }
    int rc = check_ready(c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);

    const int seg = seg_frames;
    const EvalSums sums(R, n_clips, METRIC_SEG_SLOTS, false, METRIC_SEG_SLOTS);
    const int64_t seg_stride = (int64_t)seg * HOPS;
    if ((rc = eval_ragged_reserve(c, sums.total(), est_out ? 0 : (size_t)R * seg_stride))) return rc;
    bsrnn_ctx::EvalRagged& er = c->er;
    const std::vector<MetricClip> clips = clip_table(first_row, clip_rows_host, clip_lens_host, n_clips);
    EvalTable tab;                                                    // (its lengths are not read: long_ragged_segments uploads the segments' own)
    if ((rc = eval_table_upload(c, row_lens, clips, s, tab))) return rc;
    double *p_time = sums.time(er.d_part), *p_freq = sums.freq(er.d_part);
    HIP_TRY(hipMemsetAsync(p_time, 0, (sums.n_time + sums.n_freq) * sizeof(double), s));
    launch_metric_input_sdr_ragged(speech, mix, tab.clips, n_clips, wave_stride, sums.in(er.d_part), sums.IB, s);
    HIP_TRY(hipGetLastError());

    auto segment_sums = [&](int ta, int te, int Ri, const int64_t* d_lens, const float* seg_est) -> int {
        // waveform_speech_freq of the segment's frames (Xf is free once the mask stage has run), then the segment's sums       m_dataset.py:196-213
        launch_stft_ragged_segment(c->tb, speech, wave_stride, d_lens, c->Xf, Ri, ta, te, s);
        launch_metric_ragged_segment(c->tb, seg_est, est_out ? q.out_stride : seg_stride, speech, mix, d_lens, wave_stride, c->Yf, c->Xf, Ri, ta, te,
                                     p_time, p_freq, s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if ((rc = long_ragged_segments(c, plan, mix, wave_stride, row_lens.data(), est_out ? est_out : er.d_est, est_out ? q.out_stride : seg_stride,
                                   est_out != nullptr, R, seg, s, true, segment_sums)))
        return rc;
    return eval_finish(c, s, sums, clips, metrics);
}

// --------------------------------------------------------------------------- dialog / background section mining
// The per-hop figures of gendataset-separate.py:100-105 for a ragged batch (the kernel: metrics.hip) and the script's run-length state
// machine over them (sections_host.h; plain host functions).  The hop counts travel in the ragged calls' block.
static_assert(ACT_RATIO == BSRNN_ACT_RATIO && ACT_LEVEL == BSRNN_ACT_LEVEL && ACT_Q == 2, "sections_host.h and bsrnn_hip.h disagree");
static_assert(SECTION_DIALOG == BSRNN_SECTION_DIALOG && SECTION_BACKGROUND == BSRNN_SECTION_BACKGROUND && SECTION_NONE == 0,
              "sections_host.h and bsrnn_hip.h disagree");

int bsrnn_hop_activity(bsrnn_ctx* c, const float* mix, int64_t mix_stride, const float* est, int64_t est_stride, const int32_t* hops_host,
                       int32_t R, int32_t Hmax, double* act, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!mix || !est || !act) return fail(BSRNN_EARG, "bsrnn_hop_activity: null argument (need mix_dev, est_dev and act_dev)");
    if (R < 1 || Hmax < 1) return fail(BSRNN_EARG, "bsrnn_hop_activity: need R >= 1 rows and Hmax >= 1 hops, got R = %d, Hmax = %d", R, Hmax);
    const int64_t row = (int64_t)Hmax * HOPS;
    if (mix_stride < row)
        return fail(BSRNN_EARG, "bsrnn_hop_activity: mix_stride %lld is less than Hmax * 1024 = %lld", (long long)mix_stride, (long long)row);
    if (est_stride < row)
        return fail(BSRNN_EARG, "bsrnn_hop_activity: est_stride %lld is less than Hmax * 1024 = %lld", (long long)est_stride, (long long)row);
    for (int r = 0; hops_host && r < R; ++r)
        if (hops_host[r] < 0 || hops_host[r] > Hmax)
            return fail(BSRNN_EARG, "bsrnn_hop_activity: hops_host[%d] = %d is outside [0, %d]", r, hops_host[r], Hmax);
    // the floats the rows span: behind the last row of a view lies somebody else's memory
    const size_t act_bytes = (size_t)R * Hmax * 2 * sizeof(double);
    if (ranges_overlap(act, act_bytes, mix, ((size_t)(R - 1) * mix_stride + (size_t)row) * sizeof(float)) ||
        ranges_overlap(act, act_bytes, est, ((size_t)(R - 1) * est_stride + (size_t)row) * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_hop_activity: act_dev must not overlap the floats the rows of mix_dev or est_dev span");
    if (int rc = check_device(c)) return rc;                          // (no model stage: needs no committed weights)
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const int32_t* d_hops = nullptr;
    if (hops_host) {
        const size_t bytes = (size_t)R * sizeof(int32_t);
        if (int rc = c->rg.upload(bytes, s, [&](char* h) { memcpy(h, hops_host, bytes); })) return rc;
        d_hops = reinterpret_cast<const int32_t*>(c->rg.d);
    }
    launch_hop_activity(mix, mix_stride, est, est_stride, d_hops, R, Hmax, act, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

void bsrnn_section_rule_default(bsrnn_section_rule* rule)
{
    if (!rule) return;
    const SectionRule q;
    rule->dialog_db = q.dialog_db; rule->bridge_db = q.bridge_db; rule->background_db = q.background_db; rule->silence_db = q.silence_db;
    rule->level_floor = q.level_floor; rule->floor_db = q.floor_db; rule->min_run = q.min_run;
}

void bsrnn_section_state_reset(bsrnn_section_state* state)
{
    if (!state) return;
    state->n_dialog = state->n_background = 0;
    state->open_kind = BSRNN_SECTION_NONE;
    state->open_hop = state->hop = 0;
}

int bsrnn_sections_scan(const bsrnn_section_rule* rule, bsrnn_section_state* state, const double* act_host, int64_t n_hops, int32_t flush,
                        bsrnn_section* out, int64_t cap, int64_t* n_out)
{
    SectionRule q;
    if (rule) {
        q.dialog_db = rule->dialog_db; q.bridge_db = rule->bridge_db; q.background_db = rule->background_db; q.silence_db = rule->silence_db;
        q.level_floor = rule->level_floor; q.floor_db = rule->floor_db; q.min_run = rule->min_run;
    }
    switch (sections_check(q, state, act_host, n_hops, cap, n_out)) {
    case SECTIONS_NULL_STATE: return fail(BSRNN_EARG, "bsrnn_sections_scan: null state");
    case SECTIONS_NULL_COUNT: return fail(BSRNN_EARG, "bsrnn_sections_scan: null n_out");
    case SECTIONS_NEGATIVE: return fail(BSRNN_EARG, "bsrnn_sections_scan: n_hops = %lld and cap = %lld must not be negative", (long long)n_hops, (long long)cap);
    case SECTIONS_MIN_RUN: return fail(BSRNN_EARG, "bsrnn_sections_scan: min_run = %d, need at least 1", q.min_run);
    case SECTIONS_NULL_ACT: return fail(BSRNN_EARG, "bsrnn_sections_scan: act_host is null with n_hops = %lld", (long long)n_hops);
    case SECTIONS_OK: break;
    }
    if (!out && cap > 0) return fail(BSRNN_EARG, "bsrnn_sections_scan: out is null with cap = %lld", (long long)cap);
    SectionState st;
    st.n_dialog = state->n_dialog; st.n_background = state->n_background; st.open_kind = state->open_kind;
    st.open_hop = state->open_hop; st.hop = state->hop;
    *n_out = sections_scan(q, st, act_host, n_hops, flush != 0, out, cap);
    state->n_dialog = st.n_dialog; state->n_background = st.n_background; state->open_kind = st.open_kind;
    state->open_hop = st.open_hop; state->hop = st.hop;
    return 0;
}

// --------------------------------------------------------------------------- measurement
int bsrnn_set_profiling(bsrnn_ctx* c, int32_t on)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    if (on && c->pool.empty()) {
        c->pool.resize(8192);
        // timing-only events: without the system-scope release fence a record costs the stream ~1 us instead of ~10
        for (auto& r : c->pool) {
            HIP_TRY(hipEventCreateWithFlags(&r.a, hipEventDisableSystemFence));
            HIP_TRY(hipEventCreateWithFlags(&r.b, hipEventDisableSystemFence));
        }
    }
    c->prof = on < 0 ? 0xffffffffu : (unsigned)on;   // bit i enables stage i; negative = all stages
    return 0;
}
int bsrnn_stage_count(void) { return NSTAGE; }
const char* bsrnn_stage_name(int32_t i) { return (i >= 0 && i < NSTAGE) ? kStageNames[i] : ""; }

int bsrnn_stage_times(bsrnn_ctx* c, double* ms_out, int64_t* n_out, int32_t reset)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    for (size_t i = 0; i < c->pool_used; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->pool[i].a, c->pool[i].b) == hipSuccess) {
            c->acc_ms[c->pool[i].stage] += ms;
            c->acc_n[c->pool[i].stage] += 1;
        }
    }
    c->pool_used = 0;
    for (int i = 0; i < NSTAGE; ++i) {
        if (ms_out) ms_out[i] = c->acc_ms[i];
        if (n_out) n_out[i] = c->acc_n[i];
    }
    if (reset) { memset(c->acc_ms, 0, sizeof c->acc_ms); memset(c->acc_n, 0, sizeof c->acc_n); }
    return 0;
}

// --------------------------------------------------------------------------- device memory helpers
int bsrnn_dev_alloc(bsrnn_ctx* c, int64_t nbytes, void** out)
{
    if (!c || !out || nbytes < 0) return fail(BSRNN_EARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(out, (size_t)nbytes));
    return 0;
}
int bsrnn_dev_free(bsrnn_ctx* c, void* p)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipFree(p));
    return 0;
}
int bsrnn_copy_h2d(bsrnn_ctx* c, void* dst, const void* src, int64_t nbytes)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(dst, src, (size_t)nbytes, hipMemcpyHostToDevice));
    return 0;
}
int bsrnn_copy_d2h(bsrnn_ctx* c, void* dst, const void* src, int64_t nbytes)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(dst, src, (size_t)nbytes, hipMemcpyDeviceToHost));
    return 0;
}
int bsrnn_sync(bsrnn_ctx* c, void* stream)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (int rcj = ovl_join_host(c)) return rcj;
    return check_range(c);
}

}  // extern "C"
