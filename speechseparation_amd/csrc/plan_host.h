// The call plan and its index arithmetic: which kernels a call of C rows x T frames runs, how a batch is cut into concurrent row blocks
// and where their hand-over flags sit, the dispatch orders of the overlapped dual path, the fused chains' task tables, the workspace
// segments, and the cut of a long clip into segments, windows and hops.  Host arithmetic only (api.hip reads the environment, allocates,
// uploads and launches), so tests run it without a GPU (tests/test_call_plan.py).
#pragma once
#include "descriptors.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace bsrnn {

constexpr int MAX_PARTS = 4;          // concurrent row blocks of one call, at most
constexpr int OVL_HEAD = 16;          // ints in front of a block's progress words (the resident counter on a line of its own)

// --------------------------------------------------------------------------- the call plan
// Which kernels one model call runs, decided once per call by plan_call() and read by everything that launches or sizes something for it
// (run_stage, the overlapped dual path, bsrnn_separate's row blocks): the time-axis launch and the consumers that wait on its progress
// words agree on its sequences per workgroup because they all read Flow::seqs.
// Band-axis blocks: a few frame rows (streaming) as one launch of the whole block, fc + residual included (band_block_small_kernel); both
// layers in one launch writing the shares of the block's fc that the time-axis launch adds (kernels.h); both layers in one launch and the fc
// + residual as a grouped-GEMM launch; one launch per layer and the same fc launch.
enum BandForm { BAND_SMALL, BAND_PAIR_PARTS, BAND_PAIR, BAND_LAYERS };
struct Flow {
    bool exact;          // force_f32(): the range-guard re-run - every launch on the exact-fp32 kernels
    bool lstm_f32;       // the recurrent layers on the fp32 kernels (BSRNN_LSTM=f32, or exact)
    bool gemv;           // a call of <= GEMV_MAX_FRAME_ROWS frame rows: its per-band layers as GEMV launches (gemm_slot, gemv.hip)
    bool chains;         // the per-band MLPs as fused chains (mlp_chain.hip); else one launch per layer
    int band;            // BandForm of the band-axis blocks
    bool time_fc;        // the time-axis launch forms its block's fc + residual itself (no MS_TIMEFC launch)
    int seqs, nwg;       // the time-axis launch: sequences per workgroup (4, or 8 on time_lstm_h2w8_kernel) and workgroups
    bool overlap;        // the dual path runs overlapped (run_overlapped), given its tables and no graph capture (ovl_table)
    int band_tiles;      // the pair launch: tiles of 16 sequences per workgroup, 1 or 2 (band_pair_tiles)
};
// What the process fixed at first use (api.hip reads the environment): BSRNN_BAND_PAIR=0 one launch per band
// layer; BSRNN_BAND_FC=gemm the band block's fc + residual as a grouped-GEMM launch instead of the shares the pair launch writes and the
// time-axis launch adds (the second layer alone with the shares sits at the edge of 256 VGPRs - as a kernel of its own it spilled four
// registers - and is not shipped); BSRNN_TIME_KERNEL=v3 the time block's fc as a launch of its own; BSRNN_TIME_SEQ8 = 0 / 1: eight
// sequences per time-axis workgroup never / always (unset, -1: where four would need more than one round of workgroups);
// BSRNN_BAND_PAIR=tiles1 / tiles2: the pair launch with one / two tiles per workgroup whatever the call's size (A/Bs and tests).
struct PlanKnobs {
    bool band_pair, band_parts, time_fused;
    int seq8;
    int gemm_mode, lstm_mode;      // GemmMode, LstmMode
    int cus;                       // CUs of the device
    int band_tiles = 0;            // 1 / 2: tiles per workgroup of the pair launch forced; 0: by the call's size (band_pair_tiles)
};
// What the thread and the context contribute: force_f32() (the exact re-run plans again), fused chains, and the context's sticky fall-backs
struct PlanState { bool exact, fused, band_pair_off, overlap_env, overlap_off; };

// Tiles of 16 sequences per workgroup of the band-pair launch over N sequences (the call's frame rows).  A workgroup loads both layers'
// weights (343 KB of fragments) whatever it computes with them, and the launch holds 2 workgroups per CU: where one tile per workgroup
// (2 directions x ceil(N / 16) workgroups) needs more than one dispatch round, a workgroup takes two tiles on one set of weights and the
// launch half as many workgroups.  Within one round nothing would be gained, only the launch's parallelism halved.
inline int band_pair_tiles(int N, int cus, int force = 0)
{
    if (force == 1 || force == 2) return force;
    return 2 * ((N + 15) / 16) > 2 * cus ? 2 : 1;
}
// Workgroups of that launch: a slot is `tiles` consecutive tiles (an odd tile count leaves the last slot of two with one), and 16
// consecutive workgroups are the two directions of eight slots - partners 8 ids apart (lstm.hip::band_tiles_of_block)
inline int band_pair_slots(int N, int tiles) { const int nt = (N + 15) / 16; return tiles == 2 ? (nt + 1) / 2 : nt; }
inline int band_pair_grid(int N, int tiles) { return (band_pair_slots(N, tiles) + 7) / 8 * 16; }

// The plan of a call of C rows x T frames on K bands.  gemv / overlap: the entry point may run a few frame rows on the GEMV kernels / the
// dual path overlapped.
inline Flow plan_call(int K, int C, int T, bool gemv, bool overlap, const PlanKnobs& kn, const PlanState& st)
{
    Flow f;
    const int M = C * T, N = C * K, cus = kn.cus;
    f.exact = st.exact;
    f.lstm_f32 = f.exact || kn.lstm_mode == LSTM_F32;
    const bool gemm16 = !f.exact && kn.gemm_mode != GEMM_F32;
    f.gemv = gemv && M <= GEMV_MAX_FRAME_ROWS;
    f.chains = st.fused && !f.exact && !f.gemv;
    // the fc inside the time-axis kernel unless the Linear layers are asked to be exact fp32 (BSRNN_GEMM=f32)
    f.time_fc = !f.lstm_f32 && gemm16 && kn.time_fused;
    // the pair launch is fp16x2 only; a context whose pair launch once reported that its partner workgroups did not meet runs one launch
    // per layer from then on.  The fc in parts needs the pair launch and the fused time-axis kernel.
    const bool pair = !f.lstm_f32 && kn.band_pair && !st.band_pair_off;
    if (!f.lstm_f32 && gemm16 && M <= 8 && K <= BS_MAXL) f.band = BAND_SMALL;
    else if (pair && kn.band_parts && f.time_fc) f.band = BAND_PAIR_PARTS;
    else f.band = pair ? BAND_PAIR : BAND_LAYERS;
    f.band_tiles = band_pair_tiles(M, cus, kn.band_tiles);
    f.seqs = f.time_fc && (kn.seq8 == 1 || (kn.seq8 < 0 && (N + 3) / 4 > cus)) ? 8 : 4;
    f.nwg = (N + f.seqs - 1) / f.seqs;
    // Overlapped: the parts flow with fused chains (the launches that know how to publish / wait), a time-axis launch that leaves CUs free
    // (at most 7/8 of them) and enough frames for a head start to exist
    f.overlap = overlap && st.overlap_env && !st.overlap_off && f.band == BAND_PAIR_PARTS && st.fused && f.nwg >= 32 && f.nwg <= cus - cus / 8 &&
                T >= 32 && T < (4 << OVL_EPOCH_SHIFT) - 8;
    return f;
}

// --------------------------------------------------------------------------- state size
// The time-axis LSTM state of C rows, [4][2][C*K][64]: two Time blocks x (h, c) x 2 layers; one Time block's slab of it
inline size_t state_floats(int C, int K) { return (size_t)4 * 2 * C * K * HID; }
inline size_t state_slab_floats(int C, int K) { return (size_t)2 * 2 * C * K * HID; }

// --------------------------------------------------------------------------- task tables of the fused chains
// (descriptor index, first frame row) of one workgroup of a chain launch; the kernels read it as an int2
struct ChainTask { int desc, row0; };
// Task table of a fused chain launch for M frame rows: one entry (descriptor, first row) per workgroup, in dispatch order:
// longest workgroups first (the descriptors are sorted by class and cost at commit), all row blocks of a band together
// (they share its weight stream through L2).  Measured and dropped: interleaving the fill-bound 768-wide band with the
// others (its workgroups take 97 us on half the CUs against 129 us on all of them, tools/chain_bench.hip) - the late starts
// of the long workgroups cost more than the contention saves (310 vs 250 us per chain).
inline void build_chain_tasks(const std::vector<ChainDesc>& ds, int M, std::vector<ChainTask>& out)
{
    out.clear();
    for (size_t di = 0; di < ds.size(); ++di)
        for (int r0 = 0; r0 < M; r0 += chain_rows(ds[di])) out.push_back(ChainTask{(int)di, r0});
}

// --------------------------------------------------------------------------- overlapped dual path: dispatch orders by readiness
// ints per time block of the progress words: the head, then one word per time-axis workgroup
inline int ovl_stride(int nwg) { return OVL_HEAD + ((nwg + 15) & ~15); }
// The consumers' dispatch orders for a call of M = C * T frame rows whose time-axis launch has nwg workgroups on a device of cus CUs
struct OvlOrders { std::vector<int> band_order; std::vector<ChainTask> mask_tasks; };
inline OvlOrders ovl_orders(int M, int T, int nwg, int cus, const std::vector<ChainDesc>& ds /* the mask chain */)
{
    // band block: tiles of 16 frame rows m = row * T + frame, sorted by the last frame the tile needs (a tile that straddles two batch
    // rows needs the first one's last frame); padded with -1 to the launch's whole groups of eight tiles
    const int tiles = (M + 15) / 16, n_ord = ((tiles + 7) / 8) * 8;
    std::vector<int> order(tiles), ready(tiles);
    for (int t = 0; t < tiles; ++t) {
        const int m0 = 16 * t, m1 = std::min(M - 1, m0 + 15);
        order[t] = t;
        ready[t] = m0 / T != m1 / T ? T - 1 : m1 % T;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ready[a] < ready[b]; });
    order.resize(n_ord, -1);
    // mask chain: its task table (longest workgroups first) with the workgroups that can START while the time-axis launch still runs
    // in front: as many as that launch leaves CUs free (each runs longer than the rest of it), the earliest-ready of the heavy classes
    // (<= 80 rows per workgroup: the widest bands, which also end the launch when they start late)
    std::vector<ChainTask> tasks;
    build_chain_tasks(ds, M, tasks);
    std::vector<int> cand;
    auto task_ready = [&](const ChainTask& t) {
        const int m1 = std::min(M - 1, t.row0 + chain_rows(ds[t.desc]) - 1);
        return t.row0 / T != m1 / T ? T - 1 : m1 % T;
    };
    for (int i = 0; i < (int)tasks.size(); ++i)
        if (!ds[tasks[i].desc].constant && chain_rows(ds[tasks[i].desc]) <= 80 && task_ready(tasks[i]) < T - 1) cand.push_back(i);
    std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return task_ready(tasks[a]) < task_ready(tasks[b]); });
    const int n_early = std::min((int)cand.size(), std::max(0, cus - nwg));
    std::vector<char> early(tasks.size(), 0);
    std::vector<ChainTask> mt;
    for (int i = 0; i < n_early; ++i) { mt.push_back(tasks[cand[i]]); early[cand[i]] = 1; }
    for (int i = 0; i < (int)tasks.size(); ++i)
        if (!early[i]) mt.push_back(tasks[i]);
    return OvlOrders{std::move(order), std::move(mt)};
}

// --------------------------------------------------------------------------- concurrent row blocks of one call (bsrnn_separate)
// Rows are independent, so the batch is cut into `parts` contiguous row blocks that run the whole
// stage sequence concurrently on separate streams: the ramps, tails and latency-bound stages of
// one block (e.g. the time-axis LSTM occupies 192 of 256 CUs) overlap matrix work of the other.
// (one block while the time-axis launch of the whole batch is one round of workgroups - eight sequences each from 1 024 sequences on -,
//  two from there: 128 / 160 rows 1.75 / 2.26 -> 1.73 / 2.18 ms with one block, 192 / 256 rows 2.59 / 3.43 ms with two against 2.72 / 3.47)
// whole_nwg: the time-axis workgroups of the whole batch's plan.
inline int row_block_count(int R, int T, int whole_nwg, int cus)
{
    int parts = R >= 128 && whole_nwg > cus ? 2 : 1;
    if (R < 2 * parts || (int64_t)R * T < 2048) parts = 1;
    return parts;
}
// Block j of `parts` is rows [r0[j], r0[j + 1]); ms[j] = its frame rows (what its task table is keyed by: ensure_tasks)
struct RowBlocks { int parts; int r0[MAX_PARTS + 1]; int ms[MAX_PARTS]; };
inline RowBlocks row_blocks(int R, int T, int parts)
{
    RowBlocks b;
    b.parts = parts;
    for (int j = 0; j <= parts; ++j) b.r0[j] = (int)((int64_t)R * j / parts);
    for (int j = 0; j < parts; ++j) b.ms[j] = (b.r0[j + 1] - b.r0[j]) * T;
    return b;
}
// The band-pair launch's hand-over flags: 2 ints per tile of 16 frame rows.  Row block j, whose first frame row is m0, starts j pairs
// behind its first tile's natural place: block j - 1 ends at most at floor(m0 / 16) + 1 + (j - 1), so the pair ranges of concurrent
// blocks are disjoint for any row split (odd R, 3 or 4 blocks included; bsrnn_separate checks row_blocks_share_flags)
inline size_t flag_offset(size_t m0, int j) { return 2 * (m0 / 16 + j); }
inline size_t flag_ints_used(size_t M) { return 2 * ((M + 15) / 16); }                     // by a block of M frame rows
inline size_t flag_ints_reserved(size_t rows) { return rows / 8 + 2 * MAX_PARTS + 64; }    // by a workspace of `rows` frame rows (+ slack per row block)
inline bool row_blocks_share_flags(const RowBlocks& b, int T, int j)                       // blocks j - 1 and j, j >= 1
{
    return flag_offset((size_t)b.r0[j] * T, j) < flag_offset((size_t)b.r0[j - 1] * T, j - 1) + flag_ints_used((size_t)(b.r0[j] - b.r0[j - 1]) * T);
}

// --------------------------------------------------------------------------- workspace layout (ensure_ws)
// Floats of the workspace's segments for `rows` frame rows, each a multiple of 64: Xf, Yf [rows][LDP] | A1, A2 [rows][LDA] | P [rows][LDP]
// | Z0, Z1 [rows][K 64] | HB0, HB1 [rows][K 128] | H1 [rows][K 64] | the hand-over flags (ints)
constexpr int WS_SEGS = 11;
inline void workspace_segments(size_t rows, int LDP, int LDA, int K, size_t sizes[WS_SEGS])
{
    const size_t KH = (size_t)K * HID;
    auto seg = [](size_t n) { return (n + 63) & ~size_t(63); };
    const size_t s[WS_SEGS] = {seg(rows * LDP), seg(rows * LDP), seg(rows * LDA), seg(rows * LDA), seg(rows * LDP),
                               seg(rows * KH), seg(rows * KH), seg(rows * KH * 2), seg(rows * KH * 2), seg(rows * KH),
                               seg(flag_ints_reserved(rows))};
    std::copy(s, s + WS_SEGS, sizes);
}

// --------------------------------------------------------------------------- long-form separation: segments, windows, hops
// Clip samples [*lo, *hi] that the STFT of frames [ta, te) reads, reflections included: frame t covers t*1024 - 1024 .. t*1024 + 1023,
// an index below 0 reflects to at most 1024 (< n), one above n - 1 to 2 (n - 1) - index - for the clip's last frame down to one sample
// in front of the frame's own first when n is a multiple of 1024 (never below 1: n > 1024).
inline void segment_window(int64_t n, int ta, int te, int64_t* lo, int64_t* hi)
{
    const int64_t a = (int64_t)ta * HOPS - HOPS, b = (int64_t)(te - 1) * HOPS + HOPS - 1;
    int64_t l = std::max<int64_t>(a, 0), h = std::min<int64_t>(b, n - 1);
    if (a < 0) h = std::max<int64_t>(h, std::min<int64_t>(-a, n - 1));
    if (b >= n) l = std::min<int64_t>(l, 2 * (n - 1) - b);
    *lo = l; *hi = h;
}
// Segment i of a clip of n samples, T frames, cut into segments of `seg` frames: frames [ta, te), the hops [hop0, hop0 + nh) it
// completes, and its window, the wl clip samples from lo on
struct SegmentCut { int ta, te, hop0, nh; int64_t lo, wl; };
inline SegmentCut segment_cut(int64_t n, int T, int seg, int i)
{
    SegmentCut q;
    q.ta = i * seg; q.te = std::min(T, q.ta + seg);
    q.hop0 = std::max(q.ta - 1, 0); q.nh = q.te - 1 - q.hop0;
    int64_t hi;
    segment_window(n, q.ta, q.te, &q.lo, &hi);
    q.wl = hi - q.lo + 1;
    return q;
}
// Floats per row of the host-buffer entry point's staging for segments of `seg` frames: a window holds at most (seg + 1) * 1024 + 1
// samples per row (segment_window), a block at most seg hops
inline size_t staging_window_floats(int seg) { return (size_t)(seg + 2) * HOPS; }
inline size_t staging_block_floats(int seg) { return (size_t)seg * HOPS; }
// The frame-row counts of a clip's segments (the whole ones, and the tail if there is one): returns how many entries of ms are set
inline int long_frame_rows(int R, int T, int seg, int ms[2])
{
    ms[0] = R * seg; ms[1] = R * (T % seg);
    return ms[1] ? 2 : 1;
}

// --------------------------------------------------------------------------- ragged batches: rows of different lengths (bsrnn_separate_ragged)
// Row r holds lens[r] samples, 1024 < lens[r] <= stride (reflect padding needs more than half a frame; rows are `stride` floats apart), and
// has T_r = 1 + lens[r] / 1024 frames of its own.  The call runs on the rectangle R x Tmax, Tmax = the largest T_r, and writes rows of
// (Tmax - 1) * 1024 samples.  The first row that breaks a bound is refused: bad_row >= 0, bad_len its length, why = RAGGED_SHORT / RAGGED_LONG.
inline int64_t ragged_frames(int64_t n) { return 1 + n / HOPS; }
enum RaggedWhy { RAGGED_OK, RAGGED_SHORT, RAGGED_LONG };
struct RaggedShape { int64_t Tmax, out_stride; int bad_row; int64_t bad_len; int why; };
inline RaggedShape ragged_shape(const int64_t* lens, int R, int64_t stride)
{
    RaggedShape q = {0, 0, -1, 0, RAGGED_OK};
    for (int r = 0; r < R; ++r) {
        if (lens[r] <= NFFT / 2 || lens[r] > stride) {
            return RaggedShape{0, 0, r, lens[r], lens[r] > stride ? RAGGED_LONG : RAGGED_SHORT};
        }
        q.Tmax = std::max(q.Tmax, ragged_frames(lens[r]));
    }
    q.out_stride = (q.Tmax - 1) * HOPS;
    return q;
}
// Frame rows R * Tmax one ragged call may run on (the frame-row index and twice it stay ints)
inline bool ragged_too_many(int64_t R, int64_t Tmax) { return R > INT32_MAX / 2 || (R > 0 && Tmax > (INT32_MAX / 2) / R); }

// --------------------------------------------------------------------------- ragged long-form: rows of different lengths in segments (bsrnn_separate_long_ragged)
// The rectangle R x Tmax of a ragged batch cut into segments of `seg` frames: segment i covers frames [ta, te) = [i * seg, min(Tmax, (i + 1) * seg))
// and runs on the ALIVE PREFIX of the rows, rows[i] = 1 + max{ r : T_r > ta } - rows are never reordered, so a row inside the prefix that
// has already ended is carried as zero frames (any order is correct, longest first is the cheap one).  rows[i] never increases with i, and
// rows[0] = R (every row has two frames).  ms: the distinct frame-row counts rows[i] * (te - ta), in order of first use (what the task tables
// are keyed by); frame_rows: their sum over the segments, the model work of the call.  shape: ragged_shape's answer, refusals included
// (nothing else is filled then); too_many: R * min(seg, Tmax) is beyond what one segment takes (long_prepare's limit).
struct RaggedLongPlan { RaggedShape shape; bool too_many; int nseg; std::vector<int> rows, ms; int64_t frame_rows; };
inline RaggedLongPlan ragged_long_plan(const int64_t* lens, int R, int64_t stride, int seg)
{
    RaggedLongPlan q;
    q.shape = ragged_shape(lens, R, stride);
    q.too_many = false; q.nseg = 0; q.frame_rows = 0;
    if (q.shape.why != RAGGED_OK || R < 1 || seg < 1) return q;
    const int64_t Tmax = q.shape.Tmax;
    if ((int64_t)R * std::min<int64_t>(seg, Tmax) > INT32_MAX / 2) { q.too_many = true; return q; }
    // most[r] = the largest T of rows r .. R - 1: row r is inside the prefix of a segment that starts at ta exactly when most[r] > ta
    std::vector<int64_t> most((size_t)R);
    for (int r = R - 1; r >= 0; --r) most[r] = std::max(ragged_frames(lens[r]), r + 1 < R ? most[r + 1] : 0);
    q.nseg = (int)((Tmax + seg - 1) / seg);
    q.rows.reserve((size_t)q.nseg);
    int alive = R;
    for (int i = 0; i < q.nseg; ++i) {
        const int64_t ta = (int64_t)i * seg, te = std::min<int64_t>(Tmax, ta + seg);
        while (alive > 1 && most[alive - 1] <= ta) --alive;
        const int m = alive * (int)(te - ta);
        q.rows.push_back(alive);
        q.frame_rows += m;
        if (std::find(q.ms.begin(), q.ms.end(), m) == q.ms.end()) q.ms.push_back(m);
    }
    return q;
}

// What segment [ta, te) of that cut owns of a row of Tr frames (bsrnn_evaluate_long_ragged forms a row's sums segment by segment): the clip
// hops it completes, [max(ta - 1, 0), te - 1), as far as they are the row's own (h < Tr - 1), and its frames as far as the row has them
// (t < Tr).  Over the segments of a cut every hop and every frame of the row is owned exactly once.  hops / frames = 0: nothing.
struct SegmentOwned { int hop0, hops, frame0, frames; };
BSRNN_HD inline SegmentOwned segment_owned(int ta, int te, int Tr)
{
    const int h0 = ta > 0 ? ta - 1 : 0;
    const int h1 = te < Tr ? te - 1 : Tr - 1, f1 = te < Tr ? te : Tr;
    return SegmentOwned{h0, h1 > h0 ? h1 - h0 : 0, ta, f1 > ta ? f1 - ta : 0};
}

// --------------------------------------------------------------------------- ragged evaluate: clips of different lengths (bsrnn_evaluate_ragged)
// The unit of the validation metrics is a CLIP: clip c owns rows[c] >= 1 consecutive rows (rows == nullptr: one each) of lens[c] samples each,
// 1024 < lens[c] <= stride.  The call runs bsrnn_separate_ragged on the R = sum rows[c] rows, whose per-row lengths are the per-clip ones
// expanded.  The first clip that breaks a bound is refused: bad_clip >= 0, bad_value its row count (CLIPS_ROWS) or its length (CLIPS_SHORT /
// CLIPS_LONG); CLIPS_MANY: R * Tmax is beyond what one ragged call takes (bad_clip -1).  row_lens / first_row are filled only for CLIPS_OK.
enum ClipsWhy { CLIPS_OK, CLIPS_ROWS, CLIPS_SHORT, CLIPS_LONG, CLIPS_MANY };
struct ClipShape { int64_t R, Tmax, out_stride; int bad_clip; int64_t bad_value; int why; };
inline ClipShape clip_shape(const int64_t* lens, const int32_t* rows, int n_clips, int64_t stride, std::vector<int64_t>& row_lens,
                            std::vector<int>& first_row)
{
    ClipShape q = {0, 0, 0, -1, 0, CLIPS_OK};
    row_lens.clear(); first_row.clear();
    for (int c = 0; c < n_clips; ++c) {
        const int64_t nr = rows ? rows[c] : 1;
        if (nr < 1) return ClipShape{0, 0, 0, c, nr, CLIPS_ROWS};
        if (lens[c] <= NFFT / 2 || lens[c] > stride) return ClipShape{0, 0, 0, c, lens[c], lens[c] > stride ? CLIPS_LONG : CLIPS_SHORT};
        q.R += nr;
        q.Tmax = std::max(q.Tmax, ragged_frames(lens[c]));
    }
    if (ragged_too_many(q.R, q.Tmax)) return ClipShape{q.R, q.Tmax, 0, -1, 0, CLIPS_MANY};
    q.out_stride = (q.Tmax - 1) * HOPS;
    row_lens.reserve((size_t)q.R); first_row.reserve((size_t)n_clips);
    for (int c = 0; c < n_clips; ++c) {
        first_row.push_back((int)row_lens.size());
        row_lens.insert(row_lens.end(), (size_t)(rows ? rows[c] : 1), lens[c]);
    }
    return q;
}

}  // namespace bsrnn
