// What the host units of libbsrnn_hip.so share (api.hip, api_stream.hip, api_resample.hip, api_pool.hip, api_critic.hip): the handle types the C ABI
// names, error plumbing, the upload ring, and the helpers every entry point opens and closes with.  Everything but the handle types lives
// in bsrnn::host; nothing here is exported (-fvisibility=hidden).  Not a public header.
#pragma once
#include "../../include/bsrnn_hip.h"
#include "kernels.h"
#include "commit_host.h"
#include "plan_host.h"
#include "resample_bank_host.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace bsrnn::host {

// --------------------------------------------------------------------------- first-use accounting (bsrnn_debug_counter)
// What the library has done that does not belong on a real-time thread: device / pinned allocations, stream captures, graph
// instantiations.  Process-wide; tests read them around the LADSPA plugin's run() (tests/test_gpu_entrypoints.py).  The fifth counts work, not
// first use: the frame rows (rows x frames) bsrnn_separate_long_ragged / bsrnn_evaluate_long_ragged have handed to the model, which is what shows
// that rows retire.
extern std::atomic<long long> g_dbg[5];
enum { DBG_ALLOC = 0, DBG_CAPTURE = 1, DBG_INSTANTIATE = 2, DBG_GRAPH_LAUNCH = 3, DBG_LONG_RAGGED_ROWS = 4 };

// --------------------------------------------------------------------------- error plumbing
// Sets the calling thread's bsrnn_last_error() text and returns `code`.
int fail(int code, const char* fmt, ...);
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(BSRNN_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// --------------------------------------------------------------------------- the upload ring
// How a small host table reaches the device in front of a call's kernels without the host waiting: `bytes` of it are written into a
// pinned mirror and copied on the caller's stream into the ONE device block `d`.  There are MIRRORS mirrors, used in turn, and mirror k is
// written again only when the copy that last read it has completed (ev[k]; an event never recorded counts as complete), so the caller's
// array is free when the call returns and calls still queue up behind each other.
// (Eight mirrors: the six ragged calls of one training step - two analyses, the synthesis, the loss and the two backward calls - queue up
// without the host waiting for a copy of the same step.)
struct UploadRing {
    static constexpr int MIRRORS = 8;
    size_t cap = 0;                               // bytes of the device block and of each mirror
    char *d = nullptr, *h = nullptr;              // h: MIRRORS mirrors of cap bytes
    unsigned turns = 0;
    hipEvent_t ev[MIRRORS] = {};

    // Blocks of exactly `bytes` unless they hold as much already.  Synchronises the device first - queued copies read the old mirrors,
    // queued kernels the old block - and frees both old blocks; on failure nothing is left allocated.
    hipError_t reserve(size_t bytes);
    // The two halves of an upload: the next mirror, once the copy that last read it has completed; that mirror k has been read on stream s
    // (after the caller's own copy out of it, to `d` or elsewhere).
    int next(char** mirror, int* k)
    {
        *k = (int)(turns++ % MIRRORS);
        HIP_TRY(hipEventSynchronize(ev[*k]));
        *mirror = h + (size_t)*k * cap;
        return 0;
    }
    int record(int k, hipStream_t s) { HIP_TRY(hipEventRecord(ev[k], s)); return 0; }
    // One upload: room for `bytes` (grow-only, geometrically), fill(mirror), the copy to `d` on stream s.
    template <class FILL>
    int upload(size_t bytes, hipStream_t s, FILL fill)
    {
        if (bytes > cap) {
            const hipError_t e = reserve((bytes + bytes / 2 + 255) & ~size_t(255));
            if (e != hipSuccess) return fail(BSRNN_EHIP, "hipMalloc: %s", hipGetErrorString(e));
        }
        char* mirror = nullptr; int k = 0;
        if (int rc = next(&mirror, &k)) return rc;
        fill(mirror);
        HIP_TRY(hipMemcpyAsync(d, mirror, bytes, hipMemcpyHostToDevice, s));
        return record(k, s);
    }
    void release();                               // everything, events included (the device is idle)
};

// --------------------------------------------------------------------------- context
struct Param {
    std::string key;
    int64_t d0 = 0, d1 = 0;
    int ndim = 1;
    std::vector<float> data;
    bool set = false;
    int64_t numel() const { return ndim == 2 ? d0 * d1 : d0; }
};

enum Stage { ST_LAYOUT, ST_STFT, ST_BANDSPLIT, ST_BAND_LSTM, ST_BAND_FC, ST_TIME_LSTM, ST_TIME_FC, ST_MASK, ST_ISTFT, ST_STREAM_DSP, NSTAGE };
struct EvRec { hipEvent_t a, b; int stage; };

}  // namespace bsrnn::host

using namespace bsrnn;
using namespace bsrnn::host;

struct bsrnn_ctx {
    int device = 0;                 // HIP ordinal; -1 = host-only context (parameter staging / file validation, no compute)
    // Concurrency contract (include/bsrnn_hip.h): one call at a time per context.  `busy` turns an overlapping call from a
    // second host thread into BSRNN_ESTATE; a call on a different HIP stream than the previous one first waits for that
    // stream on the host (the context has ONE workspace); `gen` counts reallocations of anything a captured streaming
    // graph may point at (workspace, tap buffer, weight arena) so that the graph is re-captured instead of replayed.
    std::atomic<int> busy{0};
    int range_policy = BSRNN_RANGE_EXACT;      // what a model entry point does about the fp16x2 range guard (bsrnn_set_range_policy)
    unsigned gen = 1;
    int live_streams = 0;           // bsrnn_stream objects that point at this context
    bool zombie = false;            // bsrnn_destroy() was called while streams were alive: freed with the last stream
    bool have_last = false;
    std::vector<int> widths, off;   // bins per band, start bin
    int K = 0;
    std::vector<Param> params;
    std::map<std::string, int> index;
    bool committed = false;

    // activation column layout
    std::vector<int> aoff, poff;
    int LDA = 0, LDP = 0;

    // device-resident weights and tables
    float* d_arena = nullptr;
    GemmJob* d_jobs = nullptr;
    int2* d_tiles = nullptr;
    SlotTables slots;               // jobs and tiles of every layer slot inside d_jobs / d_tiles (commit_host.h)

    // fused per-band MLP chains (mlp_chain.hip): device descriptor arrays, grouped by class (kernels.h, ChainLaunch)
    bool stage_error = false;       // run_stage() found no task table for its row count (cannot happen: ensure_tasks runs first); reported by the entry point
    bool fused = false;             // false: per-layer launches (BSRNN_MLP=layers, fp32 mode, or a band too wide for the LDS image)
    ChainDesc* d_chain[2] = {nullptr, nullptr};
    std::vector<ChainDesc> h_chain[2];          // host copies (geometry per band: the task tables are made from them)
    struct TaskTable { int2* d[2]; int n[2]; };
    std::map<int, TaskTable> chain_tasks;       // per row count M: device task tables of the two chains
    size_t task_cap = 64, ovl_cap = 16;         // bounds of the two table caches (chain_tasks, ovl_tables); bsrnn_stream_reserve raises them to
                                                // hold one table per block length it was asked for

    // recurrent weights per dual-path block, segments of the arena (commit_host.h, BlockSegs; the *16 ones hold fp16x2 pieces in MFMA operand order)
    const float *bandW[2][2], *bandB[2][2], *bandW16[2][2], *timeW[2], *timeB[2], *timeW16[2];
    const float* timeFc16[2] = {nullptr, nullptr};  // the time blocks' fc as fp16x2 B fragments (fused into the time-axis launch, lstm.hip)
    const float* timeFcB[2] = {nullptr, nullptr};
    const float* bandFc16[2] = {nullptr, nullptr};  // the band blocks' fc (128 -> 64) likewise, for the few-sequence kernel (band_block_small_kernel)
    const float* bandFcB[2] = {nullptr, nullptr};
    int *h_range = nullptr, *d_range = nullptr;    // range guard of the fp16x2 kernels: host-mapped word the kernels set
    float* d_tables = nullptr;
    float* d_train_ws = nullptr;       // grow-only scratch of the training entry points (stream-ordered reuse: one call at a time)
    size_t train_ws_floats = 0;
    std::vector<float*> train_ws_retired;   // outgrown scratch buffers: a captured training graph (train.GraphedTrainStep) may still point at
                                            // them, so they live until the context goes (growth is geometric: at most ~4x the final size in all)
    std::vector<void*> retired;             // likewise the outgrown workspaces / tap buffers / progress words (bsrnn_stft, _istft, _istft_backward and
                                            // every model entry point put workspace addresses into captured kernel nodes)
    int* d_colmap = nullptr;
    FftTables tb;
    float* d_cs_tables = nullptr;      // tables of the critic's 4096-point analysis, built and uploaded by the first bsrnn_critic_spectrum (api_critic.hip)
    CsTables cs{};

    // workspace (grow-only)
    size_t cap_rows = 0;
    float* d_ws = nullptr;
    float *Xf, *Yf, *A1, *A2, *P, *Z0, *Z1, *HB0, *HB1, *H1;
    int* band_flags = nullptr;      // band_pair_h2_kernel's hand-over flags (2 per tile of 16 frame rows + slack per row block), zero at allocation
    bool band_pair_off = false;     // a pair launch reported that its partner workgroups did not meet (value 4): one launch per layer from then on
    size_t tap_rows = 0;
    float* d_tap = nullptr;

    // profiling
    unsigned prof = 0;            // bitmask of stages bracketed by events
    std::vector<EvRec> pool;
    size_t pool_used = 0;
    double acc_ms[NSTAGE];
    int64_t acc_n[NSTAGE];
    hipStream_t last_stream = nullptr;

    // Overlapped dual path (run_overlapped below; kernels.h, OvlProducer / OvlConsumer): the second band block runs beside the first
    // time-axis launch and the mask chain beside the second, on the context's first auxiliary stream.
    bool overlap_env = true;        // BSRNN_OVERLAP=0: one launch after the other on the caller's stream (A/B; bit-identical results)
    int overlap_sabotage = 0;       // BSRNN_OVERLAP=timeout (test hook): the producers publish nothing, the consumers give up after ~2 ms
    bool overlap_off = false;       // a consumer's wait expired once (range flag value 5): this context runs launch after launch from then on
    int* d_ovl = nullptr;           // [2 time blocks][OVL_HEAD ints: resident counter | progress word per time-axis workgroup]
    int ovl_stride = 0;             // ints per block
    struct OvlTable { int2* mask_tasks; int n_mask; int* band_order; int n_ord; };
    std::map<std::pair<int, int>, OvlTable> ovl_tables;       // per (rows C, frames T): consumer dispatch orders by readiness
    hipEvent_t ev_ovl_fork = nullptr, ev_ovl_join = nullptr;
    int ovl_epoch = 0;              // overlapped calls so far on this context (upper bits of the progress words, kernels.h); reset every 2^18
    int ovl_epoch_period = 1 << 18; // (test hook BSRNN_OVL_EPOCHS: a short period exercises the reset)
    int ovl_resident_total[2] = {0, 0};      // time-axis workgroups the two resident counters have been promised so far (the gates' targets)
    bool ovl_unjoined = false;      // the auxiliary stream may still be draining the last overlapped call (a host-side join follows where one is needed)
    // How a consumer launch is held back until every workgroup of its producer is resident: a one-wave gate kernel that spins on the
    // resident counter (default).  A resident foreign wave costs a band launch its pairing (its partners sit 8 ids apart and complete inside
    // one round of 512 slots; with 511 the last eight pairs straddle two rounds: +18 us), so the gates are kept off the band launches'
    // dispatch by events (fork in front of gate 0, a mid event between band 1 and gate 1).  (A stream wait on signal memory instead of the
    // gate kernel was measured and rejected, profiles/r04_gate_kernel_vs_cp.txt: on this runtime hipStreamWaitValue32 is a blit kernel that
    // spins so hard that the time-axis launch beside it takes 3x as long.)
    hipEvent_t ev_ovl_mid = nullptr;

    // concurrent row blocks of one call (bsrnn_separate): two row blocks on two streams once the batch's time-axis launch no longer fits one
    // round of workgroups (bsrnn_separate: from 171 rows on at K = 12; until round 4, with four sequences per workgroup only, from 128 rows on),
    // the second one stage behind the first: one block's matrix work fills the other's latency-bound time-axis LSTM (192 of 256
    // CUs, serial chain) and the ramps / tails of the fused chain launches (+8-12 % at 128 rows).  At the benchmark's 64 rows
    // two blocks of 32 gain 3 % (1.157 -> 1.119 ms per step) but every kernel then runs beside another
    // block's kernels: the per-kernel durations (and with them the roofline figure of bench.py) stop describing the kernel,
    // so one block there.  Rows are independent; tests/test_gpu_edges.py checks 64- and 130-row calls bit for bit against
    // their row blocks.  (That check first failed: see the note at the top of fft.hip.)
    hipStream_t aux[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[4] = {nullptr, nullptr, nullptr, nullptr};

    // Long-form separation (bsrnn_separate_long / _long_host): what one segment of a clip hands to the next - the time-axis LSTM state and
    // the synthesis carry (the windowed second half of the segment's last frame) - exists twice, like a bsrnn_stream's carry: segment i
    // reads set i & 1 and writes the other one, so a segment that leaves the fp16 range is run again from its untouched starting point.
    // The host-buffer entry point stages through two pinned input windows and two pinned output blocks with device mirrors of the same
    // sizes, copied on a stream of their own.  All of it is sized by (rows, frames per segment), never by the clip.
    struct LongForm {
        int rows = 0;                                         // rows the carry sets were made for (grow-only)
        float *state[2] = {nullptr, nullptr}, *carry[2] = {nullptr, nullptr};      // one allocation, state[0] its base
        size_t in_floats = 0, out_floats = 0;                 // floats per input window / output block of the staging (grow-only)
        float *h_base = nullptr, *d_base = nullptr;           // the pinned and the device allocation: [in 0 | in 1 | out 0 | out 1]
        float *h_in[2], *h_out[2], *d_in[2], *d_out[2];
        hipStream_t copy = nullptr;
        // per block: its H2D has completed / the segment that read d_in and wrote d_out is final / its D2H has completed
        hipEvent_t ev_h2d[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_d2h[2] = {nullptr, nullptr};
    } lf;

    // Ragged batches (bsrnn_separate_ragged): what the kernels of one call read besides the waveform - the rows' lengths and, for the fused
    // chains, the task tables of its R * Tmax frame rows - travels as ONE block [R int64 lengths | split tasks | mask tasks], copied on the
    // caller's stream into `d` in front of the call's kernels.  (Not the table cache above: a ragged caller meets another Tmax with nearly
    // every call, and a cached table per frame-row count would make first-use work the rule and flush the bounded cache.)  Grow-only.
    UploadRing rg;

    // The evaluate calls (bsrnn_evaluate, bsrnn_evaluate_ragged, bsrnn_evaluate_long_ragged): the metric kernels' table [R int64 row lengths |
    // n_clips MetricClip] travels through a ring of its own - the bsrnn_separate_ragged inside an evaluate call overwrites rg's device block -
    // and their scratch is two device blocks, the sums (doubles; accumulators in the segmented call) with a pinned mirror for the one
    // download of a call, and the estimate when the caller wants none: [R][n_est], or ONE segment [R][seg * 1024] in the segmented call.
    // All grow-only: a call that fits allocates nothing, and the blocks are RETAINED until the context goes - the estimate block too, about
    // 32 MB after a bsrnn_evaluate of 64 rows x 128 000 samples without est_out.
    struct EvalRagged {
        UploadRing table;
        size_t part_cap = 0, est_cap = 0;             // doubles / floats the scratch holds
        double *d_part = nullptr, *h_part = nullptr;
        float* d_est = nullptr;
    } er;

    // Sample-rate conversion (bsrnn_resample, bsrnn_resampler_*): the polyphase table of each reduced (up, down) this context has met, designed
    // on the host and uploaded at first use (bsrnn_debug_counter(0)); grow-only, a handful of entries of at most 100 KB, freed with the context.
    struct ResampleTable { ResampleRatio q; ResampleTiling g; float* d; };
    std::vector<ResampleTable> rs_tables;

    // Long FIR convolution (bsrnn_convolve_ragged): the two spectrum buffers of a row group, `frames` spectra of CONV_LD floats each.
    // Grow-only; the row table of a call travels in the ragged calls' block above (rg).
    struct Conv {
        float *X = nullptr, *Y = nullptr;
        int64_t frames = 0;
    } cv;
};

struct bsrnn_stream {
    bsrnn_ctx* ctx;
    int C;
    // What a step carries to the next one - the sliding analysis buffer, the previous synthesis frame and the LSTM state - exists
    // twice: step k reads set k & 1 and writes the other one, so a step whose operands leave the fp16 range can be run again,
    // exactly, from its untouched starting point (range policy, finish_call), without a copy per step.
    float *base = nullptr;             // the one allocation
    float *buf[2], *prev[2], *state[2];
    int cur = 0;                       // the set the NEXT step reads
    float *X, *Y, *chunk, *out;
    int* row_frames = nullptr;         // [C]: the hops of every row of a bsrnn_stream_process_hops call (its analysis launch writes them, its time-axis launches read them)
    float *h_in = nullptr, *h_out = nullptr;   // pinned staging for the host-buffer entry point
    // One step = analysis, ~18 launches of the model, synthesis.  The model part works on fixed buffers (X -> Y, state set p -> set
    // 1 - p), so it is captured once per parity into a hipGraph and replayed (launch-bound inner loop); the two DSP kernels are
    // launched around it with the caller's own chunk / output pointers and the wet/dry control as a kernel argument (no staging copies).
    hipGraphExec_t exec[2] = {nullptr, nullptr};
    hipGraph_t graph[2] = {nullptr, nullptr};
    hipStream_t cap = nullptr;
    bool use_graph = true;
    unsigned gen = 0;                  // context generation the graphs were captured against
};

// A bank of streaming resamplers: every row on one of the declared pairs and at its own place in its own stream, one launch per call
// (per BANK_GROUP_ROWS rows).  The per-row arithmetic: resample_bank_host.h; the kernel: resample_bank_kernel of resample.hip.
struct bsrnn_resampler_bank {
    bsrnn_ctx* ctx;
    int C, n_pairs;
    ResampleRatio q[BANK_PAIRS_MAX];
    int tile[BANK_PAIRS_MAX];
    BankPair* pairs;                 // [n_pairs] on the device, written by _create and constant afterwards
    float* carry;                    // two sets of C * cap floats; row r's current set is pos[r].cur
    int64_t cap;                     // the largest resample_carry_floats of the declared pairs
    std::vector<BankPos> pos, next;  // [C]: where every row stands; next is a call's scratch (nothing is allocated after _create)
    std::vector<BankRow> desc;       // [C], a call's descriptors
    std::vector<uint8_t> seen;       // [C], for "a row listed twice"
};

namespace bsrnn::host {

struct StageScope {   // brackets one stage of a call with events when profiling is on
    bsrnn_ctx* c; hipStream_t s; EvRec* r = nullptr;
    StageScope(bsrnn_ctx* c_, int stage, hipStream_t s_) : c(c_), s(s_)
    {
        if (((c->prof >> stage) & 1u) && c->pool_used < c->pool.size()) {
            r = &c->pool[c->pool_used++];
            r->stage = stage;
            (void)hipEventRecord(r->a, s);
        }
    }
    ~StageScope() { if (r) (void)hipEventRecord(r->b, s); }
};

// --------------------------------------------------------------------------- helpers of the entry points (defined and described in api.hip)
int ensure_ws(bsrnn_ctx* c, size_t rows);
int ensure_tasks(bsrnn_ctx* c, const int* Ms, int n);
int ensure_tasks(bsrnn_ctx* c, int M);
Flow plan_call(const bsrnn_ctx* c, int C, int T, bool gemv, bool overlap);
int ensure_ovl(bsrnn_ctx* c, const Flow& f, int C, int T);
int ovl_join_host(bsrnn_ctx* c);
int run_model(bsrnn_ctx* c, const float* Xf, float* Yf, float* tap, int C, int T, const float* state_in, float* state_out, hipStream_t s,
              const int* row_frames = nullptr);
int take_guard(bsrnn_ctx* c);
int guard_fallback(bsrnn_ctx* c, int v, const char* who);
int check_range(bsrnn_ctx* c);
int check_device(bsrnn_ctx* c, bool model = false);
int check_ready(bsrnn_ctx* c);
int order_after_last(bsrnn_ctx* c, hipStream_t s);
float* train_scratch(bsrnn_ctx* c, size_t floats);      // the grow-only scratch of the training entry points; null when out of memory
void destroy_now(bsrnn_ctx* c);      // the end of a context: bsrnn_destroy, or the last object that pointed at a context destroyed before it

// True when the byte ranges [a, a + na) and [b, b + nb) share a byte (null pointers share none).  A call whose re-run (finish_call)
// reads an input that the first run's outputs may have overwritten is refused on this test, not just on pointer equality.
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

// End of a model entry point under the default range policy (include/bsrnn_hip.h; any_policy: whatever the context's policy): wait for
// the call's own kernels, look at the guard word the fp16x2 kernels set, and if it is set run the call again before returning - never
// wrong numbers with rc 0.  Structural fall-backs first (guard_fallback: the context switches flow; at most two such re-runs, one per
// kind), then for an operand that left the fp16 range the library's exact-fp32 kernels (fp32 weights are always resident; no range limit).
template <class F>
int finish_call(bsrnn_ctx* c, hipStream_t s, F&& rerun, bool any_policy = false)
{
    if ((c->range_policy != BSRNN_RANGE_EXACT && !any_policy) || !c->h_range || force_f32()) return 0;
    if (gemm_mode() == GEMM_F32 && lstm_mode() == LSTM_F32) return 0;
    for (int reruns = 0;; ++reruns) {
        HIP_TRY(hipStreamSynchronize(s));
        if (int rcj = ovl_join_host(c)) return rcj;      // (the second time-axis launch of an overlapped call ran on the auxiliary stream: its guard word too)
        const int v = take_guard(c);
        if (!v) return 0;
        if (v != 3 && v != 4 && v != 5) break;
        const int rc = guard_fallback(c, v, "the call");
        if (v == 3 || reruns == 2) return rc;
        if (int rc2 = rerun()) return rc2;
    }
    set_force_f32(true);
    const int rc = rerun();
    set_force_f32(false);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// One call at a time per context: an overlapping call from another host thread is refused instead of racing on the
// workspace.  (Re-entrant on the same thread: bsrnn_evaluate -> bsrnn_separate, stream_step_host -> stream_step.)
struct CallGuard {
    bsrnn_ctx* c; bool ok, outer;
    explicit CallGuard(bsrnn_ctx* c_);
    ~CallGuard();
    int refuse() const;
};
#define ENTER_CALL(c, s)                                   \
    CallGuard guard_(c);                                   \
    if (!guard_.ok) return guard_.refuse();                \
    { int rc_ = order_after_last(c, s); if (rc_) return rc_; }

// Sample-rate pairs as every entry point checks them (api_resample.hip; the pool declares its rates through it)
int resample_check_rates(int32_t rate_in, int32_t rate_out, const char* who, ResampleRatio& q);

}  // namespace bsrnn::host
