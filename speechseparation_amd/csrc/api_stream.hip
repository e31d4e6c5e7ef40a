// C ABI of libbsrnn_hip.so, streaming (bsrnn_stream_*): the stream object, the one-hop step and its captured graph, the block calls
// with all rows, a held set or a hop count per row, and the session-slot helpers.  Context and shared helpers: api_internal.h / api.hip.
#include "api_internal.h"

extern "C" {

// --------------------------------------------------------------------------- streaming
// Device layout of a stream object: two carry sets [buf | prev | state] (see bsrnn_stream), then the per-step scratch [X | Y | chunk | out]
// and the hop counts of a hops call [row_frames].
static size_t stream_carry_floats(const bsrnn_ctx* c, int C) { return (size_t)C * NFFT * 2 + state_floats(C, c->K); }
static size_t stream_total_floats(const bsrnn_ctx* c, int C)
{
    return 2 * stream_carry_floats(c, C) + (size_t)C * ((size_t)c->LDP * 2 + HOPS * 2 + 1) + 4;      // (+ 1: row_frames, one word per row)
}

int bsrnn_stream_create(bsrnn_ctx* c, int32_t C, bsrnn_stream** out)
{
    int rc = check_ready(c);
    if (rc) return rc;
    if (!out || C < 1) return fail(BSRNN_EARG, "bsrnn_stream_create: bad arguments");
    CallGuard guard_(c);
    if (!guard_.ok) return guard_.refuse();
    bsrnn_stream* st = new bsrnn_stream();
    st->ctx = c; st->C = C;
    const size_t nstate = state_floats(C, c->K);
    const size_t total = stream_total_floats(c, C);
    float* p = nullptr;
    ++g_dbg[DBG_ALLOC];
    hipError_t e = hipMalloc((void**)&p, total * sizeof(float));
    if (e != hipSuccess) { delete st; return fail(BSRNN_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
    st->base = p;
    for (int k = 0; k < 2; ++k) {
        st->buf[k] = p; p += (size_t)C * NFFT;
        st->prev[k] = p; p += (size_t)C * NFFT;
        st->state[k] = p; p += nstate;
    }
    st->X = p; p += (size_t)C * c->LDP;
    st->Y = p; p += (size_t)C * c->LDP;
    st->chunk = p; p += (size_t)C * HOPS;
    st->out = p; p += (size_t)C * HOPS;
    st->row_frames = reinterpret_cast<int*>(p); p += C;
    // The model part of a step as plain launches (default) or as one hipGraph per carry parity (BSRNN_STREAM_GRAPH=1).  Measured from C
    // (tools/stream_cloop.cpp, profiles/r04_stream_kernels.txt): the graph launch of the 14 dependent kernel nodes costs the host MORE than
    // 14 plain launches (78 vs 68 us inside the call) and the chunk 143.2 vs 139.5 us - the gaps between dependent kernels are the same
    // inside a replayed graph - so the cheaper form is the default; the graph path stays for A/B (BSRNN_NO_GRAPH is accepted and means the default).
    st->use_graph = getenv("BSRNN_STREAM_GRAPH") != nullptr && getenv("BSRNN_NO_GRAPH") == nullptr;
    if (hipHostMalloc((void**)&st->h_in, (size_t)C * HOPS * sizeof(float), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&st->h_out, (size_t)C * HOPS * sizeof(float), hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(st->base); delete st; return fail(BSRNN_EHIP, "hipHostMalloc failed");
    }
    e = hipMemset(st->base, 0, total * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(st->base); delete st; return fail(BSRNN_EHIP, "hipMemset: %s", hipGetErrorString(e)); }
    rc = ensure_ws(c, C);
    if (!rc) rc = ensure_tasks(c, C);
    if (rc) { (void)hipHostFree(st->h_in); (void)hipHostFree(st->h_out); (void)hipFree(st->base); delete st; return rc; }
    ++c->live_streams;
    // Everything a first step would otherwise do on the caller's (audio) thread happens here, as the reference does in its constructor
    // (speech-ladspa-onnx.cpp:55-120: session, FFT plans, state): one throw-away step per carry parity through the host-buffer entry
    // point - it loads every kernel's code object, captures and instantiates both parity graphs and touches the pinned staging
    // buffers - then the carry sets are zeroed again.  bsrnn_stream_step / _step_host allocate, capture and instantiate nothing
    // afterwards unless the context's workspace or weights change under the stream (generation counter).
    {
        std::vector<float> zero((size_t)C * HOPS, 0.f), sink((size_t)C * HOPS);
        for (int k = 0; k < 2 && !rc; ++k) rc = bsrnn_stream_step_host(st, zero.data(), sink.data(), 1.0f);
        if (!rc && hipMemset(st->base, 0, total * sizeof(float)) != hipSuccess) rc = fail(BSRNN_EHIP, "hipMemset failed");
        if (!rc && hipDeviceSynchronize() != hipSuccess) rc = fail(BSRNN_EHIP, "hipDeviceSynchronize failed");
        st->cur = 0;
        if (rc) { bsrnn_stream_destroy(st); return rc; }
    }
    *out = st;
    return 0;
}

static void stream_drop_graph(bsrnn_stream* st)
{
    for (int k = 0; k < 2; ++k) {
        if (st->exec[k]) { (void)hipGraphExecDestroy(st->exec[k]); st->exec[k] = nullptr; }
        if (st->graph[k]) { (void)hipGraphDestroy(st->graph[k]); st->graph[k] = nullptr; }
    }
}

void bsrnn_stream_destroy(bsrnn_stream* st)
{
    if (!st) return;
    bsrnn_ctx* c = st->ctx;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    stream_drop_graph(st);
    if (st->cap) (void)hipStreamDestroy(st->cap);
    if (st->h_in) (void)hipHostFree(st->h_in);
    if (st->h_out) (void)hipHostFree(st->h_out);
    (void)hipFree(st->base);
    delete st;
    if (--c->live_streams == 0 && c->zombie) destroy_now(c);     // bsrnn_destroy() came first: the context goes with its last stream
}

int bsrnn_stream_reset(bsrnn_stream* st, void* stream)
{
    if (!st) return fail(BSRNN_EARG, "null stream");
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipMemsetAsync(st->base, 0, stream_total_floats(st->ctx, st->C) * sizeof(float), (hipStream_t)stream));
    st->cur = 0;
    return 0;
}

// One step from carry set p = st->cur into set 1 - p: chunk -> out (device pointers of the caller or the object's own buffers).
// The model part is a graph replay when possible.  Does NOT flip st->cur: the caller does, once the step is known to be good.
// rows (kernels.h, StreamRows), HELD: only the rows of rows.active take the step; the others are held by the two DSP launches (the model part
// is the same, captured graph included: a held row enters it as a zero spectrum, and the synthesis launch - behind every launch of the
// model in stream order - puts its LSTM state back).
static const StreamRows kAllRows{};
static int stream_step_run(bsrnn_stream* st, const float* chunk, float* out, float mix, hipStream_t s, const StreamRows& rows = kAllRows)
{
    bsrnn_ctx* c = st->ctx;
    const int p = st->cur, q = p ^ 1;
    int rc;
    {
        StageScope sc(c, ST_STREAM_DSP, s);
        launch_stream_analysis(c->tb, st->buf[p], st->buf[q], chunk, st->X, st->C, rows, s);
    }
    if (st->use_graph && c->prof == 0 && !force_f32()) {
        // The captured launches hold the context's workspace and weight-arena pointers.  A larger call on the context (workspace
        // regrown) or a re-commit of the parameters (arena rebuilt) since the capture changes ctx->gen: capture again
        // instead of replaying launches that point into freed memory.
        if ((st->exec[0] || st->exec[1]) && st->gen != c->gen) {
            HIP_TRY(hipDeviceSynchronize());
            stream_drop_graph(st);
        }
        if (!st->exec[p]) {
            if (!st->cap) { ++g_dbg[DBG_ALLOC]; HIP_TRY(hipStreamCreateWithFlags(&st->cap, hipStreamNonBlocking)); }
            ++g_dbg[DBG_CAPTURE];
            HIP_TRY(hipStreamBeginCapture(st->cap, hipStreamCaptureModeThreadLocal));
            rc = run_model(c, st->X, st->Y, nullptr, st->C, 1, st->state[p], st->state[q], st->cap);
            hipGraph_t g = nullptr;
            hipError_t e = hipStreamEndCapture(st->cap, &g);           // (always ended, whatever run_model said: the stream must leave capture mode)
            if (rc || e != hipSuccess) {
                if (g) (void)hipGraphDestroy(g);                       // a failed capture leaves nothing behind
                (void)hipGetLastError();
                if (rc) return rc;
                return fail(BSRNN_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
            }
            ++g_dbg[DBG_INSTANTIATE];
            e = hipGraphInstantiate(&st->exec[p], g, nullptr, nullptr, 0);
            if (e != hipSuccess) {
                (void)hipGraphDestroy(g);
                st->exec[p] = nullptr;
                return fail(BSRNN_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
            }
            st->graph[p] = g;
            st->gen = c->gen;
        }
        ++g_dbg[DBG_GRAPH_LAUNCH];
        HIP_TRY(hipGraphLaunch(st->exec[p], s));
    } else if ((rc = run_model(c, st->X, st->Y, nullptr, st->C, 1, st->state[p], st->state[q], s))) {
        return rc;
    }
    {
        StageScope sc(c, ST_STREAM_DSP, s);
        launch_stream_synthesis(c->tb, st->Y, st->X, mix, st->prev[p], st->prev[q], out, st->state[p], st->state[q], st->C, c->K, rows, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_stream_step(bsrnn_stream* st, const float* chunk, float* out, float mix, void* stream)
{
    if (!st || !chunk || !out) return fail(BSRNN_EARG, "bsrnn_stream_step: null argument");
    bsrnn_ctx* c = st->ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if ((rc = ensure_ws(c, st->C)) || (rc = ensure_tasks(c, st->C))) return rc;
    const float* src = chunk;
    const size_t nb = (size_t)st->C * HOPS * sizeof(float);
    if (ranges_overlap(chunk, nb, out, nb) && c->range_policy == BSRNN_RANGE_EXACT) {
        // in place, or partly: a re-run (range policy) must still see the input, so it is kept aside first
        HIP_TRY(hipMemcpyAsync(st->chunk, chunk, (size_t)st->C * HOPS * sizeof(float), hipMemcpyDeviceToDevice, s));
        src = st->chunk;
    }
    if ((rc = stream_step_run(st, src, out, mix, s))) return rc;
    // default range policy: wait, look at the guard, and if an operand left the fp16 range run the step again on the exact-fp32
    // kernels from the same (untouched) carry set
    if ((rc = finish_call(c, s, [&]() -> int { return stream_step_run(st, src, out, mix, s); }))) return rc;
    st->cur ^= 1;
    return 0;
}

int bsrnn_stream_step_host(bsrnn_stream* st, const float* chunk_host, float* out_host, float mix)
{
    if (!st || !chunk_host || !out_host) return fail(BSRNN_EARG, "bsrnn_stream_step_host: null argument");
    bsrnn_ctx* c = st->ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    ENTER_CALL(c, (hipStream_t) nullptr);
    const size_t nb = (size_t)st->C * HOPS * sizeof(float);
    memcpy(st->h_in, chunk_host, nb);
    HIP_TRY(hipMemcpyAsync(st->chunk, st->h_in, nb, hipMemcpyHostToDevice, nullptr));
    // This entry point waits for its own kernels anyway, so it repairs a range violation whatever the policy says
    const int keep = c->range_policy;
    c->range_policy = BSRNN_RANGE_EXACT;
    rc = bsrnn_stream_step(st, st->chunk, st->out, mix, nullptr);
    c->range_policy = keep;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(st->h_out, st->out, nb, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    memcpy(out_host, st->h_out, nb);
    return 0;
}

// L hops from carry set p = st->cur into set 1 - p: chunk [C][L*1024] -> out [C][L*1024], the spectra in the context's workspace (one call
// at a time per context).  Does NOT flip st->cur (see stream_step_run).
// HELD: as for stream_step_run.  On the overlapped plan the second time-axis launch writes its half of state[q] on the auxiliary stream;
// run_overlapped joins that stream into `s` by an event for every call that returns LSTM state - this one does - so the synthesis launch,
// which copies the held rows' state over what the model wrote, follows both.
// HOPS (bsrnn_stream_process_hops): row r advances by its own count.  The analysis launch leaves the counts in st->row_frames, the two
// time-axis launches return every row's state after ITS last frame, and the synthesis - which follows both, as above - holds the rows at 0.
static int stream_block_run(bsrnn_stream* st, const float* chunk, float* out, int L, float mix, hipStream_t s, const StreamRows& rows = kAllRows)
{
    bsrnn_ctx* c = st->ctx;
    const int p = st->cur, q = p ^ 1;
    {
        StageScope sc(c, ST_STREAM_DSP, s);
        launch_stream_block_analysis(c->tb, st->buf[p], st->buf[q], chunk, c->Xf, st->C, L, rows, st->row_frames, s);
    }
    if (int rc = run_model(c, c->Xf, c->Yf, nullptr, st->C, L, st->state[p], st->state[q], s, rows.kind == StreamRows::HOPS ? st->row_frames : nullptr)) return rc;
    {
        StageScope sc(c, ST_STREAM_DSP, s);
        launch_stream_block_synthesis(c->tb, c->Yf, c->Xf, mix, st->prev[p], st->prev[q], out, st->state[p], st->state[q], st->C, c->K, L, rows, s);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// What the three front doors (bsrnn_stream_process, _process_rows, _process_hops; `who`) share: the buffers they refuse ...
static int stream_refuse_overlap(const char* who, const bsrnn_stream* st, const float* chunk, const float* out, int n_hops, const float* mix_rows)
{
    const size_t nb = (size_t)st->C * n_hops * HOPS * sizeof(float);
    if (st->ctx->range_policy == BSRNN_RANGE_EXACT && ranges_overlap(chunk, nb, out, nb))
        return fail(BSRNN_EARG, "%s: out_dev must not overlap chunk_dev under the exact range policy (the re-run of a call that leaves the fp16 range reads chunk_dev again)", who);
    if (ranges_overlap(mix_rows, (size_t)st->C * sizeof(float), chunk, nb) || ranges_overlap(mix_rows, (size_t)st->C * sizeof(float), out, nb))
        return fail(BSRNN_EARG, "%s: mix_rows_dev must overlap neither chunk_dev nor out_dev", who);
    return 0;
}
// ... and, behind their delegations, the call.  One hop: the step's kernels and its captured graph; more: the block path.  Both read carry set cur
// and write the other one, for held rows too: the re-run of the range policy starts from the untouched set, same rows, same counts.  none: no row takes a hop.
static int stream_call(const char* who, bsrnn_stream* st, const float* chunk, float* out, int n_hops, float mix, const StreamRows& rows, bool none, void* stream)
{
    bsrnn_ctx* c = st->ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if (none) { HIP_TRY(hipMemsetAsync(out, 0, (size_t)st->C * n_hops * HOPS * sizeof(float), s)); return 0; }
    const size_t M = (size_t)st->C * n_hops;
    if (M > (size_t)INT32_MAX / 2) return fail(BSRNN_EARG, "%s: %d rows x %d hops is too many frame rows for one call", who, st->C, n_hops);
    if ((rc = ensure_ws(c, M)) || (rc = ensure_tasks(c, (int)M))) return rc;
    auto run = [&]() -> int { return n_hops == 1 ? stream_step_run(st, chunk, out, mix, s, rows) : stream_block_run(st, chunk, out, n_hops, mix, s, rows); };
    if ((rc = run())) return rc;
    if ((rc = finish_call(c, s, run))) return rc;
    st->cur ^= 1;
    return 0;
}

int bsrnn_stream_process(bsrnn_stream* st, const float* chunk, float* out, int32_t n_hops, float mix, void* stream)
{
    if (!st || !chunk || !out) return fail(BSRNN_EARG, "bsrnn_stream_process: null argument");
    if (n_hops < 1) return fail(BSRNN_EARG, "bsrnn_stream_process: n_hops = %d (at least one hop)", n_hops);
    if (int rc = check_ready(st->ctx)) return rc;                                 // (this front door answers a context that cannot compute first)
    if (int rc = stream_refuse_overlap("bsrnn_stream_process", st, chunk, out, n_hops, nullptr)) return rc;
    if (n_hops == 1) return bsrnn_stream_step(st, chunk, out, mix, stream);       // the step itself: bit-identical by construction
    return stream_call("bsrnn_stream_process", st, chunk, out, n_hops, mix, kAllRows, false, stream);
}

int bsrnn_stream_reserve(bsrnn_stream* st, int32_t max_hops)
{
    if (!st || max_hops < 1) return fail(BSRNN_EARG, "bsrnn_stream_reserve: bad arguments");
    bsrnn_ctx* c = st->ctx;
    int rc = check_ready(c);
    if (rc) return rc;
    ENTER_CALL(c, (hipStream_t) nullptr);
    const int C = st->C;
    if ((size_t)C * max_hops > (size_t)INT32_MAX / 2) return fail(BSRNN_EARG, "bsrnn_stream_reserve: %d rows x %d hops is too many frame rows for one call", C, max_hops);
    if ((rc = ensure_ws(c, (size_t)C * max_hops))) return rc;
    // one task table and (where the plan overlaps the dual path) one pair of dispatch orders per block length: they are keyed by the row
    // count, and a later call of any length up to max_hops must find its own.  The caches' bounds grow so that this set fits beside what
    // is there already (a few KB per table).
    std::vector<int> ms;
    size_t missing = 0, ovl_missing = 0;
    for (int L = 1; L <= max_hops; ++L) {
        ms.push_back(C * L);
        missing += c->fused && c->chain_tasks.find(C * L) == c->chain_tasks.end();
        ovl_missing += plan_call(c, C, L, true, true).overlap && c->ovl_tables.find(std::make_pair(C, L)) == c->ovl_tables.end();
    }
    c->task_cap = std::max(c->task_cap, c->chain_tasks.size() + missing);
    c->ovl_cap = std::max(c->ovl_cap, c->ovl_tables.size() + ovl_missing + 1);
    if ((rc = ensure_tasks(c, ms.data(), (int)ms.size()))) return rc;
    for (int L = 1; L <= max_hops; ++L)
        if ((rc = ensure_ovl(c, plan_call(c, C, L, true, true), C, L))) return rc;
    // Load the kernels of every plan a block can take (GEMV rows, few-row band block, chains, overlapped dual path) and fill the launchers'
    // function-local statics: throw-away blocks of zeros from the current carry set into the OTHER one, which the next real call
    // overwrites completely (cur is not flipped).
    const int cand[4] = {2, 8, 31, max_hops};
    float* tmp = nullptr;
    const size_t nfl = (size_t)C * max_hops * HOPS;
    ++g_dbg[DBG_ALLOC];
    HIP_TRY(hipMalloc((void**)&tmp, 2 * nfl * sizeof(float)));
    hipError_t e = hipMemset(tmp, 0, 2 * nfl * sizeof(float));
    int last = 1;
    for (int i = 0; i < 4 && !rc && e == hipSuccess; ++i) {
        const int L = std::min(cand[i], (int)max_hops);
        if (L <= last) continue;
        last = L;
        rc = stream_block_run(st, tmp, tmp + nfl, L, 1.0f, nullptr);
        if (!rc) rc = stream_block_run(st, tmp, tmp + nfl, L, 0.5f, nullptr);
        if (C <= STREAM_ROWS_MAX && L <= STREAM_HOPS_MAX) {      // ... and of the same plans as bsrnn_stream_process_hops runs them (the ragged time-axis kernels, the HopRows DSP pair)
            StreamRows ha;
            RowHopsInfo info;
            std::vector<int32_t> cnt((size_t)C);
            for (int r = 0; r < C; ++r) cnt[r] = L - (r & 1);
            ha.kind = StreamRows::HOPS;
            if (pack_row_hops(cnt.data(), C, L, ha.hops, info) < 0) {
                if (!rc) rc = stream_block_run(st, tmp, tmp + nfl, L, 1.0f, nullptr, ha);
                if (!rc) rc = stream_block_run(st, tmp, tmp + nfl, L, 0.5f, nullptr, ha);
            }
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (!rc) rc = ovl_join_host(c);
    (void)hipFree(tmp);
    if (rc) return rc;
    if (e != hipSuccess) return fail(BSRNN_EHIP, "bsrnn_stream_reserve: %s", hipGetErrorString(e));
    return check_range(c);
}

int bsrnn_stream_get_state(bsrnn_stream* st, float* state_host)
{
    if (!st || !state_host) return fail(BSRNN_EARG, "null argument");
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t nstate = state_floats(st->C, st->ctx->K);
    HIP_TRY(hipMemcpy(state_host, st->state[st->cur], nstate * sizeof(float), hipMemcpyDeviceToHost));
    return check_range(st->ctx);          // steps made under the 'deferred' policy report a range violation here (or at the next call / bsrnn_sync)
}

// --------------------------------------------------------------------------- streaming, row by row (session slots)
static_assert(BSRNN_STREAM_ROWS_MAX == STREAM_ROWS_MAX, "include/bsrnn_hip.h and stream_rows_host.h disagree");

int bsrnn_stream_process_rows(bsrnn_stream* st, const float* chunk, float* out, int32_t n_hops, const uint8_t* active_host, const float* mix_rows,
                              float mix, void* stream)
{
    if (!st || !chunk || !out) return fail(BSRNN_EARG, "bsrnn_stream_process_rows: null argument");
    if (n_hops < 1) return fail(BSRNN_EARG, "bsrnn_stream_process_rows: n_hops = %d (at least one hop)", n_hops);
    StreamRows ra;
    ra.kind = StreamRows::HELD; ra.mix_rows = mix_rows;
    const int n_active = pack_row_set(active_host, st->C, ra.active);      // (the caller's array is not looked at again)
    if (n_active < 0)
        return fail(BSRNN_EARG, "bsrnn_stream_process_rows: the stream has %d rows, the rows calls take at most BSRNN_STREAM_ROWS_MAX = %d", st->C, STREAM_ROWS_MAX);
    if (int rc = stream_refuse_overlap("bsrnn_stream_process_rows", st, chunk, out, n_hops, mix_rows)) return rc;
    // every row, one wet / dry value: the plain call itself
    if (n_active == st->C && !mix_rows) return bsrnn_stream_process(st, chunk, out, n_hops, mix, stream);
    return stream_call("bsrnn_stream_process_rows", st, chunk, out, n_hops, mix, ra, n_active == 0, stream);
}

static_assert(BSRNN_STREAM_HOPS_MAX == STREAM_HOPS_MAX, "include/bsrnn_hip.h and stream_rows_host.h disagree");

int bsrnn_stream_process_hops(bsrnn_stream* st, const float* chunk, float* out, int32_t n_hops, const int32_t* hops_host, const float* mix_rows,
                              float mix, void* stream)
{
    if (n_hops < 1 || n_hops > STREAM_HOPS_MAX)
        return fail(BSRNN_EARG, "bsrnn_stream_process_hops: n_hops = %d (1 to BSRNN_STREAM_HOPS_MAX = %d hops per call)", n_hops, STREAM_HOPS_MAX);
    if (!st || !chunk || !out || !hops_host) return fail(BSRNN_EARG, "bsrnn_stream_process_hops: null argument");
    if (st->C > STREAM_ROWS_MAX)
        return fail(BSRNN_EARG, "bsrnn_stream_process_hops: the stream has %d rows, the rows calls take at most BSRNN_STREAM_ROWS_MAX = %d", st->C, STREAM_ROWS_MAX);
    StreamRows ha;
    RowHopsInfo info;
    ha.kind = StreamRows::HOPS; ha.mix_rows = mix_rows;
    const int bad = pack_row_hops(hops_host, st->C, n_hops, ha.hops, info);      // (the caller's array is not looked at again, but for the delegation below)
    if (bad >= 0) return fail(BSRNN_EARG, "bsrnn_stream_process_hops: row %d has %d hops, outside [0, n_hops = %d]", bad, hops_host[bad], n_hops);
    if (int rc = stream_refuse_overlap("bsrnn_stream_process_hops", st, chunk, out, n_hops, mix_rows)) return rc;
    // every count 0 or n_hops (none at all included): the rows call itself, bit-identical by construction, one-hop graph path and all
    if (info.all_or_none) {
        std::vector<uint8_t> active((size_t)st->C);
        for (int r = 0; r < st->C; ++r) active[r] = hops_host[r] != 0;
        return bsrnn_stream_process_rows(st, chunk, out, n_hops, active.data(), mix_rows, mix, stream);
    }
    // mixed counts always take the block path (n_hops >= 2 here)
    return stream_call("bsrnn_stream_process_hops", st, chunk, out, n_hops, mix, ha, false, stream);
}

int bsrnn_stream_reset_rows(bsrnn_stream* st, const int32_t* rows_host, int32_t n_rows, void* stream)
{
    if (!st) return fail(BSRNN_EARG, "bsrnn_stream_reset_rows: null stream");
    if (!rows_host || n_rows < 1) return fail(BSRNN_EARG, "bsrnn_stream_reset_rows: no rows (null list or n_rows = %d)", n_rows);
    if (st->C > STREAM_ROWS_MAX)
        return fail(BSRNN_EARG, "bsrnn_stream_reset_rows: the stream has %d rows, the rows calls take at most BSRNN_STREAM_ROWS_MAX = %d", st->C, STREAM_ROWS_MAX);
    RowSet rs;
    const int bad = pack_row_list(rows_host, n_rows, st->C, rs);
    if (bad >= 0) return fail(BSRNN_EARG, "bsrnn_stream_reset_rows: row %d (entry %d of the list) is outside [0, %d)", rows_host[bad], bad, st->C);
    HIP_TRY(hipSetDevice(st->ctx->device));
    launch_stream_reset_rows(st->buf[st->cur], st->prev[st->cur], st->state[st->cur], st->C, st->ctx->K, rs, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t bsrnn_stream_row_floats(const bsrnn_stream* st) { return st ? stream_row_floats(st->ctx->K) : -1; }

// One row's carry <-> blob [buf 2048 | prev 2048 | state 4*2 slabs of K*64]: two plain copies and one strided one (the row's slab is
// K*64 contiguous floats at dim 2 = row*K of each of the eight [C*K][64] slabs).
static int stream_move_row(bsrnn_stream* st, int row, float* blob, bool get)
{
    bsrnn_ctx* c = st->ctx;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    const int p = st->cur;
    const size_t slab = (size_t)c->K * HID * sizeof(float), pitch = slab * st->C;
    float* buf = st->buf[p] + (size_t)row * NFFT;
    float* prev = st->prev[p] + (size_t)row * NFFT;
    float* state = st->state[p] + (size_t)row * c->K * HID;
    if (get) {
        HIP_TRY(hipMemcpy(blob, buf, NFFT * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(blob + NFFT, prev, NFFT * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(blob + 2 * NFFT, slab, state, pitch, slab, 8, hipMemcpyDeviceToHost));
    } else {
        HIP_TRY(hipMemcpy(buf, blob, NFFT * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(prev, blob + NFFT, NFFT * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy2D(state, pitch, blob + 2 * NFFT, slab, slab, 8, hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());
    }
    return 0;
}

int bsrnn_stream_get_row(bsrnn_stream* st, int32_t row, float* blob_host)
{
    if (!st || !blob_host) return fail(BSRNN_EARG, "bsrnn_stream_get_row: null argument");
    if (row < 0 || row >= st->C) return fail(BSRNN_EARG, "bsrnn_stream_get_row: row %d is outside [0, %d)", row, st->C);
    if (int rc = stream_move_row(st, row, blob_host, true)) return rc;
    return check_range(st->ctx);          // as bsrnn_stream_get_state: calls made under the 'deferred' policy report a range violation here
}

int bsrnn_stream_set_row(bsrnn_stream* st, int32_t row, const float* blob_host)
{
    if (!st || !blob_host) return fail(BSRNN_EARG, "bsrnn_stream_set_row: null argument");
    if (row < 0 || row >= st->C) return fail(BSRNN_EARG, "bsrnn_stream_set_row: row %d is outside [0, %d)", row, st->C);
    return stream_move_row(st, row, const_cast<float*>(blob_host), false);
}

}  // extern "C"
