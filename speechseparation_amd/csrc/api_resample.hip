// C ABI of libbsrnn_hip.so, sample-rate conversion and FIR (bsrnn_resample*, bsrnn_resampler_*, bsrnn_resampler_bank_*,
// bsrnn_fir_bank_*, bsrnn_convolve_ragged, bsrnn_remix_ragged, bsrnn_fir_stream_*).  Each object owns its handle type and reaches the context through api_internal.h.
#include "api_internal.h"

int bsrnn::host::resample_check_rates(int32_t rate_in, int32_t rate_out, const char* who, ResampleRatio& q)
{
    q = resample_ratio(rate_in, rate_out);
    if (q.why == RESAMPLE_BAD_RATE)
        return fail(BSRNN_EARG, "%s: rates must be at least 1, got rate_in = %d, rate_out = %d", who, rate_in, rate_out);
    if (q.why == RESAMPLE_TOO_FINE)
        return fail(BSRNN_EARG, "%s: %d -> %d reduces to %lld / %lld, beyond the limit of %d for max(up, down)", who, rate_in, rate_out,
                    (long long)q.up, (long long)q.down, RESAMPLE_MAX_FACTOR);
    return 0;
}

extern "C" {

// --------------------------------------------------------------------------- sample-rate conversion
// The definition and all index arithmetic: resample_host.h; the kernel: resample.hip.  One launch per call, for the one-shot form and
// for the streaming object alike.
struct bsrnn_resampler {
    bsrnn_ctx* ctx;
    int C;
    ResampleRatio q;
    ResampleTiling g;
    const float* tab;              // the context's table of (up, down)
    // The inputs that outputs not yet determined still need, per row: two buffers of cap floats per row, a call reads set `cur` and
    // writes the other (the launch that reads the carry also writes the next one).  N inputs taken and J outputs given so far; the
    // carry holds inputs [max(0, resample_base(J)), N).
    float* carry[2];
    int64_t cap;
    int cur;
    int64_t N, J;
};

// The context's table of q's (up, down): designed in double, rounded to fp32 and uploaded when the pair is met first (synchronous).
static int resample_table_of(bsrnn_ctx* c, const ResampleRatio& q, const bsrnn_ctx::ResampleTable** out)
{
    for (const auto& t : c->rs_tables)
        if (t.q.up == q.up && t.q.down == q.down) { *out = &t; return 0; }
    bsrnn_ctx::ResampleTable t{q, resample_tiling(q), nullptr};
    const std::vector<float> tab = resample_table_by_output(q, resample_design(q), t.g.ld);
    ++g_dbg[DBG_ALLOC];
    HIP_TRY(hipMalloc((void**)&t.d, tab.size() * sizeof(float)));
    if (hipError_t e = hipMemcpy(t.d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice)) {
        (void)hipFree(t.d);
        return fail(BSRNN_EHIP, "resampling table upload: %s", hipGetErrorString(e));
    }
    c->rs_tables.push_back(t);
    *out = &c->rs_tables.back();
    return 0;
}

static ResampleArgs resample_args(const ResampleRatio& q, const ResampleTiling& g, const float* tab)
{
    ResampleArgs a{};
    a.tab = tab; a.up = (int)q.up; a.down = (int)q.down; a.Kh = q.Kh; a.ld = g.ld; a.chunk = g.chunk; a.tile = g.tile;
    return a;
}

int64_t bsrnn_resample_len(int64_t n_in, int32_t rate_in, int32_t rate_out)
{
    const ResampleRatio q = resample_ratio(rate_in, rate_out);
    if (q.why != RESAMPLE_OK || n_in < 1 || n_in > (INT64_MAX >> 12)) return -1;
    return resample_n_out(n_in, q.up, q.down);
}

int bsrnn_resample(bsrnn_ctx* c, const float* in, int64_t in_stride, float* out, int64_t out_stride, int32_t R, int64_t n_in,
                   int32_t rate_in, int32_t rate_out, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!in || !out || R < 1) return fail(BSRNN_EARG, "bsrnn_resample: need an input, an output and R >= 1, got R = %d", R);
    ResampleRatio q;
    if (int rc = resample_check_rates(rate_in, rate_out, "bsrnn_resample", q)) return rc;
    if (n_in < 1 || n_in > (INT64_MAX >> 12)) return fail(BSRNN_EARG, "bsrnn_resample: need n_in >= 1 samples, got %lld", (long long)n_in);
    const int64_t n_out = resample_n_out(n_in, q.up, q.down);
    if (in_stride < n_in) return fail(BSRNN_EARG, "bsrnn_resample: in_stride %lld is less than n_in = %lld", (long long)in_stride, (long long)n_in);
    if (out_stride < n_out)
        return fail(BSRNN_EARG, "bsrnn_resample: out_stride %lld is less than the %lld samples of a row's result", (long long)out_stride, (long long)n_out);
    // the extent of what the rows span, not R * in_stride: behind the last row of a column view (buf[:, a:b]) lies somebody else's memory
    if (ranges_overlap(in, ((size_t)(R - 1) * in_stride + n_in) * sizeof(float), out, ((size_t)(R - 1) * out_stride + n_out) * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_resample: out_dev must not overlap the (R - 1) * in_stride + n_in floats the rows of in_dev span "
                                "(rows are read while others are written)");
    if (int rc = check_device(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if (q.up == q.down) {           // equal rates: a copy
        HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * sizeof(float), in, (size_t)in_stride * sizeof(float), (size_t)n_in * sizeof(float), R,
                                 hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const bsrnn_ctx::ResampleTable* t = nullptr;
    if (int rc = resample_table_of(c, q, &t)) return rc;
    ResampleArgs a = resample_args(t->q, t->g, t->d);
    a.b = in; a.b_stride = in_stride; a.n_total = n_in;
    a.out = out; a.out_stride = out_stride; a.n_j = n_out;
    a.n_tiles = (int)((n_out + t->g.tile - 1) / t->g.tile);
    launch_resample(a, R, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int64_t resampler_keep_from(const bsrnn_resampler* rs, int64_t J)
{
    const int64_t b = resample_base(J, rs->q.up, rs->q.down, rs->q.Kh);
    return b > 0 ? b : 0;
}

int bsrnn_resampler_create(bsrnn_ctx* c, int32_t C, int32_t rate_in, int32_t rate_out, bsrnn_resampler** out)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!out || C < 1) return fail(BSRNN_EARG, "bsrnn_resampler_create: need C >= 1 rows and a place for the object, got C = %d", C);
    ResampleRatio q;
    if (int rc = resample_check_rates(rate_in, rate_out, "bsrnn_resampler_create", q)) return rc;
    if (int rc = check_device(c)) return rc;
    CallGuard guard_(c);
    if (!guard_.ok) return guard_.refuse();
    const bsrnn_ctx::ResampleTable* t = nullptr;
    if (int rc = resample_table_of(c, q, &t)) return rc;
    bsrnn_resampler* rs = new bsrnn_resampler();
    rs->ctx = c; rs->C = C; rs->q = t->q; rs->g = t->g; rs->tab = t->d;
    rs->cap = resample_carry_floats(q);
    rs->cur = 0; rs->N = rs->J = 0;
    float* p = nullptr;
    ++g_dbg[DBG_ALLOC];
    const size_t bytes = 2 * (size_t)C * rs->cap * sizeof(float);
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess && (e = hipMemset(p, 0, bytes)) != hipSuccess) (void)hipFree(p);
    if (e != hipSuccess) { delete rs; return fail(BSRNN_EHIP, "bsrnn_resampler_create: %s", hipGetErrorString(e)); }
    rs->carry[0] = p; rs->carry[1] = p + (size_t)C * rs->cap;
    // the kernel's first launch (code object loading) happens here, not in the first bsrnn_resampler_process: an empty carry hand-over
    ResampleArgs a = resample_args(rs->q, rs->g, rs->tab);
    a.a = rs->carry[0]; a.a_stride = rs->cap; a.carry = rs->carry[1]; a.carry_stride = rs->cap;
    launch_resample(a, C, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { (void)hipFree(p); delete rs; return fail(BSRNN_EHIP, "bsrnn_resampler_create: %s", hipGetErrorString(e)); }
    ++c->live_streams;
    *out = rs;
    return 0;
}

void bsrnn_resampler_destroy(bsrnn_resampler* rs)
{
    if (!rs) return;
    bsrnn_ctx* c = rs->ctx;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(rs->carry[0]);
    delete rs;
    if (--c->live_streams == 0 && c->zombie) destroy_now(c);     // as bsrnn_stream_destroy: the context goes with the last object that points at it
}

int bsrnn_resampler_reset(bsrnn_resampler* rs, void* stream)
{
    if (!rs) return fail(BSRNN_EARG, "null resampler");
    (void)stream;          // nothing to enqueue: with no input taken the carry holds no sample a call would read
    rs->N = rs->J = 0;
    return 0;
}

int64_t bsrnn_resampler_ready(const bsrnn_resampler* rs, int64_t n_in)
{
    if (!rs || n_in < 0 || n_in > (INT64_MAX >> 12) - rs->N) return -1;
    return resample_ready(rs->N + n_in, rs->q.up, rs->q.down, rs->q.half) - rs->J;
}

// process (flush == false): the block joins the carry and the outputs it determines are written; flush: what is left up to the final
// length, the future taken as zeros.
static int resampler_run(bsrnn_resampler* rs, const float* in, int64_t in_stride, int64_t n_in, float* out, int64_t out_stride,
                         int64_t* n_out_host, bool flush, hipStream_t s)
{
    const char* who = flush ? "bsrnn_resampler_flush" : "bsrnn_resampler_process";
    if (!rs) return fail(BSRNN_EARG, "null resampler");
    if (!n_out_host) return fail(BSRNN_EARG, "%s: nowhere to report the sample count", who);
    if (n_in < 0 || n_in > (INT64_MAX >> 12) - rs->N) return fail(BSRNN_EARG, "%s: need n_in >= 0 samples, got %lld", who, (long long)n_in);
    if (n_in > 0 && (!in || in_stride < n_in))
        return fail(BSRNN_EARG, "%s: need an input block with in_stride >= n_in, got in_stride = %lld, n_in = %lld", who, (long long)in_stride, (long long)n_in);
    const ResampleRatio& q = rs->q;
    const int64_t N1 = rs->N + n_in;
    const int64_t J1 = flush ? resample_n_out(N1, q.up, q.down) : resample_ready(N1, q.up, q.down, q.half);
    const int64_t count = J1 - rs->J;
    if (count > 0 && (!out || out_stride < count))
        return fail(BSRNN_EARG, "%s: need an output block with out_stride >= the %lld samples this call writes per row, got out_stride = %lld", who,
                    (long long)count, (long long)out_stride);
    if (n_in > 0 && count > 0 &&
        ranges_overlap(in, ((size_t)(rs->C - 1) * in_stride + n_in) * sizeof(float), out, ((size_t)(rs->C - 1) * out_stride + count) * sizeof(float)))
        return fail(BSRNN_EARG, "%s: out_dev must not overlap in_dev (rows are read while others are written)", who);
    bsrnn_ctx* c = rs->ctx;
    if (int rc = check_device(c)) return rc;
    ENTER_CALL(c, s);
    *n_out_host = count;
    if (flush) {
        if (count > 0) {
            ResampleArgs a = resample_args(q, rs->g, rs->tab);
            a.a = rs->carry[rs->cur]; a.a_stride = rs->cap; a.a0 = resampler_keep_from(rs, rs->J); a.a1 = rs->N; a.n_total = rs->N;
            a.out = out; a.out_stride = out_stride; a.j0 = rs->J; a.n_j = count;
            a.n_tiles = (int)((count + rs->g.tile - 1) / rs->g.tile);
            launch_resample(a, rs->C, s);
            HIP_TRY(hipGetLastError());
        }
        rs->N = rs->J = 0;
        return 0;
    }
    if (n_in == 0) return 0;
    ResampleArgs a = resample_args(q, rs->g, rs->tab);
    a.a = rs->carry[rs->cur]; a.a_stride = rs->cap; a.a0 = resampler_keep_from(rs, rs->J); a.a1 = rs->N;
    a.b = in; a.b_stride = in_stride; a.n_total = N1;
    a.out = out; a.out_stride = out_stride; a.j0 = rs->J; a.n_j = count;
    a.n_tiles = (int)((count + rs->g.tile - 1) / rs->g.tile);
    a.carry = rs->carry[rs->cur ^ 1]; a.carry_stride = rs->cap; a.c0 = resampler_keep_from(rs, J1);
    if (N1 - a.c0 > rs->cap) return fail(BSRNN_ESTATE, "%s: the carry would hold %lld samples of %lld (internal error)", who, (long long)(N1 - a.c0), (long long)rs->cap);
    launch_resample(a, rs->C, s);
    HIP_TRY(hipGetLastError());
    rs->N = N1; rs->J = J1; rs->cur ^= 1;
    return 0;
}

int bsrnn_resampler_process(bsrnn_resampler* rs, const float* in, int64_t in_stride, int64_t n_in, float* out, int64_t out_stride,
                            int64_t* n_out_host, void* stream)
{
    return resampler_run(rs, in, in_stride, n_in, out, out_stride, n_out_host, false, (hipStream_t)stream);
}

int bsrnn_resampler_flush(bsrnn_resampler* rs, float* out, int64_t out_stride, int64_t* n_out_host, void* stream)
{
    return resampler_run(rs, nullptr, 0, 0, out, out_stride, n_out_host, true, (hipStream_t)stream);
}

// --------------------------------------------------------------------------- long FIR convolution of ragged rows
// torch.nn.functional.conv1d(x, h, padding='same') with the whole filter as the kernel (m_dataset.py:92-114: a room impulse response of tens
// of thousands of taps), as a uniformly partitioned overlap-save convolution on the library's own transform.  The definition, the plan and
// the row groups: convolve_host.h; the kernels: fft.hip.  A bank holds the partition spectra of its filters, built once.
struct bsrnn_fir_bank {
    bsrnn_ctx* ctx;
    std::vector<int32_t> taps;       // taps per filter
    std::vector<size_t> off;         // where a filter's image starts in d_images (floats)
    float* d_images;                 // [sum of P][CONV_LD]; null on a host-only context (the bank then only answers count / taps and refusals)
    int streams = 0;                 // live bsrnn_fir_stream objects on this bank: they read d_images
    bool zombie = false;             // bsrnn_fir_bank_destroy was called while streams lived; the last of them frees the bank
};

int bsrnn_fir_bank_create(bsrnn_ctx* c, int32_t n_filters, const float* const* taps_host, const int32_t* n_taps_host, bsrnn_fir_bank** out)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!out || !taps_host || !n_taps_host || n_filters < 1)
        return fail(BSRNN_EARG, "bsrnn_fir_bank_create: need n_filters >= 1 filters (taps_host, n_taps_host) and a place for the object, got n_filters = %d", n_filters);
    size_t n_taps = 0, n_img = 0;
    for (int i = 0; i < n_filters; ++i) {
        if (!taps_host[i]) return fail(BSRNN_EARG, "bsrnn_fir_bank_create: taps_host[%d] is null", i);
        if (n_taps_host[i] < 1 || n_taps_host[i] > CONV_MAX_TAPS)
            return fail(BSRNN_EARG, "bsrnn_fir_bank_create: n_taps_host[%d] = %d is outside [1, %d]", i, n_taps_host[i], CONV_MAX_TAPS);
        n_taps += (size_t)n_taps_host[i];
        n_img += (size_t)conv_image_floats(n_taps_host[i]);
    }
    if (c->zombie) return fail(BSRNN_ESTATE, "context was destroyed");
    std::unique_ptr<bsrnn_fir_bank> bk(new bsrnn_fir_bank());
    bk->ctx = c; bk->d_images = nullptr;
    size_t at = 0;
    for (int i = 0; i < n_filters; ++i) { bk->taps.push_back(n_taps_host[i]); bk->off.push_back(at); at += (size_t)conv_image_floats(n_taps_host[i]); }
    if (c->device >= 0) {
        if (int rc = check_device(c)) return rc;
        CallGuard guard_(c);
        if (!guard_.ok) return guard_.refuse();
        // one allocation: the images, then the taps as the caller gave them (read by the launches below, not kept apart afterwards)
        float* p = nullptr;
        ++g_dbg[DBG_ALLOC];
        hipError_t e = hipMalloc((void**)&p, (n_img + n_taps) * sizeof(float));
        size_t t_at = n_img;
        for (int i = 0; e == hipSuccess && i < n_filters; ++i) {
            e = hipMemcpy(p + t_at, taps_host[i], (size_t)n_taps_host[i] * sizeof(float), hipMemcpyHostToDevice);
            if (e == hipSuccess) { launch_fir_taps(c->tb, p + t_at, n_taps_host[i], p + bk->off[i], nullptr); e = hipGetLastError(); }
            t_at += (size_t)n_taps_host[i];
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { if (p) (void)hipFree(p); return fail(BSRNN_EHIP, "bsrnn_fir_bank_create: %s", hipGetErrorString(e)); }
        bk->d_images = p;
    }
    ++c->live_streams;
    *out = bk.release();
    return 0;
}

void bsrnn_fir_bank_destroy(bsrnn_fir_bank* bk)
{
    if (!bk) return;
    if (bk->streams > 0) { bk->zombie = true; return; }                // a stream keeps its bank alive (bsrnn_fir_stream_destroy ends it)
    bsrnn_ctx* c = bk->ctx;
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(bk->d_images);
    }
    delete bk;
    if (--c->live_streams == 0 && c->zombie) destroy_now(c);     // as bsrnn_resampler_destroy
}

int32_t bsrnn_fir_bank_count(const bsrnn_fir_bank* bk) { return bk ? (int32_t)bk->taps.size() : -1; }
int32_t bsrnn_fir_bank_taps(const bsrnn_fir_bank* bk, int32_t filter)
{
    return (bk && filter >= 0 && filter < (int32_t)bk->taps.size()) ? bk->taps[filter] : -1;
}

int bsrnn_convolve_ragged(bsrnn_fir_bank* bk, const float* in, int64_t in_stride, const int64_t* lens_host, const int32_t* filter_host, float* out,
                          int64_t out_stride, int32_t R, void* stream)
{
    // arguments first, device or not (a bank of a host-only context answers them before BSRNN_ESTATE)
    if (!bk) return fail(BSRNN_EARG, "null FIR bank");
    if (!in || !lens_host || !filter_host || !out)
        return fail(BSRNN_EARG, "bsrnn_convolve_ragged: null argument (need in_dev, lens_host, filter_host and out_dev)");
    if (R < 1) return fail(BSRNN_EARG, "bsrnn_convolve_ragged: need R >= 1 rows, got R = %d", R);
    const int32_t count = (int32_t)bk->taps.size();
    size_t in_ext = 0, out_ext = 0;                                   // floats the rows span: behind the last row of a view lies somebody else's memory
    for (int r = 0; r < R; ++r) {
        const int64_t n = lens_host[r];
        if (n < 1 || n > CONV_MAX_LEN)
            return fail(BSRNN_EARG, "bsrnn_convolve_ragged: lens_host[%d] = %lld is outside [1, 2^40]", r, (long long)n);
        if (in_stride < n)
            return fail(BSRNN_EARG, "bsrnn_convolve_ragged: in_stride %lld is less than lens_host[%d] = %lld", (long long)in_stride, r, (long long)n);
        if (out_stride < n)
            return fail(BSRNN_EARG, "bsrnn_convolve_ragged: out_stride %lld is less than lens_host[%d] = %lld", (long long)out_stride, r, (long long)n);
        if (filter_host[r] < -1 || filter_host[r] >= count)
            return fail(BSRNN_EARG, "bsrnn_convolve_ragged: filter_host[%d] = %d is outside [-1, %d)", r, filter_host[r], count);
        in_ext = std::max(in_ext, (size_t)r * in_stride + (size_t)n);
        out_ext = std::max(out_ext, (size_t)r * out_stride + (size_t)n);
    }
    if (ranges_overlap(in, in_ext * sizeof(float), out, out_ext * sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_convolve_ragged: out_dev must not overlap the floats the rows of in_dev span (rows are read while others are written)");
    bsrnn_ctx* c = bk->ctx;
    if (int rc = check_device(c)) return rc;
    for (const void* ptr : {(const void*)in, (const void*)out}) {     // the images live on the bank's device
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (at.type == hipMemoryTypeDevice && at.device != c->device)
            return fail(BSRNN_EARG, "bsrnn_convolve_ragged: %s lies on device %d, the bank was created on a context of device %d",
                        ptr == (const void*)in ? "in_dev" : "out_dev", at.device, c->device);
    }
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    // the plan: what every row computes, the row groups, where a row's spectra lie in its group's buffers
    std::vector<ConvRow> rows(R);
    std::vector<int64_t> nx(R), nb(R);
    for (int r = 0; r < R; ++r) {
        ConvRow& q = rows[r];
        q = ConvRow{};
        q.n = lens_host[r];
        if (filter_host[r] < 0) { q.nb = (int)conv_copy_blocks(q.n); nx[r] = nb[r] = 0; continue; }
        const int k = bk->taps[filter_host[r]];
        const ConvPlan pl = conv_plan(q.n, k);
        q.H = bk->d_images + bk->off[filter_host[r]];
        q.shift = pl.shift; q.P = pl.P; q.u0 = (int)pl.u0; q.nb = (int)pl.nb; q.f0 = (int)pl.f0; q.nx = (int)pl.nx;
        nx[r] = pl.nx; nb[r] = pl.nb;
    }
    const std::vector<ConvGroup> groups = conv_groups(nx.data(), nb.data(), R);
    int64_t need = 0;
    for (const ConvGroup& g : groups) {
        need = std::max(need, std::max(g.x_frames, g.y_frames));
        int64_t xo = 0, yo = 0;
        for (int r = g.first; r < g.first + g.rows; ++r) { rows[r].xoff = xo; rows[r].yoff = yo; xo += nx[r]; yo += nb[r]; }
    }
    bsrnn_ctx::Conv& cv = c->cv;
    if (need > cv.frames) {
        HIP_TRY(hipDeviceSynchronize());                              // queued kernels use the old buffers
        if (cv.X) (void)hipFree(cv.X);
        if (cv.Y) (void)hipFree(cv.Y);
        cv.X = cv.Y = nullptr; cv.frames = 0;
        const int64_t want = need >= CONV_FRAME_BUDGET ? need : std::min<int64_t>(CONV_FRAME_BUDGET, need + need / 4 + 16);
        g_dbg[DBG_ALLOC] += 2;
        HIP_TRY(hipMalloc((void**)&cv.X, (size_t)want * CONV_LD * sizeof(float)));
        const hipError_t e = hipMalloc((void**)&cv.Y, (size_t)want * CONV_LD * sizeof(float));
        if (e != hipSuccess) { (void)hipFree(cv.X); cv.X = nullptr; return fail(BSRNN_EHIP, "hipMalloc: %s", hipGetErrorString(e)); }
        cv.frames = want;
    }
    const size_t bytes = (size_t)R * sizeof(ConvRow);
    if (int rc = c->rg.upload(bytes, s, [&](char* h) { memcpy(h, rows.data(), bytes); })) return rc;
    const ConvRow* d_rows = reinterpret_cast<const ConvRow*>(c->rg.d);
    for (const ConvGroup& g : groups) {
        int max_nx = 0, max_nb = 0;
        for (int r = g.first; r < g.first + g.rows; ++r) { max_nx = std::max(max_nx, rows[r].nx); max_nb = std::max(max_nb, rows[r].nb); }
        launch_fir_group(c->tb, d_rows, g.first, g.rows, max_nx, max_nb, in, in_stride, out, out_stride, cv.X, cv.Y, s);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// --------------------------------------------------------------------------- the re-mix of an optimizer step
// MixDataSet's arithmetic (m_dataset.py:158-178) for all rows of a step in one launch.  The definition, the checks, the tile count and
// the traffic model: remix_host.h; the kernel: remix.hip.  The two tables travel as one block [R rows | n_terms terms] in the ragged
// calls' ring.
static_assert(sizeof(bsrnn_remix_term) == sizeof(RemixTerm) && offsetof(bsrnn_remix_term, src) == offsetof(RemixTerm, src) &&
              offsetof(bsrnn_remix_term, len) == offsetof(RemixTerm, len) && offsetof(bsrnn_remix_term, at) == offsetof(RemixTerm, at) &&
              offsetof(bsrnn_remix_term, gain) == offsetof(RemixTerm, gain), "remix_host.h and bsrnn_hip.h disagree");
static_assert(sizeof(bsrnn_remix_row) == sizeof(RemixRow) && offsetof(bsrnn_remix_row, n) == offsetof(RemixRow, n) &&
              offsetof(bsrnn_remix_row, first_term) == offsetof(RemixRow, first_term) && offsetof(bsrnn_remix_row, n_terms) == offsetof(RemixRow, n_terms),
              "remix_host.h and bsrnn_hip.h disagree");
static_assert(REMIX_TILE == BSRNN_REMIX_TILE, "remix_host.h and bsrnn_hip.h disagree");
static_assert(sizeof(RemixRow) % alignof(RemixTerm) == 0, "the terms follow the rows in one block");

int bsrnn_remix_ragged(bsrnn_ctx* c, const bsrnn_remix_row* rows_host, int32_t R, const bsrnn_remix_term* terms_host, int32_t n_terms,
                       float* mix, int64_t mix_stride, float* target, int64_t target_stride, int64_t width, void* stream)
{
    // arguments first, device or not (a host-only context answers them before BSRNN_ESTATE)
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!mix || !target) return fail(BSRNN_EARG, "bsrnn_remix_ragged: null argument (need mix_dev and target_dev)");
    const RemixRow* rows = reinterpret_cast<const RemixRow*>(rows_host);
    const RemixTerm* terms = reinterpret_cast<const RemixTerm*>(terms_host);
    const RemixVerdict v = remix_check(rows, R, terms, n_terms, mix_stride, target_stride, width);
    const int i = (int)v.index;
    switch (v.why) {
    case REMIX_OK: break;
    case REMIX_NULL_TABLE: return fail(BSRNN_EARG, "bsrnn_remix_ragged: null argument (need rows_host and terms_host)");
    case REMIX_BAD_COUNT: return fail(BSRNN_EARG, "bsrnn_remix_ragged: need R >= 1 rows and n_terms >= 1 terms, got R = %d, n_terms = %d", R, n_terms);
    case REMIX_BAD_WIDTH: return fail(BSRNN_EARG, "bsrnn_remix_ragged: width = %lld is outside [0, 2^40]", (long long)width);
    case REMIX_MIX_STRIDE:
        return fail(BSRNN_EARG, "bsrnn_remix_ragged: mix_stride %lld is less than width = %lld (or beyond 2^40, or R rows of it beyond 2^60)",
                    (long long)mix_stride, (long long)width);
    case REMIX_TARGET_STRIDE:
        return fail(BSRNN_EARG, "bsrnn_remix_ragged: target_stride %lld is less than width = %lld (or beyond 2^40, or R rows of it beyond 2^60)",
                    (long long)target_stride, (long long)width);
    case REMIX_ROW_LENGTH:
        return fail(BSRNN_EARG, "bsrnn_remix_ragged: rows_host[%d].n = %lld is outside [0, width = %lld]", i, (long long)rows[i].n, (long long)width);
    case REMIX_ROW_TERMS:
        return fail(BSRNN_EARG, "bsrnn_remix_ragged: rows_host[%d] owns terms [%d, %d + %d): need at least one, inside [0, %d)", i, rows[i].first_term,
                    rows[i].first_term, rows[i].n_terms, n_terms);
    case REMIX_TERM_LENGTH: return fail(BSRNN_EARG, "bsrnn_remix_ragged: terms_host[%d].len = %lld is outside [0, 2^40]", i, (long long)terms[i].len);
    case REMIX_TERM_OFFSET: return fail(BSRNN_EARG, "bsrnn_remix_ragged: terms_host[%d].at = %lld is outside [-2^40, 2^40]", i, (long long)terms[i].at);
    default: return fail(BSRNN_EARG, "bsrnn_remix_ragged: terms_host[%d].src is null with len = %lld", i, (long long)terms[i].len);
    }
    if (int rc = check_device(c)) return rc;                          // (no model stage: needs no committed weights)
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if (remix_tiles(width) < 1) return 0;                             // width = 0: nothing to write
    const size_t row_bytes = (size_t)R * sizeof(RemixRow), bytes = row_bytes + (size_t)n_terms * sizeof(RemixTerm);
    if (int rc = c->rg.upload(bytes, s, [&](char* h) { memcpy(h, rows, row_bytes); memcpy(h + row_bytes, terms, bytes - row_bytes); })) return rc;
    launch_remix_ragged(reinterpret_cast<const RemixRow*>(c->rg.d), reinterpret_cast<const RemixTerm*>(c->rg.d + row_bytes), R, mix, mix_stride,
                        target, target_stride, width, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// --------------------------------------------------------------------------- the streaming form of the FIR convolution
// C rows on one bank, each on a filter of it (or on -1: bypass) and at its own place in its own stream.  The definition and all index
// arithmetic: convolve_stream_host.h; the kernel: fft.hip (one launch per call).  On the device: the ring of the last P input spectra per
// row, the previous 1024 inputs and a FIFO of < 1024 samples per row.  On the host: filter and samples taken per row.
struct bsrnn_fir_stream {
    bsrnn_fir_bank* bank;
    int C, max_taps, align, Pmax;
    std::vector<int32_t> filter;     // -1: bypass
    std::vector<int64_t> N;          // samples the row has taken since the beginning of its stream
    std::vector<FirStreamRow> desc;  // the call being planned, and what its rows are at afterwards
    std::vector<int64_t> next_N, counts;
    std::vector<uint8_t> seen;
    float* d_ring;                  // one allocation: [C][Pmax][CONV_LD], then d_state [C][FIR_STREAM_ROW_FLOATS]; null on a host-only context
    float* d_state;
};

static int fir_stream_mark_rows(bsrnn_fir_stream* st, const int32_t* rows, int32_t n_rows, const char* who)
{
    if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(BSRNN_EARG, "%s: need a list of n_rows >= 0 rows, got n_rows = %d", who, n_rows);
    std::fill(st->seen.begin(), st->seen.end(), (uint8_t)0);
    for (int i = 0; i < n_rows; ++i) {
        const int32_t r = rows[i];
        if (r < 0 || r >= st->C) return fail(BSRNN_EARG, "%s: row %d (entry %d of the list) is outside [0, %d)", who, r, i, st->C);
        if (st->seen[r]) return fail(BSRNN_EARG, "%s: row %d is listed twice", who, r);
        st->seen[r] = 1;
    }
    return 0;
}

// the table of a call -> the device, and the one launch
static int fir_stream_launch(bsrnn_fir_stream* st, const float* in, int64_t in_stride, float* out, int64_t out_stride, hipStream_t s)
{
    bsrnn_ctx* c = st->bank->ctx;
    const size_t bytes = (size_t)st->C * sizeof(FirStreamRow);
    if (int rc = c->rg.upload(bytes, s, [&](char* h) { memcpy(h, st->desc.data(), bytes); })) return rc;
    launch_fir_stream(c->tb, reinterpret_cast<const FirStreamRow*>(c->rg.d), st->C, in, in_stride, out, out_stride, st->d_ring,
                      (int64_t)st->Pmax * CONV_LD, st->d_state, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_fir_stream_create(bsrnn_fir_bank* bk, int32_t C, int32_t max_taps, int32_t align, bsrnn_fir_stream** out)
{
    if (!bk) return fail(BSRNN_EARG, "null FIR bank");
    if (!out || C < 1) return fail(BSRNN_EARG, "bsrnn_fir_stream_create: need C >= 1 rows and a place for the object, got C = %d", C);
    if (max_taps < 1 || max_taps > CONV_MAX_TAPS)
        return fail(BSRNN_EARG, "bsrnn_fir_stream_create: max_taps = %d is outside [1, %d]", max_taps, CONV_MAX_TAPS);
    if (align != FIR_ALIGN_SAME && align != FIR_ALIGN_CAUSAL)
        return fail(BSRNN_EARG, "bsrnn_fir_stream_create: align = %d is neither BSRNN_FIR_SAME (0) nor BSRNN_FIR_CAUSAL (1)", align);
    bsrnn_ctx* c = bk->ctx;
    if (c->zombie) return fail(BSRNN_ESTATE, "context was destroyed");
    std::unique_ptr<bsrnn_fir_stream> st(new bsrnn_fir_stream());
    st->bank = bk; st->C = C; st->max_taps = max_taps; st->align = align; st->Pmax = conv_partitions(max_taps);
    st->filter.assign(C, -1);
    st->N.assign(C, 0);
    st->next_N.assign(C, 0);
    st->counts.assign(C, 0);
    st->desc.assign(C, fir_stream_row_held());
    st->seen.assign(C, 0);
    st->d_ring = st->d_state = nullptr;
    if (c->device >= 0) {
        if (int rc = check_device(c)) return rc;
        CallGuard guard_(c);
        if (!guard_.ok) return guard_.refuse();
        const size_t ring = (size_t)fir_stream_ring_floats(C, max_taps), bytes = (ring + (size_t)C * FIR_STREAM_ROW_FLOATS) * sizeof(float);
        float* p = nullptr;
        ++g_dbg[DBG_ALLOC];
        hipError_t e = hipMalloc((void**)&p, bytes);
        if (e == hipSuccess && (e = hipMemset(p, 0, bytes)) != hipSuccess) (void)hipFree(p);
        if (e != hipSuccess) return fail(BSRNN_EHIP, "bsrnn_fir_stream_create: %s", hipGetErrorString(e));
        st->d_ring = p; st->d_state = p + ring;
        // the table block of C rows and the kernel's first launch (code object loading) happen here: a call in which every row is held
        int rc = fir_stream_launch(st.get(), nullptr, 0, nullptr, 0, nullptr);
        if (!rc && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = fail(BSRNN_EHIP, "bsrnn_fir_stream_create: %s", hipGetErrorString(e));
        if (rc) { (void)hipFree(p); return rc; }
    }
    ++bk->streams;
    *out = st.release();
    return 0;
}

void bsrnn_fir_stream_destroy(bsrnn_fir_stream* st)
{
    if (!st) return;
    bsrnn_fir_bank* bk = st->bank;
    bsrnn_ctx* c = bk->ctx;
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(st->d_ring);
    }
    delete st;
    if (--bk->streams == 0 && bk->zombie) bsrnn_fir_bank_destroy(bk);      // the bank was destroyed before its last stream
}

int bsrnn_fir_stream_assign(bsrnn_fir_stream* st, const int32_t* rows, int32_t n_rows, int32_t filter)
{
    if (!st) return fail(BSRNN_EARG, "null FIR stream");
    const int32_t count = (int32_t)st->bank->taps.size();
    if (filter < -1 || filter >= count) return fail(BSRNN_EARG, "bsrnn_fir_stream_assign: filter %d is outside [-1, %d)", filter, count);
    if (filter >= 0 && st->bank->taps[filter] > st->max_taps)
        return fail(BSRNN_EARG, "bsrnn_fir_stream_assign: filter %d has %d taps, the stream was created for max_taps = %d", filter,
                    st->bank->taps[filter], st->max_taps);
    if (int rc = fir_stream_mark_rows(st, rows, n_rows, "bsrnn_fir_stream_assign")) return rc;
    // nothing to enqueue: a row at the beginning of a stream reads no ring slot, tail or FIFO sample that an earlier stream left
    for (int i = 0; i < n_rows; ++i) { st->filter[rows[i]] = filter; st->N[rows[i]] = 0; }
    return 0;
}

int bsrnn_fir_stream_reset_rows(bsrnn_fir_stream* st, const int32_t* rows, int32_t n_rows)
{
    if (!st) return fail(BSRNN_EARG, "null FIR stream");
    if (int rc = fir_stream_mark_rows(st, rows, n_rows, "bsrnn_fir_stream_reset_rows")) return rc;
    for (int i = 0; i < n_rows; ++i) st->N[rows[i]] = 0;
    return 0;
}

int32_t bsrnn_fir_stream_filter_of(const bsrnn_fir_stream* st, int32_t row) { return st && row >= 0 && row < st->C ? st->filter[row] : -2; }

int64_t bsrnn_fir_stream_ready(const bsrnn_fir_stream* st, int32_t row, int64_t n_in)
{
    if (!st || row < 0 || row >= st->C || n_in < 0 || n_in > FIR_STREAM_COUNT_MAX) return -1;
    const int32_t f = st->filter[row];
    return f < 0 ? n_in : fir_stream_ready(st->N[row], n_in, fir_stream_shift(st->bank->taps[f], st->align));
}

// process (every row takes n_in[r]) or flush (the rows marked in seen[]): the table and the next positions first, then every refusal,
// then the launch
static int fir_stream_run(bsrnn_fir_stream* st, const float* in, int64_t in_stride, const int64_t* n_in, float* out, int64_t out_stride,
                          int64_t* n_out_host, bool flush, hipStream_t s)
{
    const char* who = flush ? "bsrnn_fir_stream_flush_rows" : "bsrnn_fir_stream_process";
    if (!n_out_host) return fail(BSRNN_EARG, "%s: nowhere to report the sample counts", who);
    if (!flush && !n_in) return fail(BSRNN_EARG, "%s: need the rows' sample counts", who);
    const bsrnn_fir_bank* bk = st->bank;
    int64_t max_in = 0, max_out = 0;
    bool work = false;
    for (int r = 0; r < st->C; ++r) {
        const int64_t n = flush ? 0 : n_in[r];
        if (n < 0 || n > FIR_STREAM_COUNT_MAX)
            return fail(BSRNN_EARG, "%s: n_in_host[%d] = %lld is outside [0, 2^30]", who, r, (long long)n);
        const int32_t f = st->filter[r];
        const int k = f >= 0 ? bk->taps[f] : 0;
        const float* H = f >= 0 && bk->d_images ? bk->d_images + bk->off[f] : nullptr;
        FirStreamRow& q = st->desc[r];
        q = fir_stream_row_held();
        st->next_N[r] = st->N[r];
        int64_t count = 0;
        if (flush) {
            if (st->seen[r]) {
                st->next_N[r] = 0;
                if (f >= 0) { q = fir_stream_row_flush(H, k, st->align, st->N[r]); count = st->N[r] - fir_stream_emitted(st->N[r], fir_stream_shift(k, st->align)); }
            }
        } else if (n > 0) {
            st->next_N[r] = st->N[r] + n;
            if (f < 0) { q.n_in = (int32_t)n; count = n; }
            else { q = fir_stream_row_process(H, k, st->align, st->N[r], n); count = fir_stream_ready(st->N[r], n, q.shift); }
        }
        work = work || q.n_in > 0 || q.ue > q.ub;
        st->counts[r] = count;
        max_in = std::max(max_in, n);
        max_out = std::max(max_out, count);
    }
    if (max_in > 0 && (!in || in_stride < max_in))
        return fail(BSRNN_EARG, "%s: need an input block with in_stride >= the largest count, got in_stride = %lld, largest n_in = %lld", who,
                    (long long)in_stride, (long long)max_in);
    if (max_out > 0 && (!out || out_stride < max_out))
        return fail(BSRNN_EARG, "%s: need an output block with out_stride >= the %lld samples this call writes to a row, got out_stride = %lld", who,
                    (long long)max_out, (long long)out_stride);
    if (max_in > 0 && max_out > 0 &&
        ranges_overlap(in, ((size_t)(st->C - 1) * in_stride + max_in) * sizeof(float), out, ((size_t)(st->C - 1) * out_stride + max_out) * sizeof(float)))
        return fail(BSRNN_EARG, "%s: out_dev must not overlap the span of in_dev (rows are read while others are written)", who);
    bsrnn_ctx* c = bk->ctx;
    if (int rc = check_device(c)) return rc;
    for (const void* ptr : {(const void*)(max_in > 0 ? in : nullptr), (const void*)(max_out > 0 ? out : nullptr)}) {      // the images live on the bank's device
        hipPointerAttribute_t at;
        if (!ptr) continue;
        if (hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (at.type == hipMemoryTypeDevice && at.device != c->device)
            return fail(BSRNN_EARG, "%s: %s lies on device %d, the bank was created on a context of device %d", who,
                        ptr == (const void*)in ? "in_dev" : "out_dev", at.device, c->device);
    }
    ENTER_CALL(c, s);
    if (work)
        if (int rc = fir_stream_launch(st, max_in > 0 ? in : nullptr, in_stride, max_out > 0 ? out : nullptr, out_stride, s)) return rc;
    for (int r = 0; r < st->C; ++r) n_out_host[r] = st->counts[r];
    st->N.swap(st->next_N);
    return 0;
}

int bsrnn_fir_stream_process(bsrnn_fir_stream* st, const float* in, int64_t in_stride, const int64_t* n_in_host, float* out, int64_t out_stride,
                             int64_t* n_out_host, void* stream)
{
    if (!st) return fail(BSRNN_EARG, "null FIR stream");
    return fir_stream_run(st, in, in_stride, n_in_host, out, out_stride, n_out_host, false, (hipStream_t)stream);
}

int bsrnn_fir_stream_flush_rows(bsrnn_fir_stream* st, const int32_t* rows, int32_t n_rows, float* out, int64_t out_stride, int64_t* n_out_host,
                                void* stream)
{
    if (!st) return fail(BSRNN_EARG, "null FIR stream");
    if (int rc = fir_stream_mark_rows(st, rows, n_rows, "bsrnn_fir_stream_flush_rows")) return rc;
    return fir_stream_run(st, nullptr, 0, nullptr, out, out_stride, n_out_host, true, (hipStream_t)stream);
}

// rows_host [n_rows] -> seen[] marks them; refuses a null list, a row outside [0, C) and a row listed twice
static int bank_mark_rows(bsrnn_resampler_bank* bk, const int32_t* rows, int32_t n_rows, const char* who)
{
    if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(BSRNN_EARG, "%s: need a list of n_rows >= 0 rows, got n_rows = %d", who, n_rows);
    std::fill(bk->seen.begin(), bk->seen.end(), (uint8_t)0);
    for (int i = 0; i < n_rows; ++i) {
        const int32_t r = rows[i];
        if (r < 0 || r >= bk->C) return fail(BSRNN_EARG, "%s: row %d (entry %d of the list) is outside [0, %d)", who, r, i, bk->C);
        if (bk->seen[r]) return fail(BSRNN_EARG, "%s: row %d is listed twice", who, r);
        bk->seen[r] = 1;
    }
    return 0;
}

int bsrnn_resampler_bank_create(bsrnn_ctx* c, int32_t C, const int32_t* rates_in, const int32_t* rates_out, int32_t n_pairs,
                                bsrnn_resampler_bank** out)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!out || C < 1) return fail(BSRNN_EARG, "bsrnn_resampler_bank_create: need C >= 1 rows and a place for the object, got C = %d", C);
    if (n_pairs < 1 || n_pairs > BANK_PAIRS_MAX)
        return fail(BSRNN_EARG, "bsrnn_resampler_bank_create: n_pairs = %d is outside [1, %d]", n_pairs, BANK_PAIRS_MAX);
    if (!rates_in || !rates_out) return fail(BSRNN_EARG, "bsrnn_resampler_bank_create: need the %d rate pairs", n_pairs);
    ResampleRatio q[BANK_PAIRS_MAX];
    for (int k = 0; k < n_pairs; ++k)
        if (int rc = resample_check_rates(rates_in[k], rates_out[k], "bsrnn_resampler_bank_create", q[k])) return rc;
    if (int rc = check_device(c)) return rc;
    CallGuard guard_(c);
    if (!guard_.ok) return guard_.refuse();
    std::unique_ptr<bsrnn_resampler_bank> bk(new bsrnn_resampler_bank());
    bk->ctx = c; bk->C = C; bk->n_pairs = n_pairs; bk->cap = 0;
    BankPair host[BANK_PAIRS_MAX];
    for (int k = 0; k < n_pairs; ++k) {
        const bsrnn_ctx::ResampleTable* t = nullptr;
        if (int rc = resample_table_of(c, q[k], &t)) return rc;
        bk->q[k] = t->q; bk->tile[k] = t->g.tile;
        host[k] = BankPair{t->d, (int)t->q.up, (int)t->q.down, t->q.Kh, t->g.ld, t->g.chunk, t->g.tile};
        bk->cap = std::max(bk->cap, resample_carry_floats(t->q));
    }
    bk->pos.assign(C, BankPos());
    bk->next.assign(C, BankPos());
    bk->desc.assign(C, BankRow{0, 0, 0, 0, 0});
    bk->seen.assign(C, 0);
    // one allocation: the pair table (512 bytes), then the two carry sets
    char* p = nullptr;
    ++g_dbg[DBG_ALLOC];
    const size_t head = BANK_PAIRS_MAX * sizeof(BankPair), bytes = head + 2 * (size_t)C * bk->cap * sizeof(float);
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess && (e = hipMemset(p, 0, bytes)) == hipSuccess) e = hipMemcpy(p, host, n_pairs * sizeof(BankPair), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        bk->pairs = (BankPair*)p; bk->carry = (float*)(p + head);
        // the kernel's first launch (code object loading) happens here: every row hands an empty carry over (a block of nothing)
        for (int r = 0; r < C; ++r) bk->desc[r] = BankRow{0, 0, 0, 0, BANK_ROW_RUNS | BANK_ROW_CARRIES};
        BankLaunch L{bk->pairs, nullptr, 0, nullptr, 0, bk->carry, bk->cap, (int64_t)C * bk->cap, 0};
        launch_resample_bank(L, bk->tile, bk->desc.data(), C, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) { (void)hipFree(p); return fail(BSRNN_EHIP, "bsrnn_resampler_bank_create: %s", hipGetErrorString(e)); }
    ++c->live_streams;
    *out = bk.release();
    return 0;
}

void bsrnn_resampler_bank_destroy(bsrnn_resampler_bank* bk)
{
    if (!bk) return;
    bsrnn_ctx* c = bk->ctx;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(bk->pairs);
    delete bk;
    if (--c->live_streams == 0 && c->zombie) destroy_now(c);     // as bsrnn_resampler_destroy
}

int bsrnn_resampler_bank_assign(bsrnn_resampler_bank* bk, const int32_t* rows, int32_t n_rows, int32_t pair)
{
    if (!bk) return fail(BSRNN_EARG, "null resampler bank");
    if (pair < 0 || pair >= bk->n_pairs) return fail(BSRNN_EARG, "bsrnn_resampler_bank_assign: pair %d is outside [0, %d)", pair, bk->n_pairs);
    if (int rc = bank_mark_rows(bk, rows, n_rows, "bsrnn_resampler_bank_assign")) return rc;
    // nothing to enqueue, as bsrnn_resampler_reset: with no input taken the carry holds no sample a call would read
    for (int i = 0; i < n_rows; ++i) bank_row_assign(bk->pos[rows[i]], pair);
    return 0;
}

int bsrnn_resampler_bank_reset_rows(bsrnn_resampler_bank* bk, const int32_t* rows, int32_t n_rows)
{
    if (!bk) return fail(BSRNN_EARG, "null resampler bank");
    if (int rc = bank_mark_rows(bk, rows, n_rows, "bsrnn_resampler_bank_reset_rows")) return rc;
    for (int i = 0; i < n_rows; ++i) bank_row_reset(bk->pos[rows[i]]);
    return 0;
}

int bsrnn_resampler_bank_pair_of(const bsrnn_resampler_bank* bk, int32_t row)
{
    return bk && row >= 0 && row < bk->C ? bk->pos[row].pair : -1;
}

int64_t bsrnn_resampler_bank_ready(const bsrnn_resampler_bank* bk, int32_t row, int64_t n_in)
{
    if (!bk || row < 0 || row >= bk->C) return -1;
    const BankPos& p = bk->pos[row];
    if (n_in < 0 || n_in > (INT64_MAX >> 12) - p.N) return -1;
    return bank_row_ready(bk->q[p.pair], p, n_in);
}

// process (rows == null: every row takes n_in[r]) or flush (the rows marked in seen[]): descriptors and next positions first, then
// every refusal, then the launches
static int bank_run(bsrnn_resampler_bank* bk, const float* in, int64_t in_stride, const int64_t* n_in, float* out, int64_t out_stride,
                    int64_t* n_out_host, bool flush, hipStream_t s)
{
    const char* who = flush ? "bsrnn_resampler_bank_flush_rows" : "bsrnn_resampler_bank_process";
    if (!n_out_host) return fail(BSRNN_EARG, "%s: nowhere to report the sample counts", who);
    if (!flush && !n_in) return fail(BSRNN_EARG, "%s: need the rows' sample counts", who);
    int64_t max_in = 0, max_out = 0;
    for (int r = 0; r < bk->C; ++r) {
        const BankPos& p = bk->pos[r];
        const ResampleRatio& q = bk->q[p.pair];
        const int64_t n = flush ? 0 : n_in[r];
        const int why = flush ? (bk->seen[r] ? bank_row_flush(q, p, bk->desc[r], bk->next[r]) : bank_row_process(q, p, 0, bk->desc[r], bk->next[r]))
                              : bank_row_process(q, p, n, bk->desc[r], bk->next[r]);
        if (why == BANK_BAD_COUNT) return fail(BSRNN_EARG, "%s: need n_in >= 0 samples for every row, got %lld for row %d", who, (long long)n, r);
        if (why == BANK_BLOCK_TOO_LONG)
            return fail(BSRNN_EARG, "%s: row %d would take %lld samples or give more than %lld; one call moves at most %lld per row", who, r,
                        (long long)n, (long long)BANK_BLOCK_MAX, (long long)BANK_BLOCK_MAX);
        if (why != BANK_OK) return fail(BSRNN_ESTATE, "%s: the carry of row %d would overflow (internal error)", who, r);
        max_in = std::max(max_in, n);
        max_out = std::max(max_out, (int64_t)bk->desc[r].n_j);
    }
    if (max_in > 0 && (!in || in_stride < max_in))
        return fail(BSRNN_EARG, "%s: need an input block with in_stride >= the largest count, got in_stride = %lld, largest n_in = %lld", who,
                    (long long)in_stride, (long long)max_in);
    if (max_out > 0 && (!out || out_stride < max_out))
        return fail(BSRNN_EARG, "%s: need an output block with out_stride >= the %lld samples this call writes to a row, got out_stride = %lld", who,
                    (long long)max_out, (long long)out_stride);
    if (max_in > 0 && max_out > 0 &&
        ranges_overlap(in, ((size_t)(bk->C - 1) * in_stride + max_in) * sizeof(float), out, ((size_t)(bk->C - 1) * out_stride + max_out) * sizeof(float)))
        return fail(BSRNN_EARG, "%s: out_dev must not overlap the span of in_dev (rows are read while others are written)", who);
    bsrnn_ctx* c = bk->ctx;
    if (int rc = check_device(c)) return rc;
    ENTER_CALL(c, s);
    for (int r = 0; r < bk->C; ++r) n_out_host[r] = bk->desc[r].n_j;
    BankLaunch L{bk->pairs, max_in > 0 ? in : nullptr, in_stride, out, out_stride, bk->carry, bk->cap, (int64_t)bk->C * bk->cap, 0};
    launch_resample_bank(L, bk->tile, bk->desc.data(), bk->C, s);
    HIP_TRY(hipGetLastError());
    bk->pos.swap(bk->next);
    return 0;
}

int bsrnn_resampler_bank_process(bsrnn_resampler_bank* bk, const float* in, int64_t in_stride, const int64_t* n_in_host, float* out,
                                 int64_t out_stride, int64_t* n_out_host, void* stream)
{
    if (!bk) return fail(BSRNN_EARG, "null resampler bank");
    return bank_run(bk, in, in_stride, n_in_host, out, out_stride, n_out_host, false, (hipStream_t)stream);
}

int bsrnn_resampler_bank_flush_rows(bsrnn_resampler_bank* bk, const int32_t* rows, int32_t n_rows, float* out, int64_t out_stride,
                                    int64_t* n_out_host, void* stream)
{
    if (!bk) return fail(BSRNN_EARG, "null resampler bank");
    if (int rc = bank_mark_rows(bk, rows, n_rows, "bsrnn_resampler_bank_flush_rows")) return rc;
    return bank_run(bk, nullptr, 0, nullptr, out, out_stride, n_out_host, true, (hipStream_t)stream);
}

}  // extern "C"
