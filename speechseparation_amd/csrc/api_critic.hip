// C ABI of libbsrnn_hip.so, the critic's layers (bsrnn_critic_conv_*): Conv1d(kernel 16, stride 3) forward and backward for the
// reference's Discriminator (bsrnn.py:512-536).  The definition and every size: critic_host.h; the kernels: critic.hip.  The scratch is
// the training entry points' grow-only buffer of the context.
// And the critic's input (bsrnn_critic_spectrum): the 4096-point analysis of the reference's train-discriminator.py:62-68.  The definition,
// the slab rule and every size: critic_spectrum_host.h; the kernels: stft4096.hip.
// And the committed critic (bsrnn_critic_create / _commit / _score): the whole module frozen into an object, its first layer on the fp16x2
// matrix path under the context's range policy, the exact layers above as its re-run.  The image, the plan and every size:
// critic_score_host.h; the kernels: critic_score.hip.
// And its gradient (bsrnn_critic_enable_grad / _score_grad / _layer1_dx): the score and d score / d x in one call, the first layer's dx on
// the fp16x2 matrix path from a second image, layers 4 .. 2 on the exact dx kernel with no dW beside it.  The image, the tiles and the
// workspace: critic_grad_host.h; the kernels: critic_grad.hip.
// And both on a padded batch (bsrnn_critic_score_ragged / _score_grad_ragged / _layer1_dx_ragged): one score per clip of a rectangle of rows
// of different lengths, the padding frames of the first layer skipped.  The tables, the live tiles and the workspace: critic_ragged_host.h.
#include "api_internal.h"

#include <cmath>

// sizes first, device or not (a host-only context answers them before BSRNN_ESTATE)
static int critic_sizes_ok(int32_t C, int32_t I, int32_t T, int32_t O, const char* who)
{
    switch (critic_check(C, I, T, O)) {
    case CRITIC_OK: return 0;
    case CRITIC_BAD_SIZE: return fail(BSRNN_EARG, "%s: need C, I, O >= 1, got C = %d, I = %d, O = %d", who, C, I, O);
    case CRITIC_TOO_SHORT: return fail(BSRNN_EARG, "%s: T = %d frames is less than the kernel's %d taps: no output frame", who, T, CRITIC_TAPS);
    default:
        return fail(BSRNN_EARG, "%s: C = %d, I = %d, T = %d, O = %d: a tensor of the call (x, W, y or the partial sums) would pass 2^31 - 1 elements",
                    who, C, I, T, O);
    }
}

static int score_sizes_ok(int32_t I, int32_t C, int32_t T, int32_t x_order, const char* who)
{
    switch (csc_check(I, C, T, x_order)) {
    case CSC_OK: return 0;
    case CSC_BAD_CHANNELS: return fail(BSRNN_EARG, "%s: need in_channels >= 1, got %d", who, I);
    case CSC_BAD_ROWS: return fail(BSRNN_EARG, "%s: need C >= 1 rows, got C = %d", who, C);
    case CSC_TOO_SHORT: return fail(BSRNN_EARG, "%s: T = %d frames, the four layers need at least %d", who, T, CRITIC_MIN_T);
    case CSC_BAD_ORDER: return fail(BSRNN_EARG, "%s: x_order = %d is neither 0 (planar) nor 1 (interleaved)", who, x_order);
    case CSC_ODD_INTERLEAVED: return fail(BSRNN_EARG, "%s: an interleaved input has an even number of channels, in_channels = %d is odd", who, I);
    default:
        return fail(BSRNN_EARG, "%s: in_channels = %d, C = %d, T = %d: x, a layer's output or the workspace would pass 2^31 - 1 elements", who, I, C, T);
    }
}

// The fp32 snapshot of a committed critic: [w0 | b0 | w1 | b1 | w2 | b2 | w3 | b3 | lin_w | lin_b], every block 16-byte aligned
struct CriticParams {
    int64_t off[2 * CRITIC_LAYERS + 2], n[2 * CRITIC_LAYERS + 2], total = 0;
    explicit CriticParams(int I)
    {
        int in = I;
        for (int l = 0; l < CRITIC_LAYERS; ++l) {
            n[2 * l] = (int64_t)CRITIC_WIDTHS[l] * in * CRITIC_TAPS;
            n[2 * l + 1] = CRITIC_WIDTHS[l];
            in = CRITIC_WIDTHS[l];
        }
        n[2 * CRITIC_LAYERS] = CRITIC_WIDTHS[CRITIC_LAYERS - 1];
        n[2 * CRITIC_LAYERS + 1] = 1;
        for (int j = 0; j < 2 * CRITIC_LAYERS + 2; ++j) { off[j] = total; total += csc_round4(n[j]); }
    }
};

// A frozen critic: its own fp32 copy of every parameter (the exact chain reads it) and the first layer's fp16x2 image (critic_score_host.h)
struct bsrnn_critic {
    bsrnn_ctx* ctx = nullptr;
    int I = 0;
    bool committed = false, usable = false;      // usable: max |W| of the first layer <= 65504, the image holds finite pieces
    float wmax = 0.f;
    float* d_par = nullptr;
    void* d_img = nullptr;
    unsigned* d_max = nullptr;
    void* d_img_dx = nullptr;                    // the first layer's image in the dx product's order: bsrnn_critic_enable_grad allocates it
};

static int grad_sizes_ok(int32_t I, int32_t C, int32_t T, int32_t x_order, const char* who)
{
    switch (cgd_check(I, C, T, x_order)) {
    case CGD_OK: return 0;
    case CGD_BAD_CHANNELS: return fail(BSRNN_EARG, "%s: need in_channels >= 1, got %d", who, I);
    case CGD_BAD_ROWS: return fail(BSRNN_EARG, "%s: need C >= 1 rows, got C = %d", who, C);
    case CGD_TOO_SHORT: return fail(BSRNN_EARG, "%s: T = %d frames, the four layers need at least %d", who, T, CRITIC_MIN_T);
    case CGD_BAD_ORDER: return fail(BSRNN_EARG, "%s: x_order = %d is neither 0 (planar) nor 1 (interleaved)", who, x_order);
    case CGD_ODD_INTERLEAVED: return fail(BSRNN_EARG, "%s: an interleaved input has an even number of channels, in_channels = %d is odd", who, I);
    default:
        return fail(BSRNN_EARG, "%s: in_channels = %d, C = %d, T = %d: x, a layer's gradient, the image or the workspace would pass 2^31 - 1 elements",
                    who, I, C, T);
    }
}

// A ragged call's arguments (critic_ragged_host.h): frames and clip_rows are not null
static int ragged_args_ok(int32_t I, int32_t R, int32_t Tmax, const int32_t* frames, const int32_t* clip_rows, int32_t n_clips, int32_t x_order,
                          bool grad, const char* who)
{
    int bad = -1;
    switch (crg_check(I, R, Tmax, frames, clip_rows, n_clips, x_order, grad, &bad)) {
    case CRG_OK: return 0;
    case CRG_BAD_CHANNELS: return fail(BSRNN_EARG, "%s: need in_channels >= 1, got %d", who, I);
    case CRG_NO_CLIPS: return fail(BSRNN_EARG, "%s: need n_clips >= 1, got n_clips = %d", who, n_clips);
    case CRG_BAD_CLIP_ROWS: return fail(BSRNN_EARG, "%s: clip %d has %d rows, need at least 1", who, bad, clip_rows[bad]);
    case CRG_CLIP_TOO_SHORT:
        return fail(BSRNN_EARG, "%s: clip %d has %d frames, the four layers need at least %d", who, bad, frames[bad], CRITIC_MIN_T);
    case CRG_CLIP_TOO_LONG: return fail(BSRNN_EARG, "%s: clip %d has %d frames, more than Tmax = %d", who, bad, frames[bad], Tmax);
    case CRG_ROWS_MISMATCH: return fail(BSRNN_EARG, "%s: the clips' rows do not sum to R = %d", who, R);
    case CRG_BAD_ORDER: return fail(BSRNN_EARG, "%s: x_order = %d is neither 0 (planar) nor 1 (interleaved)", who, x_order);
    case CRG_ODD_INTERLEAVED: return fail(BSRNN_EARG, "%s: an interleaved input has an even number of channels, in_channels = %d is odd", who, I);
    default:
        return fail(BSRNN_EARG, "%s: in_channels = %d, R = %d, Tmax = %d, n_clips = %d: x, a layer's gradient, an image or the workspace would pass "
                    "2^31 - 1 elements", who, I, R, Tmax, n_clips);
    }
}

// The first layer's dx from dp1 [C][1024][T1] at ws + g.off_dp[0], whose maximum stands in the max word: fp16x2 from the image, or the
// exact kernel (through the planar dx and the scatter when dx is interleaved)
static void first_layer_dx(const bsrnn_critic* k, const CriticParams& q, const CgdPlan& g, const float* dp1, float* ws, float* dx, int x_order,
                           bool exact, hipStream_t s)
{
    const int C = g.f.C, T = g.f.T;
    if (!exact) {
        launch_critic_dx_h2(dp1, k->d_img_dx, dx, (const unsigned*)(ws + g.off_max), k->ctx->d_range, g, x_order, s);
    } else if (x_order == CSC_ORDER_INTERLEAVED) {
        launch_critic_dx(k->d_par + q.off[0], dp1, ws + g.off_dxp, C, k->I, T, CSC_O, s);
        launch_critic_scatter(ws + g.off_dxp, dx, C, k->I, T, s);
    } else {
        launch_critic_dx(k->d_par + q.off[0], dp1, dx, C, k->I, T, CSC_O, s);
    }
}

static int spectrum_args_ok(int64_t R, int64_t n, int64_t stride, float scale, const char* who)
{
    switch (cs_check(R, n, stride, scale)) {
    case CS_OK: return 0;
    case CS_BAD_ROWS: return fail(BSRNN_EARG, "%s: need R >= 1 rows, got R = %lld", who, (long long)R);
    case CS_TOO_SHORT:
        return fail(BSRNN_EARG, "%s: need n > %d samples (reflect padding of a %d-point frame), got n = %lld", who, CS_NFFT / 2, CS_NFFT, (long long)n);
    case CS_BAD_STRIDE: return fail(BSRNN_EARG, "%s: wave_stride %lld is shorter than a row of n = %lld samples", who, (long long)stride, (long long)n);
    case CS_BAD_SCALE: return fail(BSRNN_EARG, "%s: scale = %g is not finite", who, (double)scale);
    default:
        return fail(BSRNN_EARG, "%s: R = %lld, n = %lld: x [R][%d][%lld] would pass 2^31 - 1 elements", who, (long long)R, (long long)n, CS_CHANNELS,
                    (long long)cs_frames(n));
    }
}

// Twiddles of the 2048-point passes, split twiddles of the 4096-point real transform and the window, evaluated in double and rounded once.
// Built by the first bsrnn_critic_spectrum of a context, not by bsrnn_create: a context that never forms the critic's input allocates
// what it always did.
static int ensure_spectrum_tables(bsrnn_ctx* c)
{
    if (c->d_cs_tables) return 0;
    const double PI = 3.14159265358979323846;
    const size_t o_tw = 0, o_split = 2 * 2048, o_hann = (o_split + 2 * CS_BINS + 3) & ~size_t(3), total = o_hann + CS_NFFT;
    std::vector<float> t(total, 0.f);
    for (int k = 0; k < 2048; ++k) { t[o_tw + 2 * k] = (float)cos(2 * PI * k / 2048); t[o_tw + 2 * k + 1] = (float)(-sin(2 * PI * k / 2048)); }
    for (int k = 0; k < CS_BINS; ++k) { t[o_split + 2 * k] = (float)cos(2 * PI * k / CS_NFFT); t[o_split + 2 * k + 1] = (float)(-sin(2 * PI * k / CS_NFFT)); }
    for (int i = 0; i < CS_NFFT; ++i) t[o_hann + i] = (float)(0.5 - 0.5 * cos(2 * PI * i / CS_NFFT));
    float* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, total * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d, t.data(), total * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (d) (void)hipFree(d);
        return fail(BSRNN_EHIP, "bsrnn_critic_spectrum: table upload: %s", hipGetErrorString(e));
    }
    ++g_dbg[DBG_ALLOC];
    c->d_cs_tables = d;
    c->cs.tw = (const float2*)(d + o_tw);
    c->cs.split = (const float2*)(d + o_split);
    c->cs.hann = d + o_hann;
    return 0;
}

extern "C" {

int bsrnn_critic_spectrum_layout(int32_t R, int64_t n, int64_t out[4])
{
    if (!out) return fail(BSRNN_EARG, "bsrnn_critic_spectrum_layout: nowhere to write the layout");
    if (int rc = spectrum_args_ok(R, n, n, 1.0f, "bsrnn_critic_spectrum_layout")) return rc;
    const CsPlan p = cs_plan(R, n);
    out[0] = p.T; out[1] = p.slabs; out[2] = p.frames_per_slab; out[3] = p.scratch_floats;
    return 0;
}

int bsrnn_critic_spectrum(bsrnn_ctx* c, const float* wave, int64_t wave_stride, float* x, int32_t R, int64_t n, float scale, void* stream)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!wave || !x) return fail(BSRNN_EARG, "bsrnn_critic_spectrum: null argument (need wave_dev and x_dev)");
    if (int rc = spectrum_args_ok(R, n, wave_stride, scale, "bsrnn_critic_spectrum")) return rc;
    if (int rc = check_device(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if (int rc = ensure_spectrum_tables(c)) return rc;
    const CsPlan p = cs_plan(R, n);
    float* ws = train_scratch(c, (size_t)p.scratch_floats);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_critic_spectrum: out of device memory (%zu MB of workspace)", (size_t)p.scratch_floats * sizeof(float) >> 20);
    // (slab after slab on one stream: a slab's transform overwrites the records the transpose in front of it has read)
    for (int i = 0; i < p.slabs; ++i) launch_critic_spectrum_slab(c->cs, wave, wave_stride, n, scale, ws, x, p.T, cs_slab(p, R, i), s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_critic_conv_layout(int32_t C, int32_t I, int32_t T, int32_t O, int32_t out[5])
{
    if (!out) return fail(BSRNN_EARG, "bsrnn_critic_conv_layout: nowhere to write the layout");
    if (int rc = critic_sizes_ok(C, I, T, O, "bsrnn_critic_conv_layout")) return rc;
    const CriticLayout g = critic_layout(C, I, T, O);
    out[0] = g.T_out; out[1] = g.slabs; out[2] = g.ch_per_slab; out[3] = g.dw_chunks; out[4] = g.dw_frames;
    return 0;
}

int bsrnn_critic_conv_forward(bsrnn_ctx* c, const float* x, const float* w, const float* b, float* y, int32_t C, int32_t I, int32_t T,
                              int32_t O, int32_t leaky, void* stream)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!x || !w || !b || !y) return fail(BSRNN_EARG, "bsrnn_critic_conv_forward: null argument (need x_dev, w_dev, b_dev and y_dev)");
    if (int rc = critic_sizes_ok(C, I, T, O, "bsrnn_critic_conv_forward")) return rc;
    if (int rc = check_device(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const size_t n_scr = (size_t)critic_forward_scratch_floats(C, I, T, O);
    float* ws = train_scratch(c, n_scr);
    if (!ws) return fail(BSRNN_EHIP, "bsrnn_critic_conv_forward: out of device memory (%zu MB of workspace)", n_scr * sizeof(float) >> 20);
    launch_critic_forward(x, w, b, y, ws, C, I, T, O, leaky != 0, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

int bsrnn_critic_conv_backward(bsrnn_ctx* c, const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* db,
                               int32_t C, int32_t I, int32_t T, int32_t O, int32_t leaky, void* stream)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!x || !w || !dy || !dw || !db || (leaky && !y))
        return fail(BSRNN_EARG, "bsrnn_critic_conv_backward: null argument (only dx_dev may be null, and y_dev when leaky is 0)");
    if (int rc = critic_sizes_ok(C, I, T, O, "bsrnn_critic_conv_backward")) return rc;
    if (int rc = check_device(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const size_t n_scr = (size_t)critic_backward_scratch_floats(C, I, T, O, leaky != 0);
    float* ws = n_scr ? train_scratch(c, n_scr) : nullptr;
    if (n_scr && !ws) return fail(BSRNN_EHIP, "bsrnn_critic_conv_backward: out of device memory (%zu MB of workspace)", n_scr * sizeof(float) >> 20);
    launch_critic_backward(x, w, y, dy, dx, dw, db, ws, C, I, T, O, leaky != 0, s);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ the committed critic
int bsrnn_critic_score_layout(int32_t in_channels, int32_t C, int32_t T, int64_t out[10])
{
    if (!out) return fail(BSRNN_EARG, "bsrnn_critic_score_layout: nowhere to write the layout");
    if (int rc = score_sizes_ok(in_channels, C, T, CSC_ORDER_PLANAR, "bsrnn_critic_score_layout")) return rc;
    const CscPlan p = csc_plan(in_channels, C, T);
    for (int l = 0; l < CRITIC_LAYERS; ++l) out[l] = p.len[l];
    out[4] = p.slabs; out[5] = p.ch_per_slab; out[6] = p.ws_floats; out[7] = p.ws_exact_floats;
    out[8] = csc_image_halves(in_channels) * 2;
    out[9] = CriticParams(in_channels).total * (int64_t)sizeof(float);
    return 0;
}

int bsrnn_critic_create(bsrnn_ctx* c, int32_t in_channels, bsrnn_critic** out)
{
    if (!c) return fail(BSRNN_EARG, "null context");
    if (!out) return fail(BSRNN_EARG, "bsrnn_critic_create: nowhere to put the object");
    switch (csc_check_channels(in_channels)) {
    case CSC_OK: break;
    case CSC_BAD_CHANNELS: return fail(BSRNN_EARG, "bsrnn_critic_create: need in_channels >= 1, got %d", in_channels);
    default: return fail(BSRNN_EARG, "bsrnn_critic_create: in_channels = %d: the first layer's weights would pass 2^31 - 1 elements", in_channels);
    }
    if (c->zombie) return fail(BSRNN_ESTATE, "context was destroyed");
    bsrnn_critic* k = new bsrnn_critic();
    k->ctx = c; k->I = in_channels;
    if (c->device >= 0) {          // (a host-only context gets an object that answers its argument checks and then BSRNN_ESTATE)
        CallGuard guard_(c);
        if (!guard_.ok) { delete k; return guard_.refuse(); }
        const CriticParams q(in_channels);
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess) e = hipMalloc((void**)&k->d_par, (size_t)q.total * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(&k->d_img, (size_t)csc_image_halves(in_channels) * 2);
        if (e == hipSuccess) e = hipMalloc((void**)&k->d_max, sizeof(unsigned));
        if (e != hipSuccess) {
            (void)hipFree(k->d_par); (void)hipFree(k->d_img); (void)hipFree(k->d_max);
            delete k;
            (void)hipGetLastError();
            return fail(BSRNN_EHIP, "bsrnn_critic_create: %s (the snapshot and the image take %lld MB)", hipGetErrorString(e),
                        (long long)(((int64_t)q.total * 4 + csc_image_halves(in_channels) * 2) >> 20));
        }
        g_dbg[DBG_ALLOC] += 3;
    }
    ++c->live_streams;
    *out = k;
    return 0;
}

void bsrnn_critic_destroy(bsrnn_critic* k)
{
    if (!k) return;
    bsrnn_ctx* c = k->ctx;
    if (c->device >= 0) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(k->d_par); (void)hipFree(k->d_img); (void)hipFree(k->d_max); (void)hipFree(k->d_img_dx);
    }
    delete k;
    if (--c->live_streams == 0 && c->zombie) destroy_now(c);     // as bsrnn_stream_destroy: the context goes with the last object that points at it
}

int bsrnn_critic_commit(bsrnn_critic* k, const float* const conv_w[4], const float* const conv_b[4], const float* lin_w, const float* lin_b,
                        void* stream)
{
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!conv_w || !conv_b || !lin_w || !lin_b) return fail(BSRNN_EARG, "bsrnn_critic_commit: null argument (need conv_w_dev, conv_b_dev, lin_w_dev and lin_b_dev)");
    for (int l = 0; l < CRITIC_LAYERS; ++l)
        if (!conv_w[l] || !conv_b[l]) return fail(BSRNN_EARG, "bsrnn_critic_commit: null weight or bias pointer of layer %d", l);
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const CriticParams q(k->I);
    const float* src[2 * CRITIC_LAYERS + 2];
    for (int l = 0; l < CRITIC_LAYERS; ++l) { src[2 * l] = conv_w[l]; src[2 * l + 1] = conv_b[l]; }
    src[2 * CRITIC_LAYERS] = lin_w; src[2 * CRITIC_LAYERS + 1] = lin_b;
    k->committed = false;
    for (int j = 0; j < 2 * CRITIC_LAYERS + 2; ++j)
        HIP_TRY(hipMemcpyAsync(k->d_par + q.off[j], src[j], (size_t)q.n[j] * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(k->d_max, 0, sizeof(unsigned), s));
    launch_critic_commit(k->d_par + q.off[0], k->d_img, k->d_max, k->I, s);      // (from the snapshot: the caller's may change from here on)
    if (k->d_img_dx) launch_critic_grad_commit(k->d_par + q.off[0], k->d_img_dx, k->I, s);
    HIP_TRY(hipGetLastError());
    unsigned bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, k->d_max, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float top; memcpy(&top, &bits, sizeof(float));
    k->wmax = top;
    k->usable = top <= CSC_F16_MAX;                                               // (false for NaN too)
    k->committed = true;
    return 0;
}

int bsrnn_critic_score(bsrnn_critic* k, const float* x, int32_t C, int32_t T, int32_t x_order, float* score, float* y1, void* stream)
{
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!x || !score) return fail(BSRNN_EARG, "bsrnn_critic_score: null argument (need x_dev and score_dev; only y1_dev may be null)");
    if (int rc = score_sizes_ok(k->I, C, T, x_order, "bsrnn_critic_score")) return rc;
    const CscPlan p = csc_plan(k->I, C, T);
    const size_t nx = (size_t)C * k->I * T * sizeof(float), ny1 = (size_t)C * CSC_O * p.len[0] * sizeof(float);
    if (ranges_overlap(score, sizeof(float), x, nx) || ranges_overlap(y1, ny1, x, nx))
        return fail(BSRNN_EARG, "bsrnn_critic_score: %s overlaps x_dev (a call that left the fp16 range is run again from x)",
                    ranges_overlap(score, sizeof(float), x, nx) ? "score_dev" : "y1_dev");
    if (ranges_overlap(score, sizeof(float), y1, ny1)) return fail(BSRNN_EARG, "bsrnn_critic_score: score_dev overlaps y1_dev");
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    if (!k->committed) return fail(BSRNN_ESTATE, "bsrnn_critic_score: bsrnn_critic_commit() has not been called");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const CriticParams q(k->I);
    const float* const par = k->d_par;
    auto run = [&]() -> int {
        const bool exact = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
        const bool copy = exact && x_order == CSC_ORDER_INTERLEAVED;
        const size_t n_ws = (size_t)(copy ? p.ws_exact_floats : p.ws_floats);
        float* ws = train_scratch(c, n_ws);
        if (!ws) return fail(BSRNN_EHIP, "bsrnn_critic_score: out of device memory (%zu MB of workspace)", n_ws * sizeof(float) >> 20);
        float* yl[CRITIC_LAYERS];
        for (int l = 0; l < CRITIC_LAYERS; ++l) yl[l] = ws + p.off_y[l];
        if (y1) yl[0] = y1;
        float* shared = ws + p.off_shared;
        if (exact) {
            const float* xp = x;
            if (copy) { launch_critic_planar(x, ws + p.ws_floats, C, k->I, T, s); xp = ws + p.ws_floats; }
            launch_critic_forward(xp, par + q.off[0], par + q.off[1], yl[0], shared, C, k->I, T, CSC_O, 1, s);
        } else {
            launch_critic_first_h2(x, k->d_img, par + q.off[1], yl[0], shared, c->d_range, p, x_order, s);
        }
        for (int l = 1; l < CRITIC_LAYERS; ++l)
            launch_critic_forward(yl[l - 1], par + q.off[2 * l], par + q.off[2 * l + 1], yl[l], shared, C, CRITIC_WIDTHS[l - 1], p.len[l - 1],
                                  CRITIC_WIDTHS[l], l + 1 < CRITIC_LAYERS, s);
        launch_critic_tail(yl[CRITIC_LAYERS - 1], par + q.off[2 * CRITIC_LAYERS], par + q.off[2 * CRITIC_LAYERS + 1], score, C,
                           p.len[CRITIC_LAYERS - 1], s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const bool exact_now = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
    if (int rc = run()) return rc;
    if (exact_now) return 0;               // (the exact chain ran: no guard to wait for)
    return finish_call(c, s, run);
}

// ------------------------------------------------------------------------------------------------ the committed critic's gradient
int bsrnn_critic_grad_layout(int32_t in_channels, int32_t C, int32_t T, int64_t out[8])
{
    if (!out) return fail(BSRNN_EARG, "bsrnn_critic_grad_layout: nowhere to write the layout");
    if (int rc = grad_sizes_ok(in_channels, C, T, CSC_ORDER_PLANAR, "bsrnn_critic_grad_layout")) return rc;
    const CgdPlan g = cgd_plan(in_channels, C, T);
    out[0] = g.i_tiles; out[1] = g.s_tiles; out[2] = CGD_CH; out[3] = CGD_TILE_S; out[4] = CGD_TILE_T;
    out[5] = g.ws_floats; out[6] = g.ws_exact_floats; out[7] = cgd_image_halves(in_channels) * 2;
    return 0;
}

int bsrnn_critic_enable_grad(bsrnn_critic* k, void* stream)
{
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (cgd_check_channels(k->I) != CGD_OK)
        return fail(BSRNN_EARG, "bsrnn_critic_enable_grad: in_channels = %d: the dx image would pass 2^31 - 1 elements", k->I);
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if (k->d_img_dx) return 0;
    void* img = nullptr;
    const hipError_t e = hipMalloc(&img, (size_t)cgd_image_halves(k->I) * 2);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(BSRNN_EHIP, "bsrnn_critic_enable_grad: %s (the dx image takes %lld MB)", hipGetErrorString(e),
                    (long long)((cgd_image_halves(k->I) * 2) >> 20));
    }
    ++g_dbg[DBG_ALLOC];
    if (k->committed) {
        launch_critic_grad_commit(k->d_par + CriticParams(k->I).off[0], img, k->I, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    k->d_img_dx = img;
    return 0;
}

int bsrnn_critic_layer1_dx(bsrnn_critic* k, const float* dp, int32_t C, int32_t T, int32_t x_order, float* dx, void* stream)
{
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!dp || !dx) return fail(BSRNN_EARG, "bsrnn_critic_layer1_dx: null argument (need dp_dev and dx_dev)");
    if (int rc = grad_sizes_ok(k->I, C, T, x_order, "bsrnn_critic_layer1_dx")) return rc;
    const CgdPlan g = cgd_plan(k->I, C, T);
    const size_t nx = (size_t)C * k->I * T * sizeof(float), ndp = (size_t)C * CSC_O * g.f.len[0] * sizeof(float);
    if (ranges_overlap(dx, nx, dp, ndp)) return fail(BSRNN_EARG, "bsrnn_critic_layer1_dx: dx_dev overlaps dp_dev (a call that left the fp16 range is run again from dp)");
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    if (!k->committed) return fail(BSRNN_ESTATE, "bsrnn_critic_layer1_dx: bsrnn_critic_commit() has not been called");
    if (!k->d_img_dx) return fail(BSRNN_ESTATE, "bsrnn_critic_layer1_dx: bsrnn_critic_enable_grad() has not been called");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const CriticParams q(k->I);
    auto run = [&]() -> int {
        const bool exact = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
        const size_t n_ws = (size_t)(exact && x_order == CSC_ORDER_INTERLEAVED ? g.ws_exact_floats : g.ws_floats);
        float* ws = train_scratch(c, n_ws);
        if (!ws) return fail(BSRNN_EHIP, "bsrnn_critic_layer1_dx: out of device memory (%zu MB of workspace)", n_ws * sizeof(float) >> 20);
        if (!exact) {
            HIP_TRY(hipMemsetAsync(ws + g.off_max, 0, 4 * sizeof(float), s));
            launch_critic_dp_max(dp, nullptr, nullptr, (unsigned*)(ws + g.off_max), ndp / sizeof(float), s);
        }
        first_layer_dx(k, q, g, dp, ws, dx, x_order, exact, s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const bool exact_now = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
    if (int rc = run()) return rc;
    if (exact_now) return 0;
    return finish_call(c, s, run);
}

int bsrnn_critic_score_grad(bsrnn_critic* k, const float* x, int32_t C, int32_t T, int32_t x_order, const float* gscale, float* score, float* dx,
                            void* stream)
{
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!x || !score || !dx) return fail(BSRNN_EARG, "bsrnn_critic_score_grad: null argument (need x_dev, score_dev and dx_dev; only gscale_dev may be null)");
    if (int rc = grad_sizes_ok(k->I, C, T, x_order, "bsrnn_critic_score_grad")) return rc;
    const CgdPlan g = cgd_plan(k->I, C, T);
    const CscPlan& p = g.f;
    const size_t nx = (size_t)C * k->I * T * sizeof(float);
    if (ranges_overlap(dx, nx, x, nx)) return fail(BSRNN_EARG, "bsrnn_critic_score_grad: dx_dev overlaps x_dev (a call that left the fp16 range is run again from x)");
    if (ranges_overlap(score, sizeof(float), x, nx)) return fail(BSRNN_EARG, "bsrnn_critic_score_grad: score_dev overlaps x_dev");
    if (ranges_overlap(dx, nx, score, sizeof(float))) return fail(BSRNN_EARG, "bsrnn_critic_score_grad: dx_dev overlaps score_dev");
    if (ranges_overlap(gscale, sizeof(float), dx, nx) || ranges_overlap(gscale, sizeof(float), score, sizeof(float)))
        return fail(BSRNN_EARG, "bsrnn_critic_score_grad: gscale_dev overlaps an output (the re-run reads it again)");
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    if (!k->committed) return fail(BSRNN_ESTATE, "bsrnn_critic_score_grad: bsrnn_critic_commit() has not been called");
    if (!k->d_img_dx) return fail(BSRNN_ESTATE, "bsrnn_critic_score_grad: bsrnn_critic_enable_grad() has not been called");
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    const CriticParams q(k->I);
    const float* const par = k->d_par;
    auto run = [&]() -> int {
        const bool exact = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
        const bool copy = exact && x_order == CSC_ORDER_INTERLEAVED;
        const size_t n_ws = (size_t)(copy ? g.ws_exact_floats : g.ws_floats);
        float* ws = train_scratch(c, n_ws);
        if (!ws) return fail(BSRNN_EHIP, "bsrnn_critic_score_grad: out of device memory (%zu MB of workspace)", n_ws * sizeof(float) >> 20);
        float *yl[CRITIC_LAYERS], *dpl[CRITIC_LAYERS];
        for (int l = 0; l < CRITIC_LAYERS; ++l) { yl[l] = ws + p.off_y[l]; dpl[l] = ws + g.off_dp[l]; }
        float* shared = ws + p.off_shared;
        // the score, exactly as bsrnn_critic_score forms it
        if (exact) {
            const float* xp = x;
            if (copy) { launch_critic_planar(x, ws + g.off_xp, C, k->I, T, s); xp = ws + g.off_xp; }
            launch_critic_forward(xp, par + q.off[0], par + q.off[1], yl[0], shared, C, k->I, T, CSC_O, 1, s);
        } else {
            launch_critic_first_h2(x, k->d_img, par + q.off[1], yl[0], shared, c->d_range, p, x_order, s);
        }
        for (int l = 1; l < CRITIC_LAYERS; ++l)
            launch_critic_forward(yl[l - 1], par + q.off[2 * l], par + q.off[2 * l + 1], yl[l], shared, C, CRITIC_WIDTHS[l - 1], p.len[l - 1],
                                  CRITIC_WIDTHS[l], l + 1 < CRITIC_LAYERS, s);
        launch_critic_tail(yl[CRITIC_LAYERS - 1], par + q.off[2 * CRITIC_LAYERS], par + q.off[2 * CRITIC_LAYERS + 1], score, C,
                           p.len[CRITIC_LAYERS - 1], s);
        // and back: the tail, then per layer dy (in the shared block) = dx of the layer above, dp = dy * act'(y); no dW anywhere
        launch_critic_tail_grad(score, par + q.off[2 * CRITIC_LAYERS], gscale, ws + g.off_pool, dpl[CRITIC_LAYERS - 1], C, p.len[CRITIC_LAYERS - 1], s);
        HIP_TRY(hipMemsetAsync(ws + g.off_max, 0, 4 * sizeof(float), s));
        for (int l = CRITIC_LAYERS - 1; l >= 1; --l) {
            const size_t n = (size_t)C * CRITIC_WIDTHS[l - 1] * p.len[l - 1];
            launch_critic_dx(par + q.off[2 * l], dpl[l], shared, C, CRITIC_WIDTHS[l - 1], p.len[l - 1], CRITIC_WIDTHS[l], s);
            if (l > 1) launch_critic_dp(shared, yl[l - 1], dpl[l - 1], n, s);
            else launch_critic_dp_max(shared, yl[0], dpl[0], (unsigned*)(ws + g.off_max), n, s);
        }
        first_layer_dx(k, q, g, dpl[0], ws, dx, x_order, exact, s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const bool exact_now = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
    if (int rc = run()) return rc;
    if (exact_now) return 0;               // (the exact chain ran: no guard to wait for)
    return finish_call(c, s, run);
}

// ------------------------------------------------------------------------------------------------ the committed critic on a padded batch
int bsrnn_critic_ragged_layout(int32_t in_channels, int32_t R, int32_t Tmax, const int32_t* frames, const int32_t* clip_rows, int32_t n_clips,
                               int64_t out[14])
{
    if (!out) return fail(BSRNN_EARG, "bsrnn_critic_ragged_layout: nowhere to write the layout");
    if (!frames || !clip_rows) return fail(BSRNN_EARG, "bsrnn_critic_ragged_layout: null argument (need frames_host and clip_rows_host)");
    if (int rc = ragged_args_ok(in_channels, R, Tmax, frames, clip_rows, n_clips, CSC_ORDER_PLANAR, true, "bsrnn_critic_ragged_layout")) return rc;
    const CrgPlan p = crg_plan(in_channels, R, Tmax, n_clips);
    for (int l = 0; l < CRITIC_LAYERS; ++l) out[l] = p.g.f.len[l];
    out[4] = p.g.f.slabs; out[5] = p.g.f.ch_per_slab;
    out[6] = p.g.f.t_tiles; out[8] = p.g.s_tiles;
    crg_live_tiles(p, frames, clip_rows, &out[7], &out[9]);
    out[10] = p.g.f.ws_floats; out[11] = p.ws_floats; out[12] = p.ws_exact_floats; out[13] = p.table_bytes;
    return 0;
}

// What the three ragged calls share behind their argument checks: the tables go up through the context's ring, in front of the kernels
struct RaggedTables { const CrgRow* rows; const CrgClip* clips; };
static int ragged_upload(bsrnn_ctx* c, const CrgPlan& p, const int32_t* frames, const int32_t* clip_rows, hipStream_t s, RaggedTables* t)
{
    const int R = p.g.f.C;
    const size_t row_bytes = (size_t)R * sizeof(CrgRow);
    if (int rc = c->rg.upload((size_t)p.table_bytes, s, [&](char* h) {
            crg_tables(frames, clip_rows, p.n_clips, reinterpret_cast<CrgRow*>(h), reinterpret_cast<CrgClip*>(h + row_bytes));
        })) return rc;
    t->rows = reinterpret_cast<const CrgRow*>(c->rg.d);
    t->clips = reinterpret_cast<const CrgClip*>(c->rg.d + row_bytes);
    return 0;
}

// The forward of a ragged call into yl[0 .. 3] and scores: the first layer on fp16x2 with its dead tiles skipped (or the exact kernel on the
// rectangle, through a zero-padded planar copy at xp when x is interleaved), layers 2 - 4 on the rectangle, the tail per clip
static void ragged_forward(const bsrnn_critic* k, const CriticParams& q, const CrgPlan& p, const RaggedTables& t, const float* x, float* xp,
                           float* const yl[CRITIC_LAYERS], float* shared, float* scores, int x_order, bool exact, hipStream_t s)
{
    const CscPlan& f = p.g.f;
    const float* const par = k->d_par;
    const int R = f.C, Tmax = f.T;
    if (exact) {
        const float* src = x;
        if (x_order == CSC_ORDER_INTERLEAVED) { launch_critic_planar_ragged(x, xp, R, k->I, Tmax, t.rows, s); src = xp; }
        launch_critic_forward(src, par + q.off[0], par + q.off[1], yl[0], shared, R, k->I, Tmax, CSC_O, 1, s);
    } else {
        launch_critic_first_h2_ragged(x, k->d_img, par + q.off[1], yl[0], shared, k->ctx->d_range, f, x_order, t.rows, s);
    }
    for (int l = 1; l < CRITIC_LAYERS; ++l)
        launch_critic_forward(yl[l - 1], par + q.off[2 * l], par + q.off[2 * l + 1], yl[l], shared, R, CRITIC_WIDTHS[l - 1], f.len[l - 1],
                              CRITIC_WIDTHS[l], l + 1 < CRITIC_LAYERS, s);
    launch_critic_tail_ragged(yl[CRITIC_LAYERS - 1], par + q.off[2 * CRITIC_LAYERS], par + q.off[2 * CRITIC_LAYERS + 1], scores, t.clips, p.n_clips,
                              f.len[CRITIC_LAYERS - 1], s);
}

// The first layer's dx of a ragged call from dp1 [R][1024][T1max] (zeros behind a row's T1_r), whose maxima per clip stand in the max words
static void ragged_first_layer_dx(const bsrnn_critic* k, const CriticParams& q, const CrgPlan& p, const RaggedTables& t, const float* dp1, float* ws,
                                  float* dx, int x_order, bool exact, hipStream_t s)
{
    const int R = p.g.f.C, Tmax = p.g.f.T;
    if (!exact) {
        launch_critic_dx_h2_ragged(dp1, k->d_img_dx, dx, (const unsigned*)(ws + p.off_max), k->ctx->d_range, p.g, x_order, t.rows, s);
    } else if (x_order == CSC_ORDER_INTERLEAVED) {
        launch_critic_dx(k->d_par + q.off[0], dp1, ws + p.off_dxp, R, k->I, Tmax, CSC_O, s);
        launch_critic_scatter(ws + p.off_dxp, dx, R, k->I, Tmax, s);
    } else {
        launch_critic_dx(k->d_par + q.off[0], dp1, dx, R, k->I, Tmax, CSC_O, s);
    }
}

int bsrnn_critic_score_ragged(bsrnn_critic* k, const float* x, int32_t R, int32_t Tmax, const int32_t* frames, const int32_t* clip_rows,
                              int32_t n_clips, int32_t x_order, float* scores, float* y1, void* stream)
{
    const char* who = "bsrnn_critic_score_ragged";
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!x || !frames || !clip_rows || !scores)
        return fail(BSRNN_EARG, "%s: null argument (need x_dev, frames_host, clip_rows_host and scores_dev; only y1_dev may be null)", who);
    if (int rc = ragged_args_ok(k->I, R, Tmax, frames, clip_rows, n_clips, x_order, false, who)) return rc;
    const CrgPlan p = crg_plan(k->I, R, Tmax, n_clips);
    const CscPlan& f = p.g.f;
    const size_t nx = (size_t)R * k->I * Tmax * sizeof(float), ns = (size_t)n_clips * sizeof(float), ny1 = (size_t)R * CSC_O * f.len[0] * sizeof(float);
    if (ranges_overlap(scores, ns, x, nx) || ranges_overlap(y1, ny1, x, nx))
        return fail(BSRNN_EARG, "%s: %s overlaps x_dev (a call that left the fp16 range is run again from x)", who,
                    ranges_overlap(scores, ns, x, nx) ? "scores_dev" : "y1_dev");
    if (ranges_overlap(scores, ns, y1, ny1)) return fail(BSRNN_EARG, "%s: scores_dev overlaps y1_dev", who);
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    if (!k->committed) return fail(BSRNN_ESTATE, "%s: bsrnn_critic_commit() has not been called", who);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    RaggedTables t{};
    if (int rc = ragged_upload(c, p, frames, clip_rows, s, &t)) return rc;
    const CriticParams q(k->I);
    auto run = [&]() -> int {
        const bool exact = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
        const bool copy = exact && x_order == CSC_ORDER_INTERLEAVED;
        const size_t n_ws = (size_t)(copy ? f.ws_exact_floats : f.ws_floats);
        float* ws = train_scratch(c, n_ws);
        if (!ws) return fail(BSRNN_EHIP, "%s: out of device memory (%zu MB of workspace)", who, n_ws * sizeof(float) >> 20);
        float* yl[CRITIC_LAYERS];
        for (int l = 0; l < CRITIC_LAYERS; ++l) yl[l] = ws + f.off_y[l];
        if (y1) yl[0] = y1;
        ragged_forward(k, q, p, t, x, ws + f.ws_floats, yl, ws + f.off_shared, scores, x_order, exact, s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const bool exact_now = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
    if (int rc = run()) return rc;
    if (exact_now) return 0;               // (the exact chain ran: no guard to wait for)
    return finish_call(c, s, run);
}

int bsrnn_critic_layer1_dx_ragged(bsrnn_critic* k, const float* dp, int32_t R, int32_t Tmax, const int32_t* frames, const int32_t* clip_rows,
                                  int32_t n_clips, int32_t x_order, float* dx, void* stream)
{
    const char* who = "bsrnn_critic_layer1_dx_ragged";
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!dp || !frames || !clip_rows || !dx) return fail(BSRNN_EARG, "%s: null argument (need dp_dev, frames_host, clip_rows_host and dx_dev)", who);
    if (int rc = ragged_args_ok(k->I, R, Tmax, frames, clip_rows, n_clips, x_order, true, who)) return rc;
    const CrgPlan p = crg_plan(k->I, R, Tmax, n_clips);
    const size_t n_row = (size_t)CSC_O * p.g.f.len[0], nx = (size_t)R * k->I * Tmax * sizeof(float), ndp = (size_t)R * n_row * sizeof(float);
    if (ranges_overlap(dx, nx, dp, ndp)) return fail(BSRNN_EARG, "%s: dx_dev overlaps dp_dev (a call that left the fp16 range is run again from dp)", who);
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    if (!k->committed) return fail(BSRNN_ESTATE, "%s: bsrnn_critic_commit() has not been called", who);
    if (!k->d_img_dx) return fail(BSRNN_ESTATE, "%s: bsrnn_critic_enable_grad() has not been called", who);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    RaggedTables t{};
    if (int rc = ragged_upload(c, p, frames, clip_rows, s, &t)) return rc;
    const CriticParams q(k->I);
    auto run = [&]() -> int {
        const bool exact = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
        const size_t n_ws = (size_t)(exact && x_order == CSC_ORDER_INTERLEAVED ? p.ws_exact_floats : p.ws_floats);
        float* ws = train_scratch(c, n_ws);
        if (!ws) return fail(BSRNN_EHIP, "%s: out of device memory (%zu MB of workspace)", who, n_ws * sizeof(float) >> 20);
        if (!exact) {
            HIP_TRY(hipMemsetAsync(ws + p.off_max, 0, (size_t)csc_round4(n_clips) * sizeof(float), s));
            launch_critic_dp_max_rows(dp, nullptr, nullptr, (unsigned*)(ws + p.off_max), t.rows, R, n_row, s);
        }
        ragged_first_layer_dx(k, q, p, t, dp, ws, dx, x_order, exact, s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const bool exact_now = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
    if (int rc = run()) return rc;
    if (exact_now) return 0;
    return finish_call(c, s, run);
}

int bsrnn_critic_score_grad_ragged(bsrnn_critic* k, const float* x, int32_t R, int32_t Tmax, const int32_t* frames, const int32_t* clip_rows,
                                   int32_t n_clips, int32_t x_order, const float* gscale, float* scores, float* dx, void* stream)
{
    const char* who = "bsrnn_critic_score_grad_ragged";
    if (!k) return fail(BSRNN_EARG, "null critic");
    if (!x || !frames || !clip_rows || !scores || !dx)
        return fail(BSRNN_EARG, "%s: null argument (need x_dev, frames_host, clip_rows_host, scores_dev and dx_dev; only gscale_dev may be null)", who);
    if (int rc = ragged_args_ok(k->I, R, Tmax, frames, clip_rows, n_clips, x_order, true, who)) return rc;
    const CrgPlan p = crg_plan(k->I, R, Tmax, n_clips);
    const CscPlan& f = p.g.f;
    const size_t nx = (size_t)R * k->I * Tmax * sizeof(float), ns = (size_t)n_clips * sizeof(float);
    if (ranges_overlap(dx, nx, x, nx)) return fail(BSRNN_EARG, "%s: dx_dev overlaps x_dev (a call that left the fp16 range is run again from x)", who);
    if (ranges_overlap(scores, ns, x, nx)) return fail(BSRNN_EARG, "%s: scores_dev overlaps x_dev", who);
    if (ranges_overlap(dx, nx, scores, ns)) return fail(BSRNN_EARG, "%s: dx_dev overlaps scores_dev", who);
    if (ranges_overlap(gscale, ns, dx, nx) || ranges_overlap(gscale, ns, scores, ns))
        return fail(BSRNN_EARG, "%s: gscale_dev overlaps an output (the re-run reads it again)", who);
    bsrnn_ctx* c = k->ctx;
    if (int rc = check_device(c)) return rc;
    if (!k->committed) return fail(BSRNN_ESTATE, "%s: bsrnn_critic_commit() has not been called", who);
    if (!k->d_img_dx) return fail(BSRNN_ESTATE, "%s: bsrnn_critic_enable_grad() has not been called", who);
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    RaggedTables t{};
    if (int rc = ragged_upload(c, p, frames, clip_rows, s, &t)) return rc;
    const CriticParams q(k->I);
    const float* const par = k->d_par;
    auto run = [&]() -> int {
        const bool exact = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
        const bool copy = exact && x_order == CSC_ORDER_INTERLEAVED;
        const size_t n_ws = (size_t)(copy ? p.ws_exact_floats : p.ws_floats);
        float* ws = train_scratch(c, n_ws);
        if (!ws) return fail(BSRNN_EHIP, "%s: out of device memory (%zu MB of workspace)", who, n_ws * sizeof(float) >> 20);
        float *yl[CRITIC_LAYERS], *dpl[CRITIC_LAYERS];
        for (int l = 0; l < CRITIC_LAYERS; ++l) { yl[l] = ws + f.off_y[l]; dpl[l] = ws + p.g.off_dp[l]; }
        float* shared = ws + f.off_shared;
        // the scores, exactly as bsrnn_critic_score_ragged forms them
        ragged_forward(k, q, p, t, x, ws + p.off_xp, yl, shared, scores, x_order, exact, s);
        // and back: the tail per clip (zeros behind a row's T4_r), then layers 4 .. 2 on the rectangle, dp1 with the maximum per clip
        launch_critic_tail_grad_ragged(scores, par + q.off[2 * CRITIC_LAYERS], gscale, ws + p.off_pool, dpl[CRITIC_LAYERS - 1], t.clips, n_clips,
                                       f.len[CRITIC_LAYERS - 1], s);
        HIP_TRY(hipMemsetAsync(ws + p.off_max, 0, (size_t)csc_round4(n_clips) * sizeof(float), s));
        for (int l = CRITIC_LAYERS - 1; l >= 1; --l) {
            const size_t n_row = (size_t)CRITIC_WIDTHS[l - 1] * f.len[l - 1];
            launch_critic_dx(par + q.off[2 * l], dpl[l], shared, R, CRITIC_WIDTHS[l - 1], f.len[l - 1], CRITIC_WIDTHS[l], s);
            if (l > 1) launch_critic_dp(shared, yl[l - 1], dpl[l - 1], (size_t)R * n_row, s);
            else launch_critic_dp_max_rows(shared, yl[0], dpl[0], (unsigned*)(ws + p.off_max), t.rows, R, n_row, s);
        }
        ragged_first_layer_dx(k, q, p, t, dpl[0], ws, dx, x_order, exact, s);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    const bool exact_now = force_f32() || gemm_mode() == GEMM_F32 || !k->usable;
    if (int rc = run()) return rc;
    if (exact_now) return 0;               // (the exact chain ran: no guard to wait for)
    return finish_call(c, s, run);
}

}  // extern "C"
