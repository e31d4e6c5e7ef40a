// C ABI of libbsrnn_hip.so, the critic's layers (bsrnn_critic_conv_*): Conv1d(kernel 16, stride 3) forward and backward for the
// reference's Discriminator (bsrnn.py:512-536).  The definition and every size: critic_host.h; the kernels: critic.hip.  The scratch is
// the training entry points' grow-only buffer of the context.
// And the critic's input (bsrnn_critic_spectrum): the 4096-point analysis of the reference's train-discriminator.py:62-68.  The definition,
// the slab rule and every size: critic_spectrum_host.h; the kernels: stft4096.hip.
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

}  // extern "C"
