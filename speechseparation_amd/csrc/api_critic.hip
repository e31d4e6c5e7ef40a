// C ABI of libbsrnn_hip.so, the critic's layers (bsrnn_critic_conv_*): Conv1d(kernel 16, stride 3) forward and backward for the
// reference's Discriminator (bsrnn.py:512-536).  The definition and every size: critic_host.h; the kernels: critic.hip.  The scratch is
// the training entry points' grow-only buffer of the context.
#include "api_internal.h"

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

extern "C" {

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
