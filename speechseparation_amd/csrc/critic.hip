// The critic's layers (reference bsrnn.py:512-536): Conv1d(kernel 16, stride 3) forward and backward, exact fp32 on
// v_mfma_f32_16x16x4_f32 like the training products of train_ops.hip.  The definition, the tiling and the order of every sum:
// critic_host.h.  x [C][I][T], W [O][I][16], y / dy / dp [C][O][T_out], all dense.
//   forward   a product with M = o, N = t, K = (i, k): a tile of 64 o x 64 t of one row c and one slab of input channels; per stage of
//             four channels the W block [64 o][64 (i, k)] (K-contiguous in memory) and four spans of 205 floats of x go to LDS, the B
//             fragments are read at 3 t + k.  Partial sums per slab go to scratch; critic_finish_kernel adds them in slab order, then the
//             bias, then the activation.
//   dW, db    M = o, N = (i, k), K = (c, t): a tile of 64 o x 4 channels and one chunk of frames; dp [64 o][32 t] and four spans of
//             109 floats of x per stage.  db rides along in the tiles of the first channel group (the dp block is in LDS anyway).
//   dx        M = (i, k), N = t, K = o gives G[i][k][t] = sum_o W[o][i][k] dp[o][t] for four channels and 64 frames; the tile then folds G
//             through LDS into the 177 input positions those frames complete (at most six taps each, added in tap order).
// No atomics; no kernel here uses scratch memory.
#include "kernels.h"

namespace bsrnn {

typedef float v4f __attribute__((ext_vector_type(4)));

namespace {

constexpr int SW_LD = 68;        // forward: W rows of 64 k, lane (o = l & 15, k = l >> 4) reads bank 4 o + k: no conflict
constexpr int SX_LD = 208;       // a span of 205 floats
constexpr int SDP_LD = 36;       // dW: dp rows of 32 t, lane (o, t) reads bank 36 o + t: no conflict
constexpr int SXW_LD = 112;      // dW: a span of 3 * 31 + 16 = 109 floats
constexpr int DX_KS = 32;        // dx: output channels o per stage
constexpr int DX_LD = 80;        // dx: rows of 64 (i, k) resp. 64 t, lane (m, o) reads bank 16 o + m: no conflict

__global__ __launch_bounds__(256) void critic_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ part,
                                                         int C, int I, int T, int O, CriticLayout g)
{
    __shared__ float sw[CRITIC_TILE][SW_LD], sx[CRITIC_CH][SX_LD];
    int b = blockIdx.x;
    const int bt = b % g.t_tiles; b /= g.t_tiles;
    const int bo = b % g.o_tiles; b /= g.o_tiles;
    const int c = b % C, slab = b / C;
    const int t0 = bt * CRITIC_TILE, o0 = bo * CRITIC_TILE;
    const int i_lo = slab * g.ch_per_slab, i_hi = min(I, i_lo + g.ch_per_slab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const size_t ldw = (size_t)I * CRITIC_TAPS;
    v4f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int i0 = i_lo; i0 < i_hi; i0 += CRITIC_CH) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int idx = tid + 256 * r, o = idx >> 6, kk = idx & 63;
            sw[o][kk] = (o0 + o < O && i0 + (kk >> 4) < i_hi) ? w[(size_t)(o0 + o) * ldw + (size_t)i0 * CRITIC_TAPS + kk] : 0.f;
        }
        for (int idx = tid; idx < CRITIC_CH * CRITIC_SPAN; idx += 256) {
            const int ch = idx / CRITIC_SPAN, p = idx - ch * CRITIC_SPAN, pos = CRITIC_STRIDE * t0 + p;
            sx[ch][p] = (i0 + ch < i_hi && pos < T) ? x[((size_t)c * I + i0 + ch) * T + pos] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < CRITIC_CH; ++ch)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float a = sw[16 * wave + l15][16 * ch + 4 * s + q];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sx[ch][CRITIC_STRIDE * (16 * j + l15) + 4 * s + q], acc[j], 0, 0, 0);
            }
        __syncthreads();
    }
    float* out = part + ((size_t)slab * C + c) * O * g.T_out;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + 16 * wave + 4 * q + r, t = t0 + 16 * j + l15;
            if (o < O && t < g.T_out) out[(size_t)o * g.T_out + t] = acc[j][r];
        }
}

// y = act(((p_0 + p_1) + ... + p_{slabs - 1}) + b[o]) over the n = C * O * T_out outputs, records of n floats
__global__ __launch_bounds__(256) void critic_finish_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y,
                                                            size_t n, int O, int T_out, int slabs, int leaky)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = part[i];
    for (int s = 1; s < slabs; ++s) v += part[(size_t)s * n + i];
    v += bias[(i / T_out) % O];
    y[i] = (leaky && v < 0.f) ? 0.01f * v : v;
}

// dp = dy * act'(y): slope 0.01 where y <= 0 (leaky_bwd_kernel's convention)
__global__ __launch_bounds__(256) void critic_dp_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dp, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gr = dy[i];
    dp[i] = y[i] > 0.f ? gr : 0.01f * gr;
}

// The record of chunk blockIdx.z: [O * I * 16 product | O row sums of dp] at outw / outb + z * rec (rec = 0 with one chunk: dW, db in place)
__global__ __launch_bounds__(256) void critic_dw_kernel(const float* __restrict__ x, const float* __restrict__ dp, float* __restrict__ outw,
                                                        float* __restrict__ outb, size_t rec, int C, int I, int T, int O, CriticLayout g)
{
    __shared__ float sdp[CRITIC_TILE][SDP_LD], sx[CRITIC_CH][SXW_LD], sred[4][CRITIC_TILE];
    int b = blockIdx.x;
    const int bi = b % g.i_tiles; b /= g.i_tiles;
    const int bo = b % g.o_tiles, z = b / g.o_tiles;
    const int i0 = bi * CRITIC_CH, o0 = bo * CRITIC_TILE;
    const int t_lo = z * g.dw_frames, t_hi = min(g.T_out, t_lo + g.dw_frames);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    constexpr int span = CRITIC_STRIDE * (CRITIC_DW_FRAMES - 1) + CRITIC_TAPS;
    v4f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
    float csum = 0.f;
    for (int c = 0; c < C; ++c)
        for (int ts = t_lo; ts < t_hi; ts += CRITIC_DW_FRAMES) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int idx = tid + 256 * r, o = idx >> 5, tt = idx & 31;
                sdp[o][tt] = (o0 + o < O && ts + tt < t_hi) ? dp[((size_t)c * O + o0 + o) * g.T_out + ts + tt] : 0.f;
            }
            for (int idx = tid; idx < CRITIC_CH * span; idx += 256) {
                const int ch = idx / span, p = idx - ch * span, pos = CRITIC_STRIDE * ts + p;
                sx[ch][p] = (i0 + ch < I && pos < T) ? x[((size_t)c * I + i0 + ch) * T + pos] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < CRITIC_DW_FRAMES / 4; ++s) {
                const float a = sdp[16 * wave + l15][4 * s + q];
                csum += a;                                    // (frames 4 s + q of output channel 16 wave + l15; used by the first channel group)
#pragma unroll
                for (int j = 0; j < 4; ++j)                   // N block j = channel j, column l15 = tap
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sx[j][CRITIC_STRIDE * (4 * s + q) + l15], acc[j], 0, 0, 0);
            }
            __syncthreads();
        }
    float* ow = outw + (size_t)z * rec;
    const size_t ldw = (size_t)I * CRITIC_TAPS;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + 16 * wave + 4 * q + r;
            if (o < O && i0 + j < I) ow[(size_t)o * ldw + (size_t)(i0 + j) * CRITIC_TAPS + l15] = acc[j][r];
        }
    if (bi == 0) {                                            // the four frame quarters of an output channel, added in a fixed order
        sred[q][16 * wave + l15] = csum;
        __syncthreads();
        if (tid < CRITIC_TILE && o0 + tid < O) outb[(size_t)z * rec + o0 + tid] = (sred[0][tid] + sred[1][tid]) + (sred[2][tid] + sred[3][tid]);
    }
}

// out[i] = ((r_0[i] + r_1[i]) + ...) over the chunks' records of n1 + n2 floats: the first n1 go to dW, the rest to db
__global__ __launch_bounds__(256) void critic_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                            size_t n1, size_t n2, int chunks)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = n1 + n2;
    if (i >= n) return;
    float v = part[i];
    for (int z = 1; z < chunks; ++z) v += part[(size_t)z * n + i];
    if (i < n1) dw[i] = v;
    else db[i - n1] = v;
}

__global__ __launch_bounds__(256) void critic_dx_kernel(const float* __restrict__ w, const float* __restrict__ dp, float* __restrict__ dx,
                                                        int C, int I, int T, int O, CriticLayout g)
{
    __shared__ float sw[DX_KS][DX_LD], sd[DX_KS][DX_LD], sg[CRITIC_CH * CRITIC_TAPS][CRITIC_TILE + 1];
    int b = blockIdx.x;
    const int bs = b % g.s_tiles; b /= g.s_tiles;
    const int bi = b % g.i_tiles, c = b / g.i_tiles;
    const int i0 = bi * CRITIC_CH, s0 = bs * CRITIC_DX_TILE;
    const int t_lo = bs * (CRITIC_TILE - CRITIC_DX_HALO) - CRITIC_DX_HALO;       // frames [t_lo, t_lo + 64); those outside [0, T_out) are zeros
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q = lane >> 4;
    const size_t ldw = (size_t)I * CRITIC_TAPS;
    v4f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (v4f){0.f, 0.f, 0.f, 0.f};
    for (int ob = 0; ob < O; ob += DX_KS) {
#pragma unroll
        for (int r = 0; r < DX_KS / 4; ++r) {
            const int idx = tid + 256 * r, o = idx >> 6, m = idx & 63, t = t_lo + m;
            sw[o][m] = (ob + o < O && i0 + (m >> 4) < I) ? w[(size_t)(ob + o) * ldw + (size_t)i0 * CRITIC_TAPS + m] : 0.f;
            sd[o][m] = (ob + o < O && t >= 0 && t < g.T_out) ? dp[((size_t)c * O + ob + o) * g.T_out + t] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < DX_KS / 4; ++s) {
            const float a = sw[4 * s + q][16 * wave + l15];      // A[(i, k)][o] = W[o][i][k]
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sd[4 * s + q][16 * j + l15], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sg[16 * wave + 4 * q + r][16 * j + l15] = acc[j][r];       // G[(channel wave, tap 4 q + r)][frame]
    __syncthreads();
    // position s0 + d takes tap k from frame (s0 + d - k) / 3 = t_lo + 5 + (d - k) / 3 for k = d % 3, d % 3 + 3, ... (in that order)
    for (int idx = tid; idx < CRITIC_CH * CRITIC_DX_TILE; idx += 256) {
        const int ch = idx / CRITIC_DX_TILE, d = idx - ch * CRITIC_DX_TILE, s = s0 + d;
        if (i0 + ch >= I || s >= T) continue;
        float v = 0.f;
        for (int k = d % CRITIC_STRIDE; k < CRITIC_TAPS; k += CRITIC_STRIDE) v += sg[ch * CRITIC_TAPS + k][CRITIC_DX_HALO + (d - k) / CRITIC_STRIDE];
        dx[((size_t)c * I + i0 + ch) * T + s] = v;
    }
}

}  // namespace

void launch_critic_forward(const float* x, const float* w, const float* b, float* y, float* scratch, int C, int I, int T, int O, int leaky,
                           hipStream_t s)
{
    const CriticLayout g = critic_layout(C, I, T, O);
    const size_t n = (size_t)C * O * g.T_out;
    hipLaunchKernelGGL(critic_fwd_kernel, dim3((unsigned)((size_t)g.t_tiles * g.o_tiles * C * g.slabs)), dim3(256), 0, s, x, w, scratch, C, I, T, O, g);
    hipLaunchKernelGGL(critic_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scratch, b, y, n, O, g.T_out, g.slabs, leaky);
}

void launch_critic_backward(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* db, float* scratch,
                            int C, int I, int T, int O, int leaky, hipStream_t s)
{
    const CriticLayout g = critic_layout(C, I, T, O);
    const size_t n = (size_t)C * O * g.T_out;
    const float* dp = dy;
    if (leaky) {
        hipLaunchKernelGGL(critic_dp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, y, scratch, n);
        dp = scratch;
        scratch += (n + 3) / 4 * 4;
    }
    const unsigned tiles = (unsigned)((size_t)g.i_tiles * g.o_tiles * g.dw_chunks);
    if (g.dw_chunks == 1) {
        hipLaunchKernelGGL(critic_dw_kernel, dim3(tiles), dim3(256), 0, s, x, dp, dw, db, (size_t)0, C, I, T, O, g);
    } else {
        const size_t n1 = (size_t)O * I * CRITIC_TAPS, rec = n1 + O;
        hipLaunchKernelGGL(critic_dw_kernel, dim3(tiles), dim3(256), 0, s, x, dp, scratch, scratch + n1, rec, C, I, T, O, g);
        hipLaunchKernelGGL(critic_reduce_kernel, dim3((unsigned)((rec + 255) / 256)), dim3(256), 0, s, scratch, dw, db, n1, (size_t)O, g.dw_chunks);
    }
    if (dx)
        hipLaunchKernelGGL(critic_dx_kernel, dim3((unsigned)((size_t)g.s_tiles * g.i_tiles * C)), dim3(256), 0, s, w, dp, dx, C, I, T, O, g);
}

void launch_critic_dp(const float* dy, const float* y, float* dp, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(critic_dp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, y, dp, n);
}

void launch_critic_dx(const float* w, const float* dp, float* dx, int C, int I, int T, int O, hipStream_t s)
{
    const CriticLayout g = critic_layout(C, I, T, O);
    hipLaunchKernelGGL(critic_dx_kernel, dim3((unsigned)((size_t)g.s_tiles * g.i_tiles * C)), dim3(256), 0, s, w, dp, dx, C, I, T, O, g);
}

}  // namespace bsrnn
