// The committed critic's own kernels (bsrnn_critic_commit / _score; the layout, the plan and the order of every sum: critic_score_host.h).
//   critic_commit_kernel   W [1024][I][16] fp32 -> the fp16x2 image in A-fragment order (16-byte units), and max |W|.
//   critic_fwd_h2_kernel   layer 1 as a product M = o, N = t, K = (i, k) on v_mfma_f32_32x32x16_f16, three terms (gemm.hip, Piece<2>): a tile
//                          of 128 o x 128 t of one row c and one slab of input channels per workgroup, four waves as 2 (o) x 2 (t).  Per
//                          stage of two channels 16 KB of the image are copied to LDS as they lie, and x goes to LDS as an im2col image
//                          [channel][piece][tap half h][t][8 taps]: the lane that stages (t, h) reads the 8 floats x[3 t + 8 h ..] itself
//                          (only 4-byte aligned in a plain span: 3 t + 8 h), splits them and writes ONE aligned 16-byte unit per piece, so
//                          that every B fragment is one aligned ds_read_b128 and lanes of a wave read and write contiguous LDS.  The price:
//                          a sample of x is loaded (from L1) and split by up to six lanes instead of one.  Two LDS stages, one barrier per
//                          stage; the next stage is loaded behind and split between the current stage's MFMAs, as in gemm_h2_kernel.
//   critic_h2_finish_kernel  y1 = leaky(((p_0 + p_1) + ...) + b[o]) over the slabs' partial sums hi + 2^-11 lo.
//   critic_tail_kernel     [C][32][T4] -> mean over t, mean over c, Linear(32, 1), sigmoid: one float, in a fixed order.
//   critic_planar_kernel   an interleaved x in the reference's channel order (the exact chain reads that).
//   critic_fwd_h2_kernel<true>, critic_tail_ragged_kernel, critic_planar_ragged_kernel   the same three on a padded batch of clips of
//                          different lengths (bsrnn_critic_score_ragged; critic_ragged_host.h): tiles against the row's own length, dead tiles
//                          return before staging, one tail workgroup and one score per clip, zeros behind a row's frames in the planar copy.
// No atomics except the commit's order-free integer max; no kernel here uses scratch memory.
#include "kernels.h"

namespace bsrnn {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int ST_A = CSC_CH * CSC_BLOCK;                         // halves of a stage's weight blocks: 8192
constexpr int ST_BP = 2 * CSC_TILE_T * 8;                        // halves of one piece of one channel of the im2col image: [h][t][8]
constexpr int ST_B = CSC_CH * 2 * ST_BP;                         // 8192
constexpr int STAGE = ST_A + ST_B;                               // 32 KB
static_assert(ST_A == 256 * 4 * 8, "four 16-byte units of the image per thread and stage");
static_assert(CSC_TILE_T * 2 == 256, "one (t, h) unit per thread and channel");

// Piece<2>::split of gemm.hip on eight values: a1 = fp16(a), a2 = fp16(2^11 (a - a1)), the difference and the scaling exact in fp32
__device__ __forceinline__ void split8(const float (&a)[8], h8& p0, h8& p1)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) p0[j] = (_Float16)a[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) p1[j] = (_Float16)__builtin_fmaf(-(float)p0[j], 2048.f, a[j] * 2048.f);
}

__global__ __launch_bounds__(256) void critic_commit_kernel(const float* __restrict__ w, _Float16* __restrict__ img, unsigned* __restrict__ wmax,
                                                            int I, int64_t units)
{
    __shared__ unsigned smax[4];
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned m = 0;
    if (u < units) {
        int o, i, k, piece;
        h8 p0 = {}, p1 = {};
        if (csc_image_source(I, 8 * u, &o, &i, &k, &piece)) {
            float a[8];
            const float* src = w + ((size_t)o * I + i) * CRITIC_TAPS + k;          // k is 0 or 8
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = src[j];
            split8(a, p0, p1);
            if (piece == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const unsigned b = __float_as_uint(a[j]) & 0x7fffffffu; m = b > m ? b : m; }      // (NaN bits order above infinity)
            }
        }
        *reinterpret_cast<h8*>(img + 8 * u) = piece == 0 ? p0 : p1;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned v = __shfl_xor(m, d); m = v > m ? v : m; }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        if (m) atomicMax(wmax, m);
    }
}

// RAGGED (bsrnn_critic_score_ragged; critic_ragged_host.h): row c holds rows[c].frames <= T frames; the tile is taken against the row's own
// T1_r, a tile wholly at or behind it returns before it stages anything, and nothing at or behind x[c][.][rows[c].frames] is loaded.
template <bool RAGGED>
__global__ __launch_bounds__(256, 2) void critic_fwd_h2_kernel(const float* __restrict__ x, const _Float16* __restrict__ img, float* __restrict__ part,
                                                               int* range_flag, CscPlan p, int x_order, const CrgRow* __restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) _Float16 sm[2 * STAGE];
    // The tiles (c, t tile) of one (slab, o tile) read the same weight blocks: they sit on consecutive workgroups of one XCD (speed only)
    const int inner_n = p.C * p.t_tiles, groups = p.slabs * p.o_tiles;
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int inner = q % inner_n, grp = (q / inner_n) * 8 + xcd;
    if (grp >= groups) return;
    const int bt = inner % p.t_tiles, c = inner / p.t_tiles;
    const int bo = grp % p.o_tiles, slab = grp / p.o_tiles;
    const int I = p.I, T = p.T, T1 = p.len[0];
    const int t0 = bt * CSC_TILE_T, o0 = bo * CSC_TILE_O;
    int T1r = T1;                                            // the row's own frames behind the layer (T and T1 stay the strides)
    if constexpr (RAGGED) {
        T1r = crg_t_out(rows[c].frames);
        if (t0 >= T1r) return;
    }
    const int i_lo = slab * p.ch_per_slab, i_hi = min(I, i_lo + p.ch_per_slab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, half = lane >> 5, r32 = lane & 31;

    // staging: four 16-byte units of the stage's 16 KB of the image, and the unit (t = tid & 127, h = tid >> 7) of both channels
    const _Float16* const a_src = img + (size_t)bo * csc_i_pad(I) * CSC_BLOCK + 8 * tid;
    const int st = tid & (CSC_TILE_T - 1), sh = tid >> 7;
    const bool t_in = t0 + st < T1r;                         // (then 3 (t0 + st) + 15 < T: the 16 taps lie inside the row)
    const float* const x_src = x + (size_t)c * I * T + CRITIC_STRIDE * (t0 + st) + 8 * sh;
    h8 ra[4];
    float rx[CSC_CH][8];
    auto gload = [&](int i0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ra[r] = *reinterpret_cast<const h8*>(a_src + (size_t)i0 * CSC_BLOCK + 2048 * r);
#pragma unroll
        for (int r = 0; r < CSC_CH; ++r) {
            if (t_in && i0 + r < I) {
                const float* s = x_src + (size_t)csc_channel_row(I, i0 + r, x_order) * T;
#pragma unroll
                for (int j = 0; j < 8; ++j) rx[r][j] = s[j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) rx[r][j] = 0.f;
            }
        }
    };
    float amax = 0.f;                                        // largest |x| staged by this thread (range guard; NaN drops out, as in gemm.hip)
    auto put_a = [&](_Float16* stg) {
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<h8*>(stg + 8 * tid + 2048 * r) = ra[r];
    };
    auto put_x = [&](_Float16* stg) {
#pragma unroll
        for (int r = 0; r < CSC_CH; ++r) {
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, __builtin_fabsf(rx[r][j]));
            h8 p0, p1;
            split8(rx[r], p0, p1);
            _Float16* d = stg + ST_A + r * 2 * ST_BP + sh * (CSC_TILE_T * 8) + st * 8;
            *reinterpret_cast<h8*>(d) = p0;
            *reinterpret_cast<h8*>(d + ST_BP) = p1;
        }
    };

    v16f hi[2][2], lo[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { hi[a][b] = (v16f){0}; lo[a][b] = (v16f){0}; }

    // fragment offsets (halves): A sub-tile 2 wm + s2 of [piece][sub-tile][lane][8]; B lane (t = 64 wn + 32 n2 + r32, h = half) of [piece][h][t][8]
    const int fa = (2 * wm) * 512 + lane * 8;
    const int fb = ST_A + half * (CSC_TILE_T * 8) + (64 * wn + r32) * 8;

    gload(i_lo);
    put_a(sm);
    put_x(sm);
    if (i_lo + CSC_CH < i_hi) gload(i_lo + CSC_CH);
    __syncthreads();
    int n = 0;
    for (int i0 = i_lo; i0 < i_hi; i0 += CSC_CH, ++n) {
        const _Float16* const cur = sm + (n & 1) * STAGE;
        _Float16* const nxt = sm + ((n + 1) & 1) * STAGE;
        const bool more = i0 + CSC_CH < i_hi;                // the registers hold stage i0 + CSC_CH
#pragma unroll
        for (int ch = 0; ch < CSC_CH; ++ch) {
            h8 a[2][2], b[2][2];
#pragma unroll
            for (int pc = 0; pc < 2; ++pc)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    a[s][pc] = *reinterpret_cast<const h8*>(cur + ch * CSC_BLOCK + pc * (CSC_BLOCK / 2) + fa + s * 512);
                    b[s][pc] = *reinterpret_cast<const h8*>(cur + ch * 2 * ST_BP + pc * ST_BP + fb + s * 256);
                }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    lo[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s][1], b[j][0], lo[s][j], 0, 0, 0);
                    lo[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s][0], b[j][1], lo[s][j], 0, 0, 0);
                    hi[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s][0], b[j][0], hi[s][j], 0, 0, 0);
                }
            // the next stage rides behind this channel's MFMAs: the weight copy after the first, the split of x after the second
            if (more) {
                if (ch == 0) put_a(nxt);
                else put_x(nxt);
            }
        }
        if (i0 + 2 * CSC_CH < i_hi) gload(i0 + 2 * CSC_CH);
        __syncthreads();
    }

    // C / D layout of the 32x32 MFMA: column (t) = lane & 31, row (o) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float* const out = part + ((size_t)slab * p.C + c) * CSC_O * T1;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t = t0 + 64 * wn + 32 * j + r32;
            if (t >= T1r) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int o = o0 + 64 * wm + 32 * s + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                out[(size_t)o * T1 + t] = hi[s][j][reg] + lo[s][j][reg] * (1.f / 2048.f);
            }
        }
    if (amax > CSC_F16_MAX && range_flag) *range_flag = 1;
}

__global__ __launch_bounds__(256) void critic_h2_finish_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y,
                                                               size_t n, int T_out, int slabs)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = part[i];
    for (int s = 1; s < slabs; ++s) v += part[(size_t)s * n + i];
    v += bias[(i / T_out) % CSC_O];
    y[i] = v >= 0.f ? v : 0.01f * v;
}

// One workgroup: thread (o = tid & 31, g = tid >> 5) adds frames g, g + 8, ... of channel o of row c in order; the eight runs are added
// in order and divided by T4 (the mean over t), the rows' means are added in row order and divided by C, then the dot product in
// channel order, the bias and the sigmoid.
__global__ __launch_bounds__(256) void critic_tail_kernel(const float* __restrict__ y4, const float* __restrict__ lw, const float* __restrict__ lb,
                                                          float* __restrict__ score, int C, int T4)
{
    constexpr int O4 = CRITIC_WIDTHS[CRITIC_LAYERS - 1];
    __shared__ float sp[8][O4];
    const int o = threadIdx.x & (O4 - 1), g = threadIdx.x >> 5;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        float v = 0.f;
        for (int t = g; t < T4; t += 8) v += y4[((size_t)c * O4 + o) * T4 + t];
        sp[g][o] = v;
        __syncthreads();
        if (g == 0) {
            float m = sp[0][o];
            for (int k = 1; k < 8; ++k) m += sp[k][o];
            acc += m / (float)T4;
        }
        __syncthreads();
    }
    if (g == 0) sp[0][o] = acc / (float)C;
    __syncthreads();
    if (threadIdx.x == 0) {
        float z = 0.f;
        for (int k = 0; k < O4; ++k) z += sp[0][k] * lw[k];
        z += lb[0];
        score[0] = 1.f / (1.f + __expf(-z));
    }
}

__global__ __launch_bounds__(256) void critic_planar_kernel(const float* __restrict__ x, float* __restrict__ out, int I, int T, size_t n)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int t = (int)(idx % T);
    const size_t ci = idx / T;
    const int i = (int)(ci % I);
    out[idx] = x[((ci - i) + csc_channel_row(I, i, CSC_ORDER_INTERLEAVED)) * T + t];
}

// critic_tail_kernel per clip of a padded batch: workgroup c reads rows clips[c].row0 .. + rows of y4 [R][32][T4max], the frames below the
// clip's own T4, in the same fixed order, and writes scores[c].
__global__ __launch_bounds__(256) void critic_tail_ragged_kernel(const float* __restrict__ y4, const float* __restrict__ lw, const float* __restrict__ lb,
                                                                 float* __restrict__ scores, const CrgClip* __restrict__ clips, int T4max)
{
    constexpr int O4 = CRITIC_WIDTHS[CRITIC_LAYERS - 1];
    __shared__ float sp[8][O4];
    const CrgClip cl = clips[blockIdx.x];
    const int C = cl.rows, T4 = crg_t4(cl.frames);
    const int o = threadIdx.x & (O4 - 1), g = threadIdx.x >> 5;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        float v = 0.f;
        for (int t = g; t < T4; t += 8) v += y4[((size_t)(cl.row0 + c) * O4 + o) * T4max + t];
        sp[g][o] = v;
        __syncthreads();
        if (g == 0) {
            float m = sp[0][o];
            for (int k = 1; k < 8; ++k) m += sp[k][o];
            acc += m / (float)T4;
        }
        __syncthreads();
    }
    if (g == 0) sp[0][o] = acc / (float)C;
    __syncthreads();
    if (threadIdx.x == 0) {
        float z = 0.f;
        for (int k = 0; k < O4; ++k) z += sp[0][k] * lw[k];
        z += lb[0];
        scores[blockIdx.x] = 1.f / (1.f + __expf(-z));
    }
}

// critic_planar_kernel on a padded batch: zeros behind a row's frames, whatever x holds there
__global__ __launch_bounds__(256) void critic_planar_ragged_kernel(const float* __restrict__ x, float* __restrict__ out, int I, int T, size_t n,
                                                                   const CrgRow* __restrict__ rows)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int t = (int)(idx % T);
    const size_t ci = idx / T;
    const int i = (int)(ci % I);
    out[idx] = t < rows[ci / I].frames ? x[((ci - i) + csc_channel_row(I, i, CSC_ORDER_INTERLEAVED)) * T + t] : 0.f;
}

}  // namespace

void launch_critic_commit(const float* w, void* image, unsigned* wmax, int I, hipStream_t s)
{
    const int64_t units = csc_image_halves(I) / 8;
    hipLaunchKernelGGL(critic_commit_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, w, (_Float16*)image, wmax, I, units);
}

void launch_critic_first_h2(const float* x, const void* image, const float* bias, float* y1, float* part, int* range_flag, const CscPlan& p,
                            int x_order, hipStream_t s)
{
    const int inner_n = p.C * p.t_tiles, groups = p.slabs * p.o_tiles;
    const size_t grid = (size_t)8 * ((groups + 7) / 8) * inner_n, n = (size_t)p.C * CSC_O * p.len[0];
    hipLaunchKernelGGL(critic_fwd_h2_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, x, (const _Float16*)image, part, range_flag, p, x_order,
                       (const CrgRow*)nullptr);
    hipLaunchKernelGGL(critic_h2_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, bias, y1, n, p.len[0], p.slabs);
}

// The same two launches on a padded batch: p is the rectangle's plan (C = R rows of T = Tmax frames).  The finish runs over the rectangle;
// what it writes behind a row's T1_r is unspecified (critic_ragged_host.h).
void launch_critic_first_h2_ragged(const float* x, const void* image, const float* bias, float* y1, float* part, int* range_flag, const CscPlan& p,
                                   int x_order, const CrgRow* rows, hipStream_t s)
{
    const int inner_n = p.C * p.t_tiles, groups = p.slabs * p.o_tiles;
    const size_t grid = (size_t)8 * ((groups + 7) / 8) * inner_n, n = (size_t)p.C * CSC_O * p.len[0];
    hipLaunchKernelGGL(critic_fwd_h2_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, x, (const _Float16*)image, part, range_flag, p, x_order, rows);
    hipLaunchKernelGGL(critic_h2_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, bias, y1, n, p.len[0], p.slabs);
}

void launch_critic_tail(const float* y4, const float* lin_w, const float* lin_b, float* score, int C, int T4, hipStream_t s)
{
    hipLaunchKernelGGL(critic_tail_kernel, dim3(1), dim3(256), 0, s, y4, lin_w, lin_b, score, C, T4);
}

void launch_critic_planar(const float* x, float* out, int C, int I, int T, hipStream_t s)
{
    const size_t n = (size_t)C * I * T;
    hipLaunchKernelGGL(critic_planar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, I, T, n);
}

void launch_critic_tail_ragged(const float* y4, const float* lin_w, const float* lin_b, float* scores, const CrgClip* clips, int n_clips, int T4max,
                               hipStream_t s)
{
    hipLaunchKernelGGL(critic_tail_ragged_kernel, dim3((unsigned)n_clips), dim3(256), 0, s, y4, lin_w, lin_b, scores, clips, T4max);
}

void launch_critic_planar_ragged(const float* x, float* out, int R, int I, int Tmax, const CrgRow* rows, hipStream_t s)
{
    const size_t n = (size_t)R * I * Tmax;
    hipLaunchKernelGGL(critic_planar_ragged_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, I, Tmax, n, rows);
}

}  // namespace bsrnn
