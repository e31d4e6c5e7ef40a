// The committed critic's gradient (bsrnn_critic_enable_grad / _score_grad / _layer1_dx; the second image, the tiling, the workspace and the
// order of every sum: critic_grad_host.h).
//   critic_grad_commit_kernel  W [1024][I][16] fp32 -> the fp16x2 dx image: the same two pieces as the forward's, in the A-fragment order of
//                              the product over o (16-byte units of 8 consecutive output channels).
//   critic_tail_grad_kernel    d score / d y4 through the sigmoid, Linear(32, 1), the mean over the rows and the mean over time, times the
//                              upstream scalar: 32 values (the pooled gradient), broadcast into dp4 [C][32][T4].  Plain fp32, fixed order.
//   critic_dp_max_kernel       dp = dy * act'(y) (or a plain read of dp) and max |dp| as an integer maximum of bit patterns: order-free.
//   critic_dx_h2_kernel        layer 1's dx as M = (i, k), N = t, K = o on v_mfma_f32_32x32x16_f16, three terms (gemm.hip, Piece<2>): a tile
//                              of 8 channels x 16 taps by 128 frames of one row per workgroup over the whole K = 1024, four waves as
//                              2 (m) x 2 (t).  Per stage of 32 output channels 16 KB of the image are copied to LDS as they lie; dp1 [o][t]
//                              goes to LDS as [o block][piece][o octet h][t][8 o]: the lane that stages (t, octet) loads its 8 floats (each
//                              load coalesced along t across the wave), scales them by the power of two that puts max |dp1| into
//                              [2^14, 2^15), splits them and writes ONE aligned 16-byte unit per piece, so that every B fragment is one
//                              aligned ds_read_b128.  Two LDS stages, one barrier per stage, the next stage loaded behind and split
//                              between the current stage's MFMAs, as in critic_fwd_h2_kernel.  G = hi + 2^-11 lo then goes through LDS
//                              (the stages' 64 KB) and is folded into the 369 input positions the tile completes, taps in tap order, the
//                              result multiplied by the inverse power of two and written at the row the channel map names.
//   critic_scatter_kernel      a planar dx written into the separator's interleaved order (the exact chain's way back).
//   critic_tail_grad_ragged_kernel, critic_dp_max_rows_kernel, critic_dx_h2_kernel<true>   the same three on a padded batch
//                              (bsrnn_critic_score_grad_ragged; critic_ragged_host.h): the tail's gradient per clip with zeros behind a row's
//                              T4_r, the maximum and with it the scale PER CLIP, dead position tiles written as zeros without staging.
// No atomics except the order-free integer max; no kernel here uses scratch memory.
#include "kernels.h"

namespace bsrnn {

typedef float v16f __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int KSTEPS = CGD_STAGE_O / CGD_KB;                     // MFMA K steps per stage: 2
constexpr int ST_A = KSTEPS * CSC_BLOCK;                         // halves of a stage's weight blocks: 8192
constexpr int ST_BP = 2 * CGD_TILE_T * 8;                        // halves of one piece of one K step of dp1: [h][t][8]
constexpr int ST_B = KSTEPS * 2 * ST_BP;                         // 8192
constexpr int STAGE = ST_A + ST_B;                               // 32 KB
constexpr int SG_LD = CGD_TILE_T;                                // the folded product: 128 rows of 128 floats, exactly the two stages
static_assert(ST_A == 256 * 4 * 8, "four 16-byte units of the image per thread and stage");
static_assert(CGD_TILE_T * 2 == 256, "one (t, octet) unit per thread and K step");
static_assert(CGD_CH * CRITIC_TAPS * SG_LD * 4 == 2 * STAGE * 2, "the folded product fits the two stages");
static_assert(cgd_fold_column(CGD_TILE_S - 1, (CGD_TILE_S - 1) % 3) == CGD_TILE_T - 1 && cgd_fold_column(0, 15) == 0, "the halo");

__device__ __forceinline__ void split8(const float (&a)[8], h8& p0, h8& p1)
{
#pragma unroll
    for (int j = 0; j < 8; ++j) p0[j] = (_Float16)a[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) p1[j] = (_Float16)__builtin_fmaf(-(float)p0[j], 2048.f, a[j] * 2048.f);
}

// column t of row m of the folded product: rotated by 11 m so that the fold's reads (three rows, a column every third position) spread
// over the banks
__device__ __forceinline__ int sg_at(int m, int t) { return m * SG_LD + ((t + 11 * m) & (SG_LD - 1)); }

__global__ __launch_bounds__(256) void critic_grad_commit_kernel(const float* __restrict__ w, _Float16* __restrict__ img, int I, int64_t units)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    int o, i, k, piece;
    h8 p0 = {}, p1 = {};
    if (cgd_image_source(I, 8 * u, &o, &i, &k, &piece)) {
        float a[8];
        const float* src = w + ((size_t)o * I + i) * CRITIC_TAPS + k;          // o is a multiple of 8: the unit's eight output channels
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = src[(size_t)j * I * CRITIC_TAPS];
        split8(a, p0, p1);
    }
    *reinterpret_cast<h8*>(img + 8 * u) = piece == 0 ? p0 : p1;
}

// One workgroup of 32 threads' worth of work: gp[o] = ((g * s (1 - s)) * lw[o] / C) / T4, the order autograd takes (sigmoid, Linear, the
// mean over the rows, the mean over time); then dp4[c][o][t] = gp[o] (the last layer has no activation).
__global__ __launch_bounds__(256) void critic_tail_grad_kernel(const float* __restrict__ score, const float* __restrict__ lw,
                                                               const float* __restrict__ gscale, float* __restrict__ gp, float* __restrict__ dp4,
                                                               int C, int T4)
{
    constexpr int O4 = CRITIC_WIDTHS[CRITIC_LAYERS - 1];
    __shared__ float sp[O4];
    if (threadIdx.x < O4) {
        const float s = score[0], g = gscale ? gscale[0] : 1.f;
        const float dz = g * ((1.f - s) * s);
        const float v = ((dz * lw[threadIdx.x]) / (float)C) / (float)T4;
        sp[threadIdx.x] = v;
        gp[threadIdx.x] = v;
    }
    __syncthreads();
    const int n = C * O4 * T4;
    for (int idx = threadIdx.x; idx < n; idx += 256) dp4[idx] = sp[(idx / T4) % O4];
}

// dp = y ? dy * act'(y) : dy (slope 0.01 where y <= 0, critic_dp_kernel's convention), written when dp is not null; *mx = max over the
// bit patterns of |dp| (NaN bits order above infinity).  dy and dp may be the same array.
__global__ __launch_bounds__(256) void critic_dp_max_kernel(const float* dy, const float* __restrict__ y, float* dp, unsigned* __restrict__ mx, size_t n)
{
    __shared__ unsigned smax[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned m = 0;
    if (i < n) {
        float gr = dy[i];
        if (y) gr = y[i] > 0.f ? gr : 0.01f * gr;
        if (dp) dp[i] = gr;
        m = __float_as_uint(gr) & 0x7fffffffu;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned v = __shfl_xor(m, d); m = v > m ? v : m; }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        if (m) atomicMax(mx, m);
    }
}

// RAGGED (bsrnn_critic_score_grad_ragged; critic_ragged_host.h): row c holds rows[c].frames <= T frames and reads the max word of ITS
// clip, mx[rows[c].clip]; a position tile wholly at or behind the row's frames writes zeros before it stages anything, and a live one
// writes zeros at the positions behind them, so every s < T of every row is written.
template <bool RAGGED>
__global__ __launch_bounds__(256, 2) void critic_dx_h2_kernel(const float* __restrict__ dp, const _Float16* __restrict__ img, float* __restrict__ dx,
                                                              const unsigned* __restrict__ mx, int* range_flag, CgdPlan g, int x_order,
                                                              const CrgRow* __restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) _Float16 sm[2 * STAGE];
    // The tiles (c, position tile) of one channel tile read the same weight blocks: they sit on consecutive workgroups of one XCD (speed only)
    const int inner_n = g.f.C * g.s_tiles;
    const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
    const int inner = q % inner_n, bi = (q / inner_n) * 8 + xcd;
    if (bi >= g.i_tiles) return;
    const int bs = inner % g.s_tiles, c = inner / g.s_tiles;
    const int I = g.f.I, T = g.f.T, T1 = g.f.len[0];
    const int t_lo = cgd_tile_frame0(bs), s0 = cgd_tile_first(bs), i0 = bi * CGD_CH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, half = lane >> 5, r32 = lane & 31;

    int Tr = T, T1r = T1;                                    // the row's own frames, in front of and behind the layer (T and T1 stay the strides)
    unsigned mbits;
    if constexpr (RAGGED) {
        const CrgRow row = rows[c];
        Tr = row.frames; T1r = crg_t_out(Tr);
        mbits = mx[row.clip];
    } else {
        mbits = mx[0];
    }
    const int e = cgd_scale_exponent(mbits);
    if (mbits >= 0x7f800000u && range_flag && tid == 0) *range_flag = 1;       // a non-finite dp1: the guard, as for an |x| beyond fp16
    if constexpr (RAGGED) {
        if (s0 >= Tr) {
            for (int idx = tid; idx < CGD_CH * CGD_TILE_S; idx += 256) {
                const int ch = idx / CGD_TILE_S, s = s0 + (idx - ch * CGD_TILE_S);
                if (i0 + ch < I && s < T) dx[((size_t)c * I + csc_channel_row(I, i0 + ch, x_order)) * T + s] = 0.f;
            }
            return;
        }
    }

    // staging: four 16-byte units of the stage's 16 KB of the image, and the unit (t = tid & 127, octet = tid >> 7) of both K steps
    const _Float16* const a_src = img + (size_t)bi * (CSC_O / CGD_KB) * CSC_BLOCK + 8 * tid;
    const int st = tid & (CGD_TILE_T - 1), sh = tid >> 7;
    const bool t_in = t_lo + st >= 0 && t_lo + st < T1r;
    // (a lane's offset is small and the same for every load; the row (c, o) in front of it is uniform)
    const unsigned d_off = (unsigned)(8 * sh * T1 + (t_in ? t_lo + st : 0));
    const float* const d_row = dp + (size_t)c * CSC_O * T1;
    h8 ra[4];
    float rd[KSTEPS][8];
    auto gload = [&](int o0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) ra[r] = *reinterpret_cast<const h8*>(a_src + (size_t)(o0 / CGD_KB) * CSC_BLOCK + 2048 * r);
#pragma unroll
        for (int r = 0; r < KSTEPS; ++r) {
            if (t_in) {
#pragma unroll
                for (int j = 0; j < 8; ++j) rd[r][j] = (d_row + (size_t)(o0 + CGD_KB * r + j) * T1)[d_off];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) rd[r][j] = 0.f;
            }
        }
    };
    auto put_a = [&](_Float16* stg) {
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<h8*>(stg + 8 * tid + 2048 * r) = ra[r];
    };
    auto put_d = [&](_Float16* stg) {
#pragma unroll
        for (int r = 0; r < KSTEPS; ++r) {
#pragma unroll
            for (int j = 0; j < 8; ++j) rd[r][j] = __builtin_ldexpf(rd[r][j], e);
            h8 p0, p1;
            split8(rd[r], p0, p1);
            _Float16* d = stg + ST_A + r * 2 * ST_BP + sh * (CGD_TILE_T * 8) + st * 8;
            *reinterpret_cast<h8*>(d) = p0;
            *reinterpret_cast<h8*>(d + ST_BP) = p1;
        }
    };

    v16f hi[2][2], lo[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) { hi[a][b] = (v16f){0}; lo[a][b] = (v16f){0}; }

    // fragment offsets (halves): A sub-tile 2 wm + s2 of [piece][sub-tile][lane][8]; B lane (t = 64 wn + 32 n2 + r32, octet = half) of [piece][h][t][8]
    const int fa = (2 * wm) * 512 + lane * 8;
    const int fb = ST_A + half * (CGD_TILE_T * 8) + (64 * wn + r32) * 8;

    gload(0);
    put_a(sm);
    put_d(sm);
    gload(CGD_STAGE_O);
    __syncthreads();
    int n = 0;
    for (int o0 = 0; o0 < CSC_O; o0 += CGD_STAGE_O, ++n) {
        const _Float16* const cur = sm + (n & 1) * STAGE;
        _Float16* const nxt = sm + ((n + 1) & 1) * STAGE;
        const bool more = o0 + CGD_STAGE_O < CSC_O;              // the registers hold stage o0 + CGD_STAGE_O
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            h8 a[2][2], b[2][2];
#pragma unroll
            for (int pc = 0; pc < 2; ++pc)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    a[s][pc] = *reinterpret_cast<const h8*>(cur + ks * CSC_BLOCK + pc * (CSC_BLOCK / 2) + fa + s * 512);
                    b[s][pc] = *reinterpret_cast<const h8*>(cur + ks * 2 * ST_BP + pc * ST_BP + fb + s * 256);
                }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    lo[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s][1], b[j][0], lo[s][j], 0, 0, 0);
                    lo[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s][0], b[j][1], lo[s][j], 0, 0, 0);
                    hi[s][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s][0], b[j][0], hi[s][j], 0, 0, 0);
                }
            if (more) {
                if (ks == 0) put_a(nxt);
                else put_d(nxt);
            }
        }
        if (o0 + 2 * CGD_STAGE_O < CSC_O) gload(o0 + 2 * CGD_STAGE_O);
        __syncthreads();
    }

    // C / D layout of the 32x32 MFMA: column (t) = lane & 31, row (m) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The loop's last barrier
    // has passed: nobody reads the stages any more.
    float* const sg = reinterpret_cast<float*>(sm);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t = 64 * wn + 32 * j + r32;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int m = 64 * wm + 32 * s + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                sg[sg_at(m, t)] = hi[s][j][reg] + lo[s][j][reg] * (1.f / 2048.f);
            }
        }
    __syncthreads();
    // position s0 + d takes tap k from column 5 + (d - k) / 3 for k = d % 3, d % 3 + 3, ... (in that order, as critic_dx_kernel adds them)
    for (int idx = tid; idx < CGD_CH * CGD_TILE_S; idx += 256) {
        const int ch = idx / CGD_TILE_S, d = idx - ch * CGD_TILE_S, s = s0 + d;
        if (i0 + ch >= I || s >= T) continue;
        float v = 0.f;
        for (int k = d % CRITIC_STRIDE; k < CRITIC_TAPS; k += CRITIC_STRIDE) v += sg[sg_at(ch * CRITIC_TAPS + k, cgd_fold_column(d, k))];
        if (RAGGED && s >= Tr) v = 0.f;                          // (a sum of products with zeros already: written as a plain zero)
        dx[((size_t)c * I + csc_channel_row(I, i0 + ch, x_order)) * T + s] = __builtin_ldexpf(v, -e);
    }
}

// critic_tail_grad_kernel per clip of a padded batch: workgroup c forms gp[c][o] = ((gscale[c] * s_c (1 - s_c)) * lw[o] / rows_c) / T4_c and
// writes it into dp4 [R][32][T4max] of the clip's rows for t < T4_c, and ZEROS for T4_c <= t < T4max (critic_ragged_host.h: with zeros
// there the exact dx / dp kernels of layers 4 .. 2 run on the rectangle unchanged).
__global__ __launch_bounds__(256) void critic_tail_grad_ragged_kernel(const float* __restrict__ scores, const float* __restrict__ lw,
                                                                      const float* __restrict__ gscale, float* __restrict__ gp, float* __restrict__ dp4,
                                                                      const CrgClip* __restrict__ clips, int T4max)
{
    constexpr int O4 = CRITIC_WIDTHS[CRITIC_LAYERS - 1];
    __shared__ float sp[O4];
    const CrgClip cl = clips[blockIdx.x];
    const int C = cl.rows, T4 = crg_t4(cl.frames);
    if (threadIdx.x < O4) {
        const float s = scores[blockIdx.x], g = gscale ? gscale[blockIdx.x] : 1.f;
        const float dz = g * ((1.f - s) * s);
        const float v = ((dz * lw[threadIdx.x]) / (float)C) / (float)T4;
        sp[threadIdx.x] = v;
        gp[(size_t)blockIdx.x * O4 + threadIdx.x] = v;
    }
    __syncthreads();
    const int n = C * O4 * T4max;
    float* const out = dp4 + (size_t)cl.row0 * O4 * T4max;
    for (int idx = threadIdx.x; idx < n; idx += 256) out[idx] = idx % T4max < T4 ? sp[(idx / T4max) % O4] : 0.f;
}

// critic_dp_max_kernel with the maximum per CLIP: a workgroup covers 256 values of ONE row r (per_row workgroups each) and raises
// mx[rows[r].clip]
__global__ __launch_bounds__(256) void critic_dp_max_rows_kernel(const float* dy, const float* __restrict__ y, float* dp, unsigned* __restrict__ mx,
                                                                 const CrgRow* __restrict__ rows, unsigned n_row, unsigned per_row)
{
    __shared__ unsigned smax[4];
    const unsigned r = blockIdx.x / per_row, j = (blockIdx.x - r * per_row) * 256 + threadIdx.x;
    const size_t i = (size_t)r * n_row + j;
    unsigned m = 0;
    if (j < n_row) {
        float gr = dy[i];
        if (y) gr = y[i] > 0.f ? gr : 0.01f * gr;
        if (dp) dp[i] = gr;
        m = __float_as_uint(gr) & 0x7fffffffu;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned v = __shfl_xor(m, d); m = v > m ? v : m; }
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(smax[0], smax[1]), max(smax[2], smax[3]));
        if (m) atomicMax(mx + rows[r].clip, m);
    }
}

__global__ __launch_bounds__(256) void critic_scatter_kernel(const float* __restrict__ in, float* __restrict__ out, int I, int T, size_t n)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int t = (int)(idx % T);
    const size_t ci = idx / T;
    const int i = (int)(ci % I);
    out[((ci - i) + csc_channel_row(I, i, CSC_ORDER_INTERLEAVED)) * T + t] = in[idx];
}

}  // namespace

void launch_critic_grad_commit(const float* w, void* image, int I, hipStream_t s)
{
    const int64_t units = cgd_image_halves(I) / 8;
    hipLaunchKernelGGL(critic_grad_commit_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, w, (_Float16*)image, I, units);
}

void launch_critic_tail_grad(const float* score, const float* lin_w, const float* gscale, float* gp, float* dp4, int C, int T4, hipStream_t s)
{
    hipLaunchKernelGGL(critic_tail_grad_kernel, dim3(1), dim3(256), 0, s, score, lin_w, gscale, gp, dp4, C, T4);
}

void launch_critic_dp_max(const float* dy, const float* y, float* dp, unsigned* mx, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(critic_dp_max_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dy, y, dp, mx, n);
}

void launch_critic_dx_h2(const float* dp, const void* image, float* dx, const unsigned* mx, int* range_flag, const CgdPlan& g, int x_order,
                         hipStream_t s)
{
    const size_t grid = (size_t)8 * ((g.i_tiles + 7) / 8) * g.f.C * g.s_tiles;
    hipLaunchKernelGGL(critic_dx_h2_kernel<false>, dim3((unsigned)grid), dim3(256), 0, s, dp, (const _Float16*)image, dx, mx, range_flag, g, x_order,
                       (const CrgRow*)nullptr);
}

// On a padded batch: g is the rectangle's plan, mx the clips' max words
void launch_critic_dx_h2_ragged(const float* dp, const void* image, float* dx, const unsigned* mx, int* range_flag, const CgdPlan& g, int x_order,
                                const CrgRow* rows, hipStream_t s)
{
    const size_t grid = (size_t)8 * ((g.i_tiles + 7) / 8) * g.f.C * g.s_tiles;
    hipLaunchKernelGGL(critic_dx_h2_kernel<true>, dim3((unsigned)grid), dim3(256), 0, s, dp, (const _Float16*)image, dx, mx, range_flag, g, x_order, rows);
}

void launch_critic_tail_grad_ragged(const float* scores, const float* lin_w, const float* gscale, float* gp, float* dp4, const CrgClip* clips,
                                    int n_clips, int T4max, hipStream_t s)
{
    hipLaunchKernelGGL(critic_tail_grad_ragged_kernel, dim3((unsigned)n_clips), dim3(256), 0, s, scores, lin_w, gscale, gp, dp4, clips, T4max);
}

void launch_critic_dp_max_rows(const float* dy, const float* y, float* dp, unsigned* mx, const CrgRow* rows, int R, size_t n_row, hipStream_t s)
{
    const unsigned per_row = (unsigned)((n_row + 255) / 256);
    hipLaunchKernelGGL(critic_dp_max_rows_kernel, dim3(per_row * (unsigned)R), dim3(256), 0, s, dy, y, dp, mx, rows, (unsigned)n_row, per_row);
}

void launch_critic_scatter(const float* in, float* out, int C, int I, int T, hipStream_t s)
{
    const size_t n = (size_t)C * I * T;
    hipLaunchKernelGGL(critic_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, I, T, n);
}

}  // namespace bsrnn
