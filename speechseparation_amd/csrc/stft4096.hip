// The critic's 4096-point analysis (bsrnn_critic_spectrum; the definition, the slab rule and every size: critic_spectrum_host.h).
//
// One 256-thread workgroup transforms CS_CHUNK consecutive frames of one row, like stft_walk of fft.hip.  The real 4096-point transform
// is a complex 2048-point Stockham FFT (2048 = 2 * 4^5) plus the real split: the radix-2 pass comes first (no twiddles) and runs in
// registers on the windowed samples - the thread that owns complex sample c also owns c + 1024 - and five radix-4 passes follow in LDS,
// two butterflies per thread and pass, between two 16 KB buffers.  Frames overlap by three quarters: the scaled samples stay in
// registers and only the new 1024 are loaded per frame, requested before the passes of the current frame.  Twiddles, split twiddles and
// window come from tables built in double on the host (api_critic.hip) and are fetched before the first frame.  The spectra leave as
// frame-major records of 4098 floats; spectrum_transpose_kernel moves them into the planar [R][4098][T] the critic reads.
// Built like fft.hip without the SLP vectorizer (csrc/Makefile); no atomics, no scratch memory.
#include "kernels.h"

namespace bsrnn {

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

constexpr int CPTS = CS_NFFT / 2;                     // 2048 complex points
constexpr int OWN = CPTS / 256;                       // 8 complex samples per thread: c = tid + 256 k
constexpr int FRESH = CS_HOP / 2 / 256;               // 2 of them are new per frame

// Twiddles of the five radix-4 passes (p = 2, 8, 32, 128, 512 points transformed so far): w_{4p}^{m k}, m = 1..3, k = j & (p - 1) for
// butterfly j.  A thread's two butterflies j = tid, tid + 256 share k in the first four passes.
struct Twiddles { float2 t[4][3]; float2 last[2][3]; };
__device__ __forceinline__ Twiddles load_twiddles(const float2* __restrict__ tw, int tid)
{
    Twiddles r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = 2 << (2 * q);
        const int k = tid & (p - 1);
#pragma unroll
        for (int m = 0; m < 3; ++m) r.t[q][m] = tw[(m + 1) * k * (512 / p)];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int m = 0; m < 3; ++m) r.last[h][m] = tw[(m + 1) * (tid + 256 * h)];
    return r;
}

// One radix-4 Stockham pass over 2048 points: butterflies j = tid, tid + 256
template <int P>
__device__ __forceinline__ void pass4(const float2* src, float2* dst, const float2 (&ta)[3], const float2 (&tb)[3], int tid)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        // one butterfly after the other: interleaved, the two need 5 registers more than the 128 of four workgroups per CU (spilled)
        if (h) __builtin_amdgcn_sched_barrier(0);
        const int j = tid + 256 * h;
        const int k = j & (P - 1);
        const int jo = ((j - k) << 2) + k;
        const float2(&t)[3] = h ? tb : ta;
        const float2 u0 = src[j];
        const float2 u1 = cmul(src[j + 512], t[0]), u2 = cmul(src[j + 1024], t[1]), u3 = cmul(src[j + 1536], t[2]);
        const float2 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), d = csub(u1, u3);
        const float2 v3 = make_float2(d.y, -d.x);                      // -i * d
        dst[jo] = cadd(v0, v2);
        dst[jo + P] = cadd(v1, v3);
        dst[jo + 2 * P] = csub(v0, v2);
        dst[jo + 3 * P] = csub(v1, v3);
    }
    __syncthreads();
}

// Scaled complex sample c (0..2047) of frame t: clip samples cs_sample(t, 2c), cs_sample(t, 2c + 1), each times `scale` (the product
// torch.stft(w * scale) rounds first).  Scalar loads: a reflected pair runs backwards, and rows need not be 8-byte aligned.
__device__ __forceinline__ float2 scaled_sample2(const float* __restrict__ src, int64_t n, float scale, int t, int c)
{
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        int64_t idx = (int64_t)t * CS_HOP + 2 * c + e - CS_NFFT / 2;
        if (idx < 0) idx = -idx;
        if (idx >= n) idx = 2 * (n - 1) - idx;
        v[e] = src[idx] * scale;
    }
    return make_float2(v[0], v[1]);
}

}  // namespace

constexpr int CS_OCC = 4;           // waves per SIMD (= workgroups per CU) the transform is compiled for: 32 KB of LDS each

// grid (chunks of the slab, rows of the slab); rec: the slab's records, row-local frame-major
__global__ __launch_bounds__(256, CS_OCC) void spectrum4096_kernel(CsTables tb, const float* __restrict__ wave, int64_t stride, int64_t n, float scale,
                                                                   float* __restrict__ rec, CsSlab q)
{
    __shared__ __attribute__((aligned(16))) float2 z0[CPTS], z1[CPTS];
    const int tid = threadIdx.x;
    const int t0 = q.t0 + blockIdx.x * CS_CHUNK;
    const int t1 = t0 + CS_CHUNK < q.t1 ? t0 + CS_CHUNK : q.t1;
    const float* src = wave + (size_t)(q.r0 + blockIdx.y) * stride;
    float* out = rec + ((size_t)blockIdx.y * (q.t1 - q.t0) + (t0 - q.t0)) * CS_CHANNELS;

    const Twiddles twd = load_twiddles(tb.tw, tid);
    float2 stw[OWN + 1];            // split twiddles of bins tid + 256 i, and of bin 2048
#pragma unroll
    for (int i = 0; i <= OWN; ++i) stw[i] = tb.split[i < OWN ? tid + 256 * i : CPTS];
    float2 win[OWN], raw[OWN];
#pragma unroll
    for (int k = 0; k < OWN; ++k) {
        const int c = tid + 256 * k;
        win[k] = make_float2(tb.hann[2 * c], tb.hann[2 * c + 1]);
        raw[k] = scaled_sample2(src, n, scale, t0, c);
    }
    for (int t = t0; t < t1; ++t, out += CS_CHANNELS) {
        // window, and the radix-2 pass on the pairs (c, c + 1024): points 2c and 2c + 1 of the pass's output
#pragma unroll
        for (int k = 0; k < OWN / 2; ++k) {
            const float2 a = make_float2(raw[k].x * win[k].x, raw[k].y * win[k].y);
            const float2 b = make_float2(raw[k + 4].x * win[k + 4].x, raw[k + 4].y * win[k + 4].y);
            const float2 s = cadd(a, b), d = csub(a, b);
            *reinterpret_cast<float4*>(&z0[2 * (tid + 256 * k)]) = make_float4(s.x, s.y, d.x, d.y);
        }
        __syncthreads();            // (also: every thread has read the previous frame's spectrum out of z1)
#pragma unroll
        for (int k = 0; k < OWN - FRESH; ++k) raw[k] = raw[k + FRESH];
        {   // the next frame's new quarter (no branch: after the last frame a dummy reload)
            const int tn = t + 1 < t1 ? t + 1 : t;
#pragma unroll
            for (int k = OWN - FRESH; k < OWN; ++k) raw[k] = scaled_sample2(src, n, scale, tn, tid + 256 * k);
        }
        pass4<2>(z0, z1, twd.t[0], twd.t[0], tid);
        pass4<8>(z1, z0, twd.t[1], twd.t[1], tid);
        pass4<32>(z0, z1, twd.t[2], twd.t[2], tid);
        pass4<128>(z1, z0, twd.t[3], twd.t[3], tid);
        pass4<512>(z0, z1, twd.last[0], twd.last[1], tid);
        // real split: X[k] = E[k] + w_4096^k O[k] from Z = z1.  Every thread stores bin 2048 (the same value to the same address): no
        // branch around a store, as in rfft_split_store of fft.hip.
#pragma unroll
        for (int i = 0; i <= OWN; ++i) {
            const int k = i < OWN ? tid + 256 * i : CPTS;
            const float2 zk = z1[k & (CPTS - 1)];
            const float2 zr = z1[(CPTS - k) & (CPTS - 1)];
            const float2 zc = make_float2(zr.x, -zr.y);
            const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
            const float2 dd = csub(zk, zc);                               // (zk - zc) / (2i)
            const float2 o = make_float2(0.5f * dd.y, -0.5f * dd.x);
            float2 x = cadd(e, cmul(stw[i], o));
            if (k == 0 || k == CPTS) x.y = 0.f;                           // exactly real for real input
            *reinterpret_cast<float2*>(out + 2 * k) = x;
        }
    }
}

// rec [rows][nt][2049] (re, im) -> x[(r0 + row)][b][t0 + t] = re, x[..][2049 + b][..] = im.  grid (frame tiles, bin tiles, rows); a tile of
// CS_TILE_B bins x CS_TILE_T frames goes through LDS: read with the bins along the wave (512 contiguous bytes per frame), written with the
// frames along the half-wave (128 contiguous bytes per row of x).
__global__ __launch_bounds__(256) void spectrum_transpose_kernel(const float* __restrict__ rec, float* __restrict__ x, int T, CsSlab q)
{
    __shared__ float re[CS_TILE_B][CS_TILE_T + 1], im[CS_TILE_B][CS_TILE_T + 1];
    const int nt = q.t1 - q.t0;
    const int f0 = blockIdx.x * CS_TILE_T, b0 = blockIdx.y * CS_TILE_B, row = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* in = rec + ((size_t)row * nt + f0) * CS_CHANNELS;
    if (b0 + lane < CS_BINS)
        for (int f = wave; f < CS_TILE_T && f0 + f < nt; f += 4) {
            const float2 v = *reinterpret_cast<const float2*>(in + (size_t)f * CS_CHANNELS + 2 * (b0 + lane));
            re[lane][f] = v.x;
            im[lane][f] = v.y;
        }
    __syncthreads();
    const int f = tid & (CS_TILE_T - 1);
    float* o = x + (size_t)(q.r0 + row) * CS_CHANNELS * T + q.t0 + f0 + f;
    if (f0 + f < nt)
        for (int b = tid / CS_TILE_T; b < CS_TILE_B && b0 + b < CS_BINS; b += 256 / CS_TILE_T) {
            o[(size_t)(b0 + b) * T] = re[b][f];
            o[(size_t)(CS_BINS + b0 + b) * T] = im[b][f];
        }
}

void launch_critic_spectrum_slab(const CsTables& tb, const float* wave, int64_t stride, int64_t n, float scale, float* scratch, float* x, int T,
                                 const CsSlab& q, hipStream_t s)
{
    const int rows = q.r1 - q.r0, nt = q.t1 - q.t0;
    hipLaunchKernelGGL(spectrum4096_kernel, dim3((nt + CS_CHUNK - 1) / CS_CHUNK, rows), dim3(256), 0, s, tb, wave, stride, n, scale, scratch, q);
    hipLaunchKernelGGL(spectrum_transpose_kernel, dim3((nt + CS_TILE_T - 1) / CS_TILE_T, (CS_BINS + CS_TILE_B - 1) / CS_TILE_B, rows), dim3(256), 0, s,
                       scratch, x, T, q);
}

}  // namespace bsrnn
