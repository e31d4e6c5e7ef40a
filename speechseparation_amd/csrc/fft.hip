// STFT / iSTFT / layout kernels of the callers' sandwich (infer.py:29-37, m_dataset.py:187-195,
// infer-streaming.py:116-145, speech-ladspa-onnx.cpp:191-261).
//
// One 256-thread workgroup transforms one frame.  The real 2048-point transform is done as a
// complex 1024-point radix-4 Stockham FFT in LDS (5 passes, one radix-4 butterfly per thread
// per pass) plus the real-FFT split/merge step; twiddles and windows come from tables built
// in double precision on the host.  These stages are HBM-bound (4 KiB in, 8.2 KiB out per
// frame); their loads and stores are coalesced along the frame.
#include "kernels.h"
#include <type_traits>

#include <algorithm>
#include <cstdlib>

namespace bsrnn {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }

// In-LDS complex FFT of 1024 points, Stockham autosort radix-4.  z0 holds the input, the
// result ends in the returned buffer.  INV = true computes the unnormalised inverse.
// Twiddles of the four non-trivial passes, fetched once per thread BEFORE the passes start (they
// depend only on the thread index): a global load inside each pass would put an L2 round trip into
// the dependent chain of every pass.
struct Twiddles { float2 t[4][3]; };
template <bool INV>
__device__ __forceinline__ Twiddles load_twiddles(const float2* __restrict__ tw, int tid)
{
    Twiddles r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int p = 4 << (2 * q);                 // 4, 16, 64, 256
        const int k = tid & (p - 1);
        const int step = 256 / p;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float2 t = tw[(m + 1) * k * step];
            if (INV) t = cconj(t);
            r.t[q][m] = t;
        }
    }
    return r;
}

template <bool INV>
__device__ __forceinline__ float2* fft1024(float2* z0, float2* z1, const Twiddles& twd, int tid)
{
    float2* src = z0;
    float2* dst = z1;
#ifdef FFT_ABL_NOPASSES
    __syncthreads();
    return src;
#endif
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int p = 1 << (2 * q);
        const int k = tid & (p - 1);
        const int jo = ((tid - k) << 2) + k;
        float2 u0 = src[tid], u1 = src[tid + 256], u2 = src[tid + 512], u3 = src[tid + 768];
        if (q > 0) {
            u1 = cmul(u1, twd.t[q - 1][0]); u2 = cmul(u2, twd.t[q - 1][1]); u3 = cmul(u3, twd.t[q - 1][2]);
        }
        const float2 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), d = csub(u1, u3);
        const float2 v3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);   // (+i or -i) * d
        dst[jo] = cadd(v0, v2);
        dst[jo + p] = cadd(v1, v3);
        dst[jo + 2 * p] = csub(v0, v2);
        dst[jo + 3 * p] = csub(v1, v3);
        __syncthreads();
        float2* tmp = src; src = dst; dst = tmp;
    }
    return src;
}

// Per-thread slice of the real-FFT split/merge step: bins k = tid + 256 i.  The column map and the
// 2048-point twiddles are fetched up front (before the FFT passes) so that the bin loops below contain no
// dependent global load -> global access chains.
struct SplitCtx {
    int col[5];          // column of bin tid + 256 i   (i = 4 only for tid == 0: bin 1024)
    int colr[4];         // column of bin 1024 - (tid + 256 i)
    float2 tw[5];
};
__device__ __forceinline__ SplitCtx load_split(const FftTables& tb, int tid, bool want_reverse)
{
    SplitCtx c;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int k = i < 4 ? tid + 256 * i : 1024;          // fifth slot: bin 1024, computed and stored by every thread (see rfft_split_store)
        c.col[i] = tb.colmap ? tb.colmap[k] : 2 * k;
        c.tw[i] = tb.tw2048[k];
        if (i < 4) c.colr[i] = want_reverse ? (tb.colmap ? tb.colmap[1024 - k] : 2 * (1024 - k)) : 0;
    }
    return c;
}

// real spectrum X[0..1024] from Z = FFT1024(x[2n] + i x[2n+1]); writes interleaved re/im
__device__ __forceinline__ void rfft_split_store(const float2* Z, const SplitCtx& sc, float* __restrict__ out, int tid)
{
#pragma unroll
    // No branch around a store: with the fifth (Nyquist) store conditional the compiler cannot count the stores in flight and
    // waits for vmcnt(0) - the previous frame's stores included - in front of the next frame's samples.  Every thread stores
    // bin 1024 instead (the same value to the same address).
    for (int i = 0; i < 5; ++i) {
        const int k = i < 4 ? tid + 256 * i : 1024;
        const float2 zk = Z[k & 1023];
        const float2 zc = cconj(Z[(1024 - k) & 1023]);
        const float2 e = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
        const float2 dd = csub(zk, zc);                               // (zk - zc) / (2i)
        const float2 o = make_float2(0.5f * dd.y, -0.5f * dd.x);
        float2 x = cadd(e, cmul(sc.tw[i], o));
        if (k == 0 || k == 1024) x.y = 0.f;                           // exactly real for real input
        *reinterpret_cast<float2*>(out + sc.col[i]) = x;
    }
}

// Z[k] = E[k] + i O[k] for the inverse; imaginary parts of DC / Nyquist are ignored like c2r does.
// `lin` = true: Y is a plain interleaved [2050] row (LDS copy), else columns come from sc.
struct MergeRegs { float2 xk[4], xc[4]; };
template <bool LIN>
__device__ __forceinline__ void irfft_load(const float* __restrict__ Y, const SplitCtx& sc, MergeRegs& r, int tid)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = tid + 256 * i;
        r.xk[i] = *reinterpret_cast<const float2*>(Y + (LIN ? 2 * k : sc.col[i]));
        r.xc[i] = *reinterpret_cast<const float2*>(Y + (LIN ? 2 * (1024 - k) : sc.colr[i]));
    }
}
// PINNED spells out the fused multiply-adds of o = dd * conj(tw) (istft_walk).  Left to the compiler's contraction, which of the two products
// of each component is rounded first depends on the code around the call.
template <bool PINNED = false>
__device__ __forceinline__ void irfft_store(const MergeRegs& r, const SplitCtx& sc, float2* z, int tid)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = tid + 256 * i;
        float2 a = r.xk[i], b = r.xc[i];
        if (k == 0) { a.y = 0.f; b.y = 0.f; }
        b = cconj(b);
        const float2 e = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y + b.y));
        const float2 dd = make_float2(0.5f * (a.x - b.x), 0.5f * (a.y - b.y));
        const float2 t = sc.tw[i];
        const float2 o = PINNED ? make_float2(fmaf(dd.x, t.x, dd.y * t.y), fmaf(dd.y, t.x, -(dd.x * t.y))) : cmul(dd, cconj(t));
        z[k] = make_float2(e.x - o.y, e.y + o.x);                     // e + i*o
    }
}
template <bool LIN>
__device__ __forceinline__ void irfft_merge(const float* __restrict__ Y, const SplitCtx& sc, float2* z, int tid)
{
    MergeRegs r;
    irfft_load<LIN>(Y, sc, r, tid);                                   // all loads first
    irfft_store(r, sc, z, tid);
}

// NOTE: the library is compiled with -fno-slp-vectorize (csrc/Makefile) because of this file.  With the SLP vectorizer the complex butterflies
// become packed-fp32 (v_pk_*) code, and the STFT / iSTFT kernels then returned garbage in whole frames whenever kernels of
// another process or of another stream of this process shared the GPU - always right when alone.  Found with
// tools/row_block_check.py and tests/coresident_check.py; bisected to the FFT passes (not the barriers, the twiddle loads,
// the LDS neighbours or the counted waits) and to the vectorizer (-O1 and -O3 -fno-slp-vectorize are clean, -O2 / -O3 are
// not).  The scalar code is as fast.
//
// Frames per workgroup of the two offline kernels.  All workgroups of a launch cost the same, so a grid slightly larger
// than the chip's resident capacity (CUs x workgroups per CU) runs as two rounds with the second nearly empty: at
// R = 64, T = 126 six frames per workgroup gave 1344 workgroups for 1024 (STFT) / 768 (iSTFT) slots.  The chunk length
// is chosen per launch to minimise rounds x (frames walked per workgroup); small inputs get short chunks (more
// workgroups), `extra` = frames a chunk recomputes (the iSTFT's overlap frame).
static int resident_slots(const void* kernel)
{
    int dev = 0, cus = 256, per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    return cus * per_cu;
}
static int frames_per_workgroup(int units, int rows, int slots, int extra)
{
    int best = 4;
    long best_cost = -1;
    for (int L = 16; L >= 4; --L) {
        const long wgs = (long)((units + L - 1) / L) * rows;
        const long cost = ((wgs + slots - 1) / slots) * (L + extra);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = L; }
    }
    return best;
}
// Chunk length and grid of a chunked launch: ceil(units / chunk) workgroups per row.  One resident-slots value per kernel.
struct Chunks { int len; dim3 grid; };
template <auto KERNEL>
static Chunks chunks_for(int units, int rows, int extra)
{
    static const int slots = resident_slots((const void*)KERNEL);
    const int len = frames_per_workgroup(units, rows, slots, extra);
    return {len, dim3((unsigned)((units + len - 1) / len), rows)};
}

// ------------------------------------------------------------------------------ the two frame walks
// Every chunked STFT kernel (offline, segment, ragged, block streaming) is this walk over frames [t0, t1) of one row plus its own
// sample source, row destination and epilogue, and every windowed iSTFT kernel (offline, segment, ragged) is istft_walk below: a frame
// or a hop that two of them compute has the same bits because it is the same code.
//
// Analysis.  Frames overlap by half: the thread that owns complex samples c + 512, c + 768 of frame t owns c, c + 256 of frame t + 1, so
// only the new half is loaded per frame (requested before the FFT passes of the current frame) and the raw samples stay in registers.
// sample2(t, c) = complex sample c (0..1023) of frame t, row(t) = where the spectrum of frame t goes.  The walk fetches the twiddle and split
// tables itself (passed in from the kernel, the counted vmcnt(28) wait in front of the loop became a vmcnt(0) in front of the sample loads).  Returns the raw second half of
// the last frame (complex samples 512 + tid, 768 + tid).
struct RawHalf { float2 v[2]; };
template <class SAMPLE2, class ROW>
__device__ __forceinline__ RawHalf stft_walk(const FftTables& tb, float2* z0, float2* z1, int tid, int t0, int t1,
                                             SAMPLE2 sample2, ROW row)
{
    const Twiddles twd = load_twiddles<false>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, false);
    float2 win[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) win[k] = make_float2(tb.hann[2 * (tid + 256 * k)], tb.hann[2 * (tid + 256 * k) + 1]);
    float2 raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = sample2(t0, tid + 256 * k);
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) z0[tid + 256 * k] = make_float2(raw[k].x * win[k].x, raw[k].y * win[k].y);
        __syncthreads();
        raw[0] = raw[2]; raw[1] = raw[3];
        { const int tn = t + 1 < t1 ? t + 1 : t; raw[2] = sample2(tn, tid + 512); raw[3] = sample2(tn, tid + 768); }      // (no branch: after the last frame a dummy reload)
        const float2* Z = fft1024<false>(z0, z1, twd, tid);
        rfft_split_store(Z, spl, row(t), tid);
        __syncthreads();                          // Z (= z1) is overwritten by the next frame's first pass
    }
    return {{raw[0], raw[1]}};
}

// Synthesis.  Output hop = first half of a synthesis frame + second half of the frame in front of it, divided by the window envelope
// (torch.istft).  The walk takes frames [a0, a1) of one row, each of which completes one hop, with the windowed second half of the frame
// in front in `carry` (the thread that owns complex samples c, c + 256 of a frame's first half also owns c + 512, c + 768 of the second
// half): recomputed from frame a0 - 1 (`peel`), or as the caller loaded it.  No [M][2048] frame buffer in HBM and no separate overlap-add
// launch (was 132 MB + 15 us).  The spectrum of frame t + 1 is requested before the FFT passes of frame t.  spectrum(t) = the row of
// frame t, hop(t) = where the hop that frame t completes goes.  On return `carry` holds the windowed second half of frame a1 - 1.
template <class SPECTRUM, class HOP>
__device__ __forceinline__ void istft_walk(const FftTables& tb, float2* z0, float2* z1, int tid, int a0, int a1, SPECTRUM spectrum, HOP hop,
                                           bool peel, float2 (&carry)[2])
{
    const Twiddles twd = load_twiddles<true>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, true);
    const float sc = 1.0f / 1024.0f;
    float2 wlo[2], whi[2], env[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = tid + 256 * k;
        wlo[k] = make_float2(tb.hann[2 * c] * sc, tb.hann[2 * c + 1] * sc);
        whi[k] = make_float2(tb.hann[2 * c + HOPS] * sc, tb.hann[2 * c + 1 + HOPS] * sc);
        env[k] = make_float2(tb.inv_env[2 * c], tb.inv_env[2 * c + 1]);
    }
    MergeRegs mr;
    // The frame in front of the range only fills the carry; it is peeled so that the loop body has no branch around its loads and
    // stores (the compiler then counts them and waits for the next spectrum with vmcnt(2) instead of vmcnt(0), stores included).
    auto frame = [&](int t, auto first) {
        irfft_store<true>(mr, spl, z0, tid);
        __syncthreads();
        irfft_load<false>(spectrum(t + 1 < a1 ? t + 1 : t), spl, mr, tid);      // (after the last frame: a dummy reload)
        const float2* z = fft1024<true>(z0, z1, twd, tid);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = tid + 256 * k;
            const float2 a = z[c], b = z[c + 512];
            if (!decltype(first)::value) {
                // (frame * 1/1024 * window) summed, then / envelope.  The fused multiply-add is spelled out: left to the compiler's
                // contraction, it is free to round the other product (a * wlo instead of the carry), and has done so
                const float2 v = make_float2(fmaf(a.x, wlo[k].x, carry[k].x) * env[k].x, fmaf(a.y, wlo[k].y, carry[k].y) * env[k].y);
                *reinterpret_cast<float2*>(hop(t) + 2 * c) = v;
            }
            carry[k] = make_float2(b.x * whi[k].x, b.y * whi[k].y);
        }
        __syncthreads();                          // z (= z1) is overwritten by the next frame's first pass
    };
    irfft_load<false>(spectrum(peel ? a0 - 1 : a0), spl, mr, tid);
    if (peel) frame(a0 - 1, std::true_type());
    for (int t = a0; t < a1; ++t) frame(t, std::false_type());
}

// Complex sample c (0..1023) of frame t of a clip of n samples: padded frame sample i (0..2047) is clip sample t*1024 + i - 1024, reflected
// at both ends.  `src` points at clip sample `base` (subtracted after the reflection).
__device__ __forceinline__ float2 reflected_sample2(const float* __restrict__ src, int64_t n, int64_t base, int t, int c)
{
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        int64_t idx = (int64_t)t * HOPS + 2 * c + e - NFFT / 2;
        if (idx < 0) idx = -idx;
        if (idx >= n) idx = 2 * (n - 1) - idx;
        v[e] = src[idx - base];
    }
    return make_float2(v[0], v[1]);
}

// ------------------------------------------------------------------------------ offline STFT
// One workgroup transforms `sch` consecutive frames of one row (stft_walk).
constexpr int FFT_OCC_STFT = 4;     // waves per SIMD (= workgroups per CU) the offline STFT is compiled for
constexpr int FFT_OCC_ISTFT = 4;    // ... and the offline iSTFT
template <bool ZERO_PAD>      // ZERO_PAD: samples outside [0, n) are zeros instead of reflections (the adjoint of the iSTFT, below)
__global__ __launch_bounds__(256, FFT_OCC_STFT) void stft_kernel(FftTables tb, const float* __restrict__ wave, float* __restrict__ X,
                                                   int64_t n, int T, int sch)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int t0 = blockIdx.x * sch;
    const int t1 = (t0 + sch < T) ? t0 + sch : T;
    const float* src = wave + (size_t)r * n;
    auto sample2 = [&](int t, int c) {
        if (!ZERO_PAD) return reflected_sample2(src, n, 0, t, c);
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t idx = (int64_t)t * HOPS + 2 * c + e - NFFT / 2;
            v[e] = (idx >= 0 && idx < n) ? src[idx] : 0.f;
        }
        return make_float2(v[0], v[1]);
    };
    auto row = [&](int t) { return X + ((size_t)r * T + t) * tb.ld; };
    stft_walk(tb, z0, z1, tid, t0, t1, sample2, row);
}

void launch_stft(const FftTables& tb, const float* wave, float* X, int R, int64_t n, int T, hipStream_t s)
{
    const Chunks ch = chunks_for<stft_kernel<false>>(T, R, 0);
    hipLaunchKernelGGL(stft_kernel<false>, ch.grid, dim3(256), 0, s, tb, wave, X, n, T, ch.len);
}

// ------------------------------------------------------------------------------ backward of the offline iSTFT (training step)
// torch.istft (infer.py:35-37 / m_dataset.py:192-195) is linear in the spectrum: wave[n] = (1 / env[n]) sum_t w[j] irfft(Y_t)[j],
// j = n + 1024 - 1024 t, env = sum of squared windows (two frames cover every kept sample).  Its transpose, applied to the
// loss gradient g of the waveform, is an STFT of g / env with ZERO padding (the trimmed ends carry no gradient) whose bins
// are scaled by c_k / 2048, c_0 = c_1024 = 1, else 2 (a one-sided bin stands for itself and its mirror), and the imaginary
// parts of bins 0 and 1024 (which irfft ignores) get no gradient.  dwave [R][(T-1) 1024] -> dY frame-major [R T][ld].
__global__ void istft_bwd_prescale_kernel(FftTables tb, const float* __restrict__ dwave, float* __restrict__ g, size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % HOPS);                       // rows are multiples of 1024 long
    const float w0 = tb.hann[j], w1 = tb.hann[j + HOPS];
    g[i] = dwave[i] / (w0 * w0 + w1 * w1);
}
__global__ void istft_bwd_postscale_kernel(FftTables tb, float* __restrict__ X, size_t rows)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * NBINS) return;
    const size_t row = i / NBINS;
    const int k = (int)(i % NBINS);
    float* p = X + row * tb.ld + tb.colmap[k];
    const bool edge = k == 0 || k == NBINS - 1;
    const float sc = (edge ? 1.0f : 2.0f) / (float)NFFT;
    p[0] *= sc;
    p[1] = edge ? 0.f : p[1] * sc;
}
void launch_istft_backward(const FftTables& tb, const float* dwave, float* scratch, float* dY, int R, int T, hipStream_t s)
{
    if (T < 2) return;
    const int64_t n = (int64_t)(T - 1) * HOPS;
    const size_t total = (size_t)R * n;
    hipLaunchKernelGGL(istft_bwd_prescale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, tb, dwave, scratch, total);
    const Chunks ch = chunks_for<stft_kernel<true>>(T, R, 0);
    hipLaunchKernelGGL(stft_kernel<true>, ch.grid, dim3(256), 0, s, tb, scratch, dY, n, T, ch.len);
    const size_t rows = (size_t)R * T;
    hipLaunchKernelGGL(istft_bwd_postscale_kernel, dim3((unsigned)((rows * NBINS + 255) / 256)), dim3(256), 0, s, tb, dY, rows);
}

// ------------------------------------------------------------------------------ offline iSTFT
// One workgroup produces `ich` consecutive output hops of one row: output hop b = first half of synthesis frame b + 1 + second half of
// frame b.  The workgroup walks frames b0 .. b0 + ich (istft_walk) and recomputes one frame per chunk.
__global__ __launch_bounds__(256, FFT_OCC_ISTFT) void istft_fused_kernel(FftTables tb, const float* __restrict__ Y, float* __restrict__ out, int T, int ich)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int b0 = blockIdx.x * ich;
    const int b1 = (b0 + ich < T - 1) ? b0 + ich : T - 1;          // output hops [b0, b1) <- frames b0 .. b1
    const float* Yr = Y + (size_t)r * T * tb.ld;
    float* o = out + (size_t)r * (T - 1) * HOPS;
    auto spectrum = [&](int t) { return Yr + (size_t)t * tb.ld; };
    auto hop = [&](int t) { return o + (size_t)(t - 1) * HOPS; };
    float2 carry[2];
    istft_walk(tb, z0, z1, tid, b0 + 1, b1 + 1, spectrum, hop, true, carry);
}

void launch_istft(const FftTables& tb, const float* Y, float* out, int R, int T, hipStream_t s)
{
    if (T < 2) return;
    const Chunks ch = chunks_for<istft_fused_kernel>(T - 1, R, 1);
    hipLaunchKernelGGL(istft_fused_kernel, ch.grid, dim3(256), 0, s, tb, Y, out, T, ch.len);
}

// ------------------------------------------------------------------------------ [C][2050][T] <-> [C*T][ld]
// The reference boundary is [C][2050][T] (T innermost, bsrnn.py:385); inside the library rows are
// frames and columns follow the band-padded map.  32x32 tiles through LDS, both sides coalesced.
template <bool TO_FRAME_MAJOR>
__global__ __launch_bounds__(256) void layout_kernel(FftTables tb, const float* __restrict__ src, float* __restrict__ dst, int T)
{
    __shared__ float tile[32][33];
    const int c = blockIdx.z;
    const int t0 = blockIdx.x * 32, f0 = blockIdx.y * 32;      // f = interleaved column 0..2049
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
    const float* ref = TO_FRAME_MAJOR ? src : nullptr;
    if (TO_FRAME_MAJOR) {
#pragma unroll
        for (int i = 0; i < 32; i += 8) {                      // read [f][t], t contiguous
            const int f = f0 + ty + i, t = t0 + tx;
            if (f < F2 && t < T) tile[ty + i][tx] = ref[((size_t)c * F2 + f) * T + t];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 32; i += 8) {                      // write [t][col(f)], f contiguous
            const int t = t0 + ty + i, f = f0 + tx;
            if (f < F2 && t < T) dst[((size_t)c * T + t) * tb.ld + tb.colmap[f >> 1] + (f & 1)] = tile[tx][ty + i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 32; i += 8) {                      // read [t][col(f)]
            const int t = t0 + ty + i, f = f0 + tx;
            if (f < F2 && t < T) tile[ty + i][tx] = src[((size_t)c * T + t) * tb.ld + tb.colmap[f >> 1] + (f & 1)];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 32; i += 8) {                      // write [f][t]
            const int f = f0 + ty + i, t = t0 + tx;
            if (f < F2 && t < T) dst[((size_t)c * F2 + f) * T + t] = tile[tx][ty + i];
        }
    }
}

// The same transpose for calls of many frames (T >= 32): a workgroup moves 64 interleaved columns x up to 128 frames.  On the
// [C][2050][T] side the 64 rows of a tile are ONE contiguous range when the tile spans all T frames (T <= 128: the offline sizes),
// read / written with 16-byte accesses where T allows; on the frame-major side a wave moves the 64 consecutive columns of one frame
// (256 bytes) per instruction.  32 KB in and out per workgroup instead of 4 KB: 47-49 -> 3x us per launch at R = 64, T = 126.
constexpr int LF = 64, LT = 128;
template <bool TO_FRAME_MAJOR>
__global__ __launch_bounds__(256) void layout_wide_kernel(FftTables tb, const float* __restrict__ src, float* __restrict__ dst, int T)
{
    __shared__ float tile[LF][LT + 1];                         // [column][frame], + 1: conflict-free in both directions
    const int c = blockIdx.z, f0 = blockIdx.y * LF, t0 = blockIdx.x * LT;
    const int nf = F2 - f0 < LF ? F2 - f0 : LF, nt = T - t0 < LT ? T - t0 : LT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cm0 = ((size_t)c * F2 + f0) * T + t0;         // first element of the tile on that side (row stride T)
    const bool whole = nt == T;                                // the tile's rows are adjacent in memory
    const float* const cmp = TO_FRAME_MAJOR ? src : dst;       // the [C][2050][T] side
    const bool vec4 = whole && ((nf * T) & 3) == 0 && ((cm0 & 3) == 0) && ((reinterpret_cast<size_t>(cmp) & 15) == 0);
    // frame-major side: lane = column of the tile, one frame per wave instruction
    const int fcol = f0 + lane;
    const bool col_ok = lane < nf;
    const int dcol = col_ok ? tb.colmap[fcol >> 1] + (fcol & 1) : 0;
    if (TO_FRAME_MAJOR) {
        if (vec4) {
            const int n4 = nf * T / 4;
            for (int i = tid; i < n4; i += 256) {
                const float4 v = *reinterpret_cast<const float4*>(src + cm0 + 4 * (size_t)i);
                int f = (4 * i) / T, t = 4 * i - f * T;
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) { tile[f][t] = e[k]; if (++t == T) { t = 0; ++f; } }
            }
        } else {
            for (int f = wave; f < nf; f += 4)
                for (int t = lane; t < nt; t += 64) tile[f][t] = src[cm0 + (size_t)f * T + t];
        }
        __syncthreads();
        if (col_ok)
            for (int t = wave; t < nt; t += 4) dst[((size_t)c * T + t0 + t) * tb.ld + dcol] = tile[lane][t];
    } else {
        if (col_ok)
            for (int t = wave; t < nt; t += 4) tile[lane][t] = src[((size_t)c * T + t0 + t) * tb.ld + dcol];
        __syncthreads();
        if (vec4) {
            const int n4 = nf * T / 4;
            for (int i = tid; i < n4; i += 256) {
                int f = (4 * i) / T, t = 4 * i - f * T;
                float e[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { e[k] = tile[f][t]; if (++t == T) { t = 0; ++f; } }
                *reinterpret_cast<float4*>(dst + cm0 + 4 * (size_t)i) = make_float4(e[0], e[1], e[2], e[3]);
            }
        } else {
            for (int f = wave; f < nf; f += 4)
                for (int t = lane; t < nt; t += 64) dst[cm0 + (size_t)f * T + t] = tile[f][t];
        }
    }
}

void launch_to_frame_major(const FftTables& tb, const float* x, float* xf, int C, int T, hipStream_t s)
{
    if (T >= 32) {
        hipLaunchKernelGGL(layout_wide_kernel<true>, dim3((T + LT - 1) / LT, (F2 + LF - 1) / LF, C), dim3(256), 0, s, tb, x, xf, T);
        return;
    }
    dim3 grid((T + 31) / 32, (F2 + 31) / 32, C);
    hipLaunchKernelGGL(layout_kernel<true>, grid, dim3(256), 0, s, tb, x, xf, T);
}
void launch_from_frame_major(const FftTables& tb, const float* yf, float* y, int C, int T, hipStream_t s)
{
    if (T >= 32) {
        hipLaunchKernelGGL(layout_wide_kernel<false>, dim3((T + LT - 1) / LT, (F2 + LF - 1) / LF, C), dim3(256), 0, s, tb, yf, y, T);
        return;
    }
    dim3 grid((T + 31) / 32, (F2 + 31) / 32, C);
    hipLaunchKernelGGL(layout_kernel<false>, grid, dim3(256), 0, s, tb, yf, y, T);
}

// ------------------------------------------------------------------------------ streaming DSP
// The four kernels below are templates over ROWS: AllRows is the plain call (an empty argument: the code of a kernel without it), HeldRows
// the row-masked form of bsrnn_stream_process_rows - the set of ACTIVE rows by value (stream_rows_host.h), an optional wet / dry value per
// row, and where the LSTM state of a held row lives and goes.  What a HELD row costs: its workgroups move what their kernel owns from the
// read carry set to the written one - the analysis the buffer, the synthesis the previous frame and the row's LSTM state - and write zeros
// where an active row's spectra and samples go.  A workgroup belongs to one row, so all of that is uniform over the workgroup, and it
// returns before any barrier.  An active row runs the very code of the plain call.
// HopRows (the two block kernels only) is the form of bsrnn_stream_process_hops: a hop count per row by value (stream_rows_host.h) in
// place of the set.  Row r with n = hops[r] of the call's L hops: its frames / hops below n are the plain call's, those from n on are
// zero spectra / zero samples, its carry is the one after n hops (the workgroup whose range holds frame n - 1 writes it), and n = 0 is a
// held row.  The analysis also leaves n in row_frames[r] for the time-axis launches of the call (lstm.hip, the ragged instantiations).
struct AllRows { static constexpr bool masked = false, ragged = false; };
struct HopRows {
    static constexpr bool masked = true, ragged = true;
    RowHops hops;
    const float* mix_rows;             // as HeldRows'
    const float* state_in; float* state_out; int C, K;
    int* row_frames;                   // [C] on the device (analysis only)
};
struct HeldRows {
    static constexpr bool masked = true, ragged = false;
    RowSet active;
    const float* mix_rows;             // [C] on the device, or null: the call's `mix` for every row
    // state [4][2][C*K][64]: row c owns the K*64 floats at (slab * C + c) * K * 64 of each of the eight slabs (multiples of 64 floats:
    // 16-byte aligned).  Copied by the synthesis launch, which follows every launch that wrote state_out for the call.
    const float* state_in; float* state_out; int C, K;
};
__device__ __forceinline__ void copy_floats4(const float* __restrict__ src, float* __restrict__ dst, int n4, int tid)
{
    for (int i = tid; i < n4; i += 256) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
}
__device__ __forceinline__ void zero_floats4(float* __restrict__ dst, int n4, int tid)
{
    for (int i = tid; i < n4; i += 256) reinterpret_cast<float4*>(dst)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// one hop of the caller's output, with the 8-byte stores of the computed ones (the caller's buffer need not be 16-byte aligned)
__device__ __forceinline__ void zero_hop(float* __restrict__ o, int tid)
{
#pragma unroll
    for (int k = 0; k < 2; ++k) *reinterpret_cast<float2*>(o + 2 * (tid + 256 * k)) = make_float2(0.f, 0.f);
}
template <class ROWS>
__device__ __forceinline__ void hold_state_row(const ROWS& h, int c, int tid)
{
    const int n4 = h.K * 16;                              // float4 per slab
    for (int i = tid; i < 8 * n4; i += 256) {
        const int slab = i / n4, j = i - slab * n4;
        const size_t at = ((size_t)slab * h.C + c) * n4 + j;
        reinterpret_cast<float4*>(h.state_out)[at] = reinterpret_cast<const float4*>(h.state_in)[at];
    }
}

template <class ROWS>
__global__ __launch_bounds__(256) void stream_analysis_kernel(FftTables tb, const float* __restrict__ buf_in, float* __restrict__ buf,
                                                              const float* __restrict__ chunk, float* __restrict__ X, ROWS rows)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    if constexpr (ROWS::masked) {
        // held: the buffer as it is, a zero spectrum (all ld columns: rows start 16-byte aligned and ld is a multiple of 4), chunk unread
        const int c = blockIdx.x;
        if (!row_set_has(rows.active, c)) {
            copy_floats4(buf_in + (size_t)c * NFFT, buf + (size_t)c * NFFT, NFFT / 4, tid);
            zero_floats4(X + (size_t)c * tb.ld, tb.ld / 4, tid);
            return;
        }
    }
    const Twiddles twd = load_twiddles<false>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, false);
    const int c = blockIdx.x;
    float* b = buf + (size_t)c * NFFT;
    const float* ch = chunk + (size_t)c * HOPS;
    // new buffer = [old[1024:2048], chunk]   (infer-streaming.py:116)
    float2 keep[2], fresh[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cc = tid + 256 * i;                 // complex index 0..511 of each half
        keep[i] = *reinterpret_cast<const float2*>(buf_in + (size_t)c * NFFT + HOPS + 2 * cc);
        fresh[i] = *reinterpret_cast<const float2*>(ch + 2 * cc);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cc = tid + 256 * i;
        *reinterpret_cast<float2*>(b + 2 * cc) = keep[i];
        *reinterpret_cast<float2*>(b + HOPS + 2 * cc) = fresh[i];
        z0[cc] = make_float2(keep[i].x * tb.hann[2 * cc], keep[i].y * tb.hann[2 * cc + 1]);
        z0[512 + cc] = make_float2(fresh[i].x * tb.hann[HOPS + 2 * cc], fresh[i].y * tb.hann[HOPS + 2 * cc + 1]);
    }
    __syncthreads();
    const float2* Z = fft1024<false>(z0, z1, twd, tid);
    rfft_split_store(Z, spl, X + (size_t)c * tb.ld, tid);
}

template <class ROWS>
__global__ __launch_bounds__(256) void stream_synthesis_kernel(FftTables tb, const float* __restrict__ Y, const float* __restrict__ X,
                                                               const float mix_all, const float* __restrict__ prev_in, float* __restrict__ prev,
                                                               float* __restrict__ out, ROWS rows)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    __shared__ __attribute__((aligned(16))) float spec[F2 + 2];
    const int tid = threadIdx.x;
    float mix = mix_all;
    if constexpr (ROWS::masked) {
        const int c = blockIdx.x;
        if (!row_set_has(rows.active, c)) {
            copy_floats4(prev_in + (size_t)c * NFFT, prev + (size_t)c * NFFT, NFFT / 4, tid);
            zero_hop(out + (size_t)c * HOPS, tid);
            hold_state_row(rows, c, tid);
            return;
        }
        if (rows.mix_rows) mix = rows.mix_rows[c];          // one load per workgroup; mix == 1 below is decided per row
    }
    const Twiddles twd = load_twiddles<true>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, false);
    const int c = blockIdx.x;
    const float* y = Y + (size_t)c * tb.ld;
    const float* x = X + (size_t)c * tb.ld;
    // wet/dry on the spectrum (speech-ladspa-onnx.cpp:215-226); mix = 1 is the plain model output
    const float dry = mix >= 0.f ? 1.f - mix : 1.f;
    for (int i = tid; i < F2; i += 256) {
        const int col = tb.colmap[i >> 1] + (i & 1);
        spec[i] = (mix == 1.f) ? y[col] : mix * y[col] + dry * x[col];
    }
    __syncthreads();
    irfft_merge<true>(spec, spl, z0, tid);
    __syncthreads();
    const float2* z = fft1024<true>(z0, z1, twd, tid);
    float* pv = prev + (size_t)c * NFFT;
    float* o = out + (size_t)c * HOPS;
    const float sc = 1.0f / 1024.0f;
    // out = (s_now[0:1024] + s_prev[1024:2048]) / (w[0:1024] + w[1024:2048]); prev = s_now
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cc = tid + 256 * i;                 // samples 2cc, 2cc+1 of the first half
        const float2 now = make_float2(z[cc].x * sc, z[cc].y * sc);
        const float2 old = *reinterpret_cast<const float2*>(prev_in + (size_t)c * NFFT + HOPS + 2 * cc);
        *reinterpret_cast<float2*>(o + 2 * cc) =
            make_float2((now.x + old.x) * tb.inv_wsum[2 * cc], (now.y + old.y) * tb.inv_wsum[2 * cc + 1]);
    }
    __syncthreads();
    for (int cc = tid; cc < 1024; cc += 256)
        *reinterpret_cast<float2*>(pv + 2 * cc) = make_float2(z[cc].x * sc, z[cc].y * sc);
}

// Zeroes the carry of the rows in `rows` in one carry set (bsrnn_stream_reset_rows): one workgroup per row of the stream.
__global__ __launch_bounds__(256) void stream_reset_rows_kernel(RowSet rows, float* __restrict__ buf, float* __restrict__ prev, float* __restrict__ state,
                                                                int C, int K)
{
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    if (!row_set_has(rows, c)) return;
    zero_floats4(buf + (size_t)c * NFFT, NFFT / 4, tid);
    zero_floats4(prev + (size_t)c * NFFT, NFFT / 4, tid);
    const int n4 = K * 16;
    for (int slab = 0; slab < 8; ++slab) zero_floats4(state + ((size_t)slab * C + c) * n4 * 4, n4, tid);
}

// (a one-hop call is never HOPS: kernels.h, StreamRows)
void launch_stream_analysis(const FftTables& tb, const float* buf_in, float* buf_out, const float* chunk, float* X, int C, const StreamRows& rows,
                            hipStream_t s)
{
    if (rows.kind == StreamRows::ALL) hipLaunchKernelGGL(stream_analysis_kernel<AllRows>, dim3(C), dim3(256), 0, s, tb, buf_in, buf_out, chunk, X, AllRows{});
    else hipLaunchKernelGGL(stream_analysis_kernel<HeldRows>, dim3(C), dim3(256), 0, s, tb, buf_in, buf_out, chunk, X, HeldRows{rows.active, nullptr, nullptr, nullptr, C, 0});
}
void launch_stream_synthesis(const FftTables& tb, const float* Y, const float* X, float mix, const float* prev_in, float* prev_out, float* out,
                             const float* state_in, float* state_out, int C, int K, const StreamRows& rows, hipStream_t s)
{
    if (rows.kind == StreamRows::ALL) hipLaunchKernelGGL(stream_synthesis_kernel<AllRows>, dim3(C), dim3(256), 0, s, tb, Y, X, mix, prev_in, prev_out, out, AllRows{});
    else hipLaunchKernelGGL(stream_synthesis_kernel<HeldRows>, dim3(C), dim3(256), 0, s, tb, Y, X, mix, prev_in, prev_out, out,
                            HeldRows{rows.active, rows.mix_rows, state_in, state_out, C, K});
}
void launch_stream_reset_rows(float* buf, float* prev, float* state, int C, int K, const RowSet& rows, hipStream_t s)
{
    hipLaunchKernelGGL(stream_reset_rows_kernel, dim3(C), dim3(256), 0, s, rows, buf, prev, state, C, K);
}

// ------------------------------------------------------------------------------ streaming DSP, a block of L hops per row
// The two kernels above for L consecutive hops in one launch (bsrnn_stream_process), built like the offline pair: a workgroup walks
// `sch` consecutive hops of one row (the analysis with stft_walk).  Per row the analysis reads S = buf_in[0:2048] ++ chunk[0:L*1024]; frame l is
// S[(l+1)*1024 : (l+1)*1024 + 2048] (no reflection: the history is the carried buffer), and the new carry is the last frame's raw
// samples.  Per frame the arithmetic is that of the one-hop kernels, in their order.
// ROWS = HeldRows: a held row's workgroups write zero spectra for their frames, and the one that owns the last hop copies the buffer.
template <class ROWS>
__global__ __launch_bounds__(256, FFT_OCC_STFT) void stream_block_analysis_kernel(FftTables tb, const float* __restrict__ buf_in, float* __restrict__ buf_out,
                                                                                  const float* __restrict__ chunk, float* __restrict__ X, int L, int sch,
                                                                                  ROWS rows)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int l0 = blockIdx.x * sch;
    int l1 = (l0 + sch < L) ? l0 + sch : L;
    int n = L;                                                       // the frames the row advances by
    if constexpr (ROWS::ragged) {
        n = row_hops_of(rows.hops, r);
        if (l0 == 0 && tid == 0) rows.row_frames[r] = n;
        for (int l = l0 > n ? l0 : n; l < l1; ++l) zero_floats4(X + ((size_t)r * L + l) * tb.ld, tb.ld / 4, tid);
        if (n == 0 && l0 == 0) copy_floats4(buf_in + (size_t)r * NFFT, buf_out + (size_t)r * NFFT, NFFT / 4, tid);
        if (l0 >= n) return;                                         // (uniform over the workgroup, before any barrier)
        if (l1 > n) l1 = n;
    } else if constexpr (ROWS::masked) {
        if (!row_set_has(rows.active, r)) {
            for (int l = l0; l < l1; ++l) zero_floats4(X + ((size_t)r * L + l) * tb.ld, tb.ld / 4, tid);
            if (l1 == L) copy_floats4(buf_in + (size_t)r * NFFT, buf_out + (size_t)r * NFFT, NFFT / 4, tid);
            return;
        }
    }
    const float* carry = buf_in + (size_t)r * NFFT;
    const float* fresh = chunk + (size_t)r * L * HOPS;
    // complex sample c (0..1023) of frame l = S[(l+1)*1024 + 2c], S[.. + 1]: the carried buffer below index 2048 of S, the chunk above
    // (both indices on the same side: the boundary is even)
    auto sample2 = [&](int l, int c) {
        const int64_t j = (int64_t)(l + 1) * HOPS + 2 * c;
        return *reinterpret_cast<const float2*>(j < NFFT ? carry + j : fresh + (j - NFFT));
    };
    auto row = [&](int l) { return X + ((size_t)r * L + l) * tb.ld; };
    const RawHalf last = stft_walk(tb, z0, z1, tid, l0, l1, sample2, row);
    // the workgroup that owns the last hop leaves the new carry: buf_out = S[L*1024 : L*1024 + 2048] = the last frame's samples (its
    // first half is read again here instead of being kept through the loop; buf_out is another set than buf_in).  HopRows: n for L
    if (l1 == n) {
        float* b = buf_out + (size_t)r * NFFT;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = tid + 256 * k;
            *reinterpret_cast<float2*>(b + 2 * c) = sample2(n - 1, c);
            *reinterpret_cast<float2*>(b + HOPS + 2 * c) = last.v[k];   // the last frame's second half, as the walk left it
        }
    }
}

// out hop l = (wf_l[0:1024] + wf_{l-1}[1024:2048]) * inv_wsum with wf_l = irfft(mix(Y_l, X_l)) and wf_{-1} = prev_in; no synthesis
// window.  A workgroup produces output hops [b0, b1) of one row, keeps the second half of the previous frame in registers and either
// reads it from prev_in (b0 = 0) or recomputes frame b0 - 1; the spectrum of the next frame is requested before the FFT passes of the
// current one.  MIX: the wet / dry control of stream_synthesis_kernel (the launcher picks MIX = mix != 1).
// ROWS = HeldRows: a held row's workgroups write zeros to their hops, and the first of them copies the previous frame and the row's LSTM
// state.  With a wet / dry value per row the launcher picks MIX = true, and a row at 1 skips the blend (a branch around register
// arithmetic only, uniform over the workgroup): its spectra reach the transform untouched, as under MIX = false.
template <bool MIX, class ROWS>
__global__ __launch_bounds__(256, FFT_OCC_ISTFT) void stream_block_synthesis_kernel(FftTables tb, const float* __restrict__ Y, const float* __restrict__ X,
                                                                                    const float mix_all, const float* __restrict__ prev_in,
                                                                                    float* __restrict__ prev_out, float* __restrict__ out, int L, int ich,
                                                                                    ROWS rows)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    float mix = mix_all;
    int n = L;                                                       // the hops the row advances by
    if constexpr (ROWS::ragged) {
        const int r = blockIdx.y;
        n = row_hops_of(rows.hops, r);
        const int b0 = blockIdx.x * ich;
        const int b1 = (b0 + ich < L) ? b0 + ich : L;
        for (int b = b0 > n ? b0 : n; b < b1; ++b) zero_hop(out + ((size_t)r * L + b) * HOPS, tid);
        if (n == 0 && blockIdx.x == 0) {
            copy_floats4(prev_in + (size_t)r * NFFT, prev_out + (size_t)r * NFFT, NFFT / 4, tid);
            hold_state_row(rows, r, tid);
        }
        if (b0 >= n) return;                                         // (uniform over the workgroup, before any barrier)
        if (MIX && rows.mix_rows) mix = rows.mix_rows[r];
    } else if constexpr (ROWS::masked) {
        const int r = blockIdx.y;
        if (!row_set_has(rows.active, r)) {
            const int b0 = blockIdx.x * ich;
            const int b1 = (b0 + ich < L) ? b0 + ich : L;
            for (int b = b0; b < b1; ++b) zero_hop(out + ((size_t)r * L + b) * HOPS, tid);
            if (blockIdx.x == 0) {
                copy_floats4(prev_in + (size_t)r * NFFT, prev_out + (size_t)r * NFFT, NFFT / 4, tid);
                hold_state_row(rows, r, tid);
            }
            return;
        }
        if (MIX && rows.mix_rows) mix = rows.mix_rows[r];
    }
    const bool blend = !ROWS::masked || mix != 1.f;       // (AllRows: the launcher chose MIX by it)
    const Twiddles twd = load_twiddles<true>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, true);
    const int r = blockIdx.y;
    const int b0 = blockIdx.x * ich;
    const int b1 = (b0 + ich < n) ? b0 + ich : n;                    // output hops [b0, b1) <- frames b0 - 1 .. b1 - 1 (n = L but for HopRows)
    const float sc = 1.0f / 1024.0f;
    const float dry = mix >= 0.f ? 1.f - mix : 1.f;
    float2 wsum[2], carry[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = tid + 256 * k;
        wsum[k] = make_float2(tb.inv_wsum[2 * c], tb.inv_wsum[2 * c + 1]);
    }
    const float* Yr = Y + (size_t)r * L * tb.ld;
    const float* Xr = X + (size_t)r * L * tb.ld;
    float* o = out + (size_t)r * L * HOPS;
    MergeRegs my, mx;
    auto request = [&](int t) {
        irfft_load<false>(Yr + (size_t)t * tb.ld, spl, my, tid);
        if (MIX) irfft_load<false>(Xr + (size_t)t * tb.ld, spl, mx, tid);
    };
    // The frame in front of the range only fills the carry; it is peeled so that the loop body has no branch around its loads and stores
    auto frame = [&](int t, auto first) {
        if (MIX && blend) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                my.xk[i] = make_float2(fmaf(mix, my.xk[i].x, dry * mx.xk[i].x), fmaf(mix, my.xk[i].y, dry * mx.xk[i].y));
                my.xc[i] = make_float2(fmaf(mix, my.xc[i].x, dry * mx.xc[i].x), fmaf(mix, my.xc[i].y, dry * mx.xc[i].y));
            }
        }
        // The fused multiply-adds of the blend above and of the merge are spelled out (irfft_store<true>), as in istft_walk: left to the
        // compiler's contraction, which product is rounded first differed between the instantiations of this kernel, and a row of a rows
        // call has to get the bits of the plain call whichever of them computes it.
        irfft_store<true>(my, spl, z0, tid);
        __syncthreads();
        request(t + 1 < b1 ? t + 1 : t);                              // (after the last frame: a dummy reload)
        const float2* z = fft1024<true>(z0, z1, twd, tid);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = tid + 256 * k;
            const float2 a = z[c], b = z[c + 512];
            if (!decltype(first)::value) {
                // same operation order as the one-hop kernel: frame * 1/1024, add, times 1 / window sum
                const float2 now = make_float2(a.x * sc, a.y * sc);
                *reinterpret_cast<float2*>(o + (size_t)t * HOPS + 2 * c) =
                    make_float2((now.x + carry[k].x) * wsum[k].x, (now.y + carry[k].y) * wsum[k].y);
            }
            carry[k] = make_float2(b.x * sc, b.y * sc);
        }
        __syncthreads();                              // z (= z1) is overwritten by the next frame's first pass
    };
    if (b0 == 0) {
        request(0);
#pragma unroll
        for (int k = 0; k < 2; ++k) carry[k] = *reinterpret_cast<const float2*>(prev_in + (size_t)r * NFFT + HOPS + 2 * (tid + 256 * k));
    } else {
        request(b0 - 1);
        frame(b0 - 1, std::true_type());
    }
    for (int t = b0; t < b1; ++t) frame(t, std::false_type());
    // the workgroup that owns the last hop leaves the whole last frame as the new carry, in the one-hop kernel's layout (fft1024 ends
    // in z1, which nothing has touched since the last frame)
    if (b1 == n) {
        float* pv = prev_out + (size_t)r * NFFT;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i;
            *reinterpret_cast<float2*>(pv + 2 * c) = make_float2(z1[c].x * sc, z1[c].y * sc);
        }
    }
}

// One launcher per direction: the instantiation by rows.kind.  (The chunk lengths may differ between the instantiations: a hop has the
// same bits whichever workgroup computes it, see above.)
template <class ROWS>
static void stream_block_analysis(const FftTables& tb, const float* buf_in, float* buf_out, const float* chunk, float* X, int C, int L, const ROWS& rows,
                                  hipStream_t s)
{
    const Chunks ch = chunks_for<stream_block_analysis_kernel<ROWS>>(L, C, 0);
    hipLaunchKernelGGL(stream_block_analysis_kernel<ROWS>, ch.grid, dim3(256), 0, s, tb, buf_in, buf_out, chunk, X, L, ch.len, rows);
}
void launch_stream_block_analysis(const FftTables& tb, const float* buf_in, float* buf_out, const float* chunk, float* X, int C, int L,
                                  const StreamRows& rows, int* row_frames, hipStream_t s)
{
    switch (rows.kind) {
    case StreamRows::ALL: stream_block_analysis(tb, buf_in, buf_out, chunk, X, C, L, AllRows{}, s); break;
    case StreamRows::HELD: stream_block_analysis(tb, buf_in, buf_out, chunk, X, C, L, HeldRows{rows.active, nullptr, nullptr, nullptr, C, 0}, s); break;
    case StreamRows::HOPS: stream_block_analysis(tb, buf_in, buf_out, chunk, X, C, L, HopRows{rows.hops, nullptr, nullptr, nullptr, C, 0, row_frames}, s); break;
    }
}
// MIX = false: every row's wet / dry value is 1 (no blend with X)
template <class ROWS>
static void stream_block_synthesis(const FftTables& tb, const float* Y, const float* X, float mix, bool blend, const float* prev_in, float* prev_out,
                                   float* out, int C, int L, const ROWS& rows, hipStream_t s)
{
    const Chunks ch = chunks_for<stream_block_synthesis_kernel<false, ROWS>>(L, C, 1);
    if (!blend) hipLaunchKernelGGL((stream_block_synthesis_kernel<false, ROWS>), ch.grid, dim3(256), 0, s, tb, Y, X, mix, prev_in, prev_out, out, L, ch.len, rows);
    else hipLaunchKernelGGL((stream_block_synthesis_kernel<true, ROWS>), ch.grid, dim3(256), 0, s, tb, Y, X, mix, prev_in, prev_out, out, L, ch.len, rows);
}
void launch_stream_block_synthesis(const FftTables& tb, const float* Y, const float* X, float mix, const float* prev_in, float* prev_out, float* out,
                                   const float* state_in, float* state_out, int C, int K, int L, const StreamRows& rows, hipStream_t s)
{
    const bool blend = rows.mix_rows || mix != 1.f;
    switch (rows.kind) {
    case StreamRows::ALL: stream_block_synthesis(tb, Y, X, mix, blend, prev_in, prev_out, out, C, L, AllRows{}, s); break;
    case StreamRows::HELD:
        stream_block_synthesis(tb, Y, X, mix, blend, prev_in, prev_out, out, C, L, HeldRows{rows.active, rows.mix_rows, state_in, state_out, C, K}, s);
        break;
    case StreamRows::HOPS:
        stream_block_synthesis(tb, Y, X, mix, blend, prev_in, prev_out, out, C, L, HopRows{rows.hops, rows.mix_rows, state_in, state_out, C, K, nullptr}, s);
        break;
    }
}

// ------------------------------------------------------------------------------ offline DSP, one segment of a clip
// The offline pair for frames [ta, te) of a clip of T = 1 + n / 1024 frames (bsrnn_separate_long): the clip is transformed segment after
// segment, so nothing here grows with the clip.  Both kernels run the shared walks (stft_walk / istft_walk), like stft_kernel<false> /
// istft_fused_kernel: given the same samples / spectra, a segment's rows and hops are bit-identical to the same frames of the one-shot kernels.
//
// Analysis: padded sample i of frame t is sample t*1024 + i - 1024 of the WHOLE clip, reflected at 0 and at n - 1 (never at a segment
// edge).  `src` is either the whole clip (base = 0, stride = n) or a staged window of it that starts at clip sample `base` (rows `stride`
// floats apart); `base` is subtracted after the reflection, and the caller makes the window hold every index the segment touches
// (plan_host.h: segment_window).  Rows of X are segment-local: X[(r * (te - ta) + (t - ta)) * ld].
__global__ __launch_bounds__(256, FFT_OCC_STFT) void stft_segment_kernel(FftTables tb, const float* __restrict__ wave, float* __restrict__ X,
                                                                         int64_t n, int64_t base, int64_t stride, int ta, int te, int sch)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int t0 = ta + blockIdx.x * sch;
    const int t1 = (t0 + sch < te) ? t0 + sch : te;
    const float* src = wave + (size_t)r * stride;
    auto sample2 = [&](int t, int c) { return reflected_sample2(src, n, base, t, c); };
    auto row = [&](int t) { return X + ((size_t)r * (te - ta) + (t - ta)) * tb.ld; };
    stft_walk(tb, z0, z1, tid, t0, t1, sample2, row);
}

// Synthesis: Y = the spectra of the segment's L = te - ta frames (segment-local rows).  Output hop b of the clip is the first half of
// frame b + 1 plus the second half of frame b, so the segment completes hops [max(ta - 1, 0), te - 1): every frame but the clip's first
// completes one.  A workgroup walks the frames [a0, a1) that complete its hops with the windowed second half of the frame in front in
// registers: recomputed from that frame (istft_walk's peeled frame, as in istft_fused_kernel) - or, for the segment's first frame when the clip has frames in
// front of it (carry_in != null), read from carry_in [R][1024], where the previous segment's launch left exactly those registers
// (sample j of the windowed and scaled second half at [r][j]).  The workgroup that walks frame L - 1 leaves carry_out likewise (another
// set than carry_in).  `out` points at the segment's first hop of row 0, rows out_stride floats apart.
__global__ __launch_bounds__(256, FFT_OCC_ISTFT) void istft_segment_kernel(FftTables tb, const float* __restrict__ Y, float* __restrict__ out, int64_t out_stride,
                                                                           const float* __restrict__ carry_in, float* __restrict__ carry_out, int L, int ich)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int f0 = carry_in ? 0 : 1;                                  // the first frame that completes a hop (local hop = frame - f0)
    const int a0 = f0 + blockIdx.x * ich;
    const int a1 = (a0 + ich < L) ? a0 + ich : L;                     // (a one-frame first segment: a0 = a1 = 1, the carry only)
    const float* Yr = Y + (size_t)r * L * tb.ld;
    float* o = out + (size_t)r * out_stride;
    auto spectrum = [&](int t) { return Yr + (size_t)t * tb.ld; };
    auto hop = [&](int t) { return o + (size_t)(t - f0) * HOPS; };
    float2 carry[2];
    if (a0 == 0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) carry[k] = *reinterpret_cast<const float2*>(carry_in + (size_t)r * HOPS + 2 * (tid + 256 * k));
    }
    istft_walk(tb, z0, z1, tid, a0, a1, spectrum, hop, a0 > 0, carry);
    if (a1 == L) {
#pragma unroll
        for (int k = 0; k < 2; ++k) *reinterpret_cast<float2*>(carry_out + (size_t)r * HOPS + 2 * (tid + 256 * k)) = carry[k];
    }
}

void launch_stft_segment(const FftTables& tb, const float* src, int64_t stride, int64_t base, float* X, int R, int64_t n, int ta, int te, hipStream_t s)
{
    const Chunks ch = chunks_for<stft_segment_kernel>(te - ta, R, 0);
    hipLaunchKernelGGL(stft_segment_kernel, ch.grid, dim3(256), 0, s, tb, src, X, n, base, stride, ta, te, ch.len);
}
void launch_istft_segment(const FftTables& tb, const float* Y, float* out, int64_t out_stride, const float* carry_in, float* carry_out, int R, int L,
                          hipStream_t s)
{
    const int hops = L - (carry_in ? 0 : 1);                           // 0: a one-frame first segment (one workgroup per row leaves the carry)
    const Chunks ch = chunks_for<istft_segment_kernel>(hops > 0 ? hops : 1, R, 1);
    hipLaunchKernelGGL(istft_segment_kernel, ch.grid, dim3(256), 0, s, tb, Y, out, out_stride, carry_in, carry_out, L, ch.len);
}

// ------------------------------------------------------------------------------ offline DSP, rows of different lengths
// The offline pair for a batch whose row r holds lens[r] samples (bsrnn_separate_ragged): T_r = 1 + lens[r] / 1024 frames of its own inside a
// rectangle of Tmax = max T_r frames per row.  Both kernels run the shared walks (stft_walk / istft_walk), like stft_kernel<false> /
// istft_fused_kernel: a frame or a hop that both compute has the same bits.  Row and chunk belong to the workgroup, so every condition below is
// workgroup-uniform, and each walk is one loop over the real frames / hops (no branch inside it) and one over the padded ones.
//
// Analysis: frames t < T_r of row r come from wave + r * stride, reflected at 0 and at lens[r] - 1 (never at the stride: samples
// [lens[r], stride) are not read).  Frames T_r <= t < Tmax are written as zeros in ALL ld columns of their row of X: the workspace is reused
// from call to call, and what an earlier call left there must reach neither the range guard nor, through 0 * mask, the rows of Y.
__global__ __launch_bounds__(256, FFT_OCC_STFT) void stft_ragged_kernel(FftTables tb, const float* __restrict__ wave, float* __restrict__ X,
                                                                        int64_t stride, const int64_t* __restrict__ lens, int Tmax, int sch)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int64_t n = lens[r];
    const int Tr = 1 + (int)(n / HOPS);
    const int t0 = blockIdx.x * sch;
    const int te = (t0 + sch < Tmax) ? t0 + sch : Tmax;               // the chunk: frames [t0, te) of the rectangle
    const int t1 = te < Tr ? te : Tr;                                 // its real frames: [t0, t1), none when t1 <= t0
    float* Xr = X + (size_t)r * Tmax * tb.ld;
    if (t0 < t1) {
        const float* src = wave + (size_t)r * stride;
        auto sample2 = [&](int t, int c) { return reflected_sample2(src, n, 0, t, c); };
        auto row = [&](int t) { return Xr + (size_t)t * tb.ld; };
        stft_walk(tb, z0, z1, tid, t0, t1, sample2, row);
    }
    // the padded frames of the chunk (rows of X start 16-byte aligned and ld is a multiple of 4: commit_host.h, band_columns)
    for (int t = t0 > t1 ? t0 : t1; t < te; ++t) {
        float4* row = reinterpret_cast<float4*>(Xr + (size_t)t * tb.ld);
        for (int i = tid; i < tb.ld / 4; i += 256) row[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Synthesis: Y = the spectra of the rectangle, [R * Tmax][ld]; row r of `out` starts at out + r * out_stride and holds Tmax - 1 hops.  Hops
// b < T_r - 1 are computed from frames b and b + 1 by istft_walk, as istft_fused_kernel's are; hops T_r - 1 <= b < Tmax - 1 are STORED as zeros, not
// computed (hop T_r - 1 would add the row's last real second half to a padded frame).  A workgroup whose chunk lies past the row's end does
// no FFT.
__global__ __launch_bounds__(256, FFT_OCC_ISTFT) void istft_ragged_kernel(FftTables tb, const float* __restrict__ Y, float* __restrict__ out, int64_t out_stride,
                                                                          const int64_t* __restrict__ lens, int Tmax, int ich)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int Tr = 1 + (int)(lens[r] / HOPS);
    const int b0 = blockIdx.x * ich;
    const int be = (b0 + ich < Tmax - 1) ? b0 + ich : Tmax - 1;      // the chunk: hops [b0, be) of the rectangle
    const int b1 = be < Tr - 1 ? be : Tr - 1;                         // its real hops: [b0, b1) <- frames b0 .. b1, none when b1 <= b0
    float* o = out + (size_t)r * out_stride;
    if (b0 < b1) {
        const float* Yr = Y + (size_t)r * Tmax * tb.ld;
        auto spectrum = [&](int t) { return Yr + (size_t)t * tb.ld; };
        auto hop = [&](int t) { return o + (size_t)(t - 1) * HOPS; };
        float2 carry[2];
        istft_walk(tb, z0, z1, tid, b0 + 1, b1 + 1, spectrum, hop, true, carry);
    }
    // the padded hops of the chunk, at the addresses and with the 8-byte stores of the real ones
    for (int b = b0 > b1 ? b0 : b1; b < be; ++b) {
#pragma unroll
        for (int k = 0; k < 2; ++k) *reinterpret_cast<float2*>(o + (size_t)b * HOPS + 2 * (tid + 256 * k)) = make_float2(0.f, 0.f);
    }
}

void launch_stft_ragged(const FftTables& tb, const float* wave, int64_t stride, const int64_t* lens, float* X, int R, int Tmax, hipStream_t s)
{
    const Chunks ch = chunks_for<stft_ragged_kernel>(Tmax, R, 0);
    hipLaunchKernelGGL(stft_ragged_kernel, ch.grid, dim3(256), 0, s, tb, wave, X, stride, lens, Tmax, ch.len);
}
void launch_istft_ragged(const FftTables& tb, const float* Y, float* out, int64_t out_stride, const int64_t* lens, int R, int Tmax, hipStream_t s)
{
    if (Tmax < 2) return;
    const Chunks ch = chunks_for<istft_ragged_kernel>(Tmax - 1, R, 1);
    hipLaunchKernelGGL(istft_ragged_kernel, ch.grid, dim3(256), 0, s, tb, Y, out, out_stride, lens, Tmax, ch.len);
}

// ------------------------------------------------------------------------------ backward of the ragged iSTFT (ragged training step)
// The transpose of istft_ragged_kernel, row by row: launch_istft_backward's three passes with the row's own bounds.  Row r of dwave (rows
// `stride` floats apart) carries gradient in its first n_est_r = (T_r - 1) * 1024 samples; what lies behind them is never read.
//   1. g[r][i] = dwave[r][i] / envelope, i < n_est_r only (the arithmetic of istft_bwd_prescale_kernel);
//   2. the ZERO_PAD analysis of g on frames t < T_r with the bound n_est_r - stft_walk, as stft_kernel<true> runs it, so a frame that both
//      compute has the same bits - and zero rows for frames T_r <= t < Tmax, in all ld columns;
//   3. the bin weights of istft_bwd_postscale_kernel on frames t < T_r only (the padded rows stay the zeros of pass 2).
// Row and chunk belong to the workgroup in all three, so every length condition is workgroup-uniform.
__global__ __launch_bounds__(256) void istft_ragged_bwd_prescale_kernel(FftTables tb, const float* __restrict__ dwave, float* __restrict__ g,
                                                                        int64_t stride, const int64_t* __restrict__ lens)
{
    const int r = blockIdx.y;
    const int64_t hops = lens[r] / HOPS;                               // n_est_r / 1024
    const float* src = dwave + (size_t)r * stride;
    float* dst = g + (size_t)r * stride;
    for (int64_t b = blockIdx.x; b < hops; b += gridDim.x)
        for (int j = threadIdx.x; j < HOPS; j += 256) {
            const float w0 = tb.hann[j], w1 = tb.hann[j + HOPS];
            dst[b * HOPS + j] = src[b * HOPS + j] / (w0 * w0 + w1 * w1);
        }
}
__global__ __launch_bounds__(256, FFT_OCC_STFT) void stft_ragged_zero_pad_kernel(FftTables tb, const float* __restrict__ g, float* __restrict__ X,
                                                                                 int64_t stride, const int64_t* __restrict__ lens, int Tmax, int sch)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int Tr = 1 + (int)(lens[r] / HOPS);
    const int64_t n = (int64_t)(Tr - 1) * HOPS;                        // n_est_r: samples outside [0, n) are zeros
    const int t0 = blockIdx.x * sch;
    const int te = (t0 + sch < Tmax) ? t0 + sch : Tmax;               // the chunk: frames [t0, te) of the rectangle
    const int t1 = te < Tr ? te : Tr;                                 // its real frames: [t0, t1), none when t1 <= t0
    float* Xr = X + (size_t)r * Tmax * tb.ld;
    if (t0 < t1) {
        const float* src = g + (size_t)r * stride;
        auto sample2 = [&](int t, int c) {
            float v[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int64_t idx = (int64_t)t * HOPS + 2 * c + e - NFFT / 2;
                v[e] = (idx >= 0 && idx < n) ? src[idx] : 0.f;
            }
            return make_float2(v[0], v[1]);
        };
        auto row = [&](int t) { return Xr + (size_t)t * tb.ld; };
        stft_walk(tb, z0, z1, tid, t0, t1, sample2, row);
    }
    for (int t = t0 > t1 ? t0 : t1; t < te; ++t) {
        float4* row = reinterpret_cast<float4*>(Xr + (size_t)t * tb.ld);
        for (int i = tid; i < tb.ld / 4; i += 256) row[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// grid (Tmax, R): one frame row per workgroup
__global__ __launch_bounds__(256) void istft_ragged_bwd_postscale_kernel(FftTables tb, float* __restrict__ X, const int64_t* __restrict__ lens, int Tmax)
{
    const int r = blockIdx.y, t = blockIdx.x;
    if (t >= 1 + (int)(lens[r] / HOPS)) return;
    float* row = X + ((size_t)r * Tmax + t) * tb.ld;
    for (int k = threadIdx.x; k < NBINS; k += 256) {
        float* p = row + tb.colmap[k];
        const bool edge = k == 0 || k == NBINS - 1;
        const float sc = (edge ? 1.0f : 2.0f) / (float)NFFT;
        p[0] *= sc;
        p[1] = edge ? 0.f : p[1] * sc;
    }
}
void launch_istft_ragged_backward(const FftTables& tb, const float* dwave, float* scratch, float* dY, const int64_t* lens, int R, int Tmax, hipStream_t s)
{
    if (Tmax < 2) return;
    const int64_t stride = (int64_t)(Tmax - 1) * HOPS;
    const int pre = Tmax - 1 < 64 ? Tmax - 1 : 64;
    hipLaunchKernelGGL(istft_ragged_bwd_prescale_kernel, dim3(pre, R), dim3(256), 0, s, tb, dwave, scratch, stride, lens);
    const Chunks ch = chunks_for<stft_ragged_zero_pad_kernel>(Tmax, R, 0);
    hipLaunchKernelGGL(stft_ragged_zero_pad_kernel, ch.grid, dim3(256), 0, s, tb, scratch, dY, stride, lens, Tmax, ch.len);
    hipLaunchKernelGGL(istft_ragged_bwd_postscale_kernel, dim3(Tmax, R), dim3(256), 0, s, tb, dY, lens, Tmax);
}

// ------------------------------------------------------------------------------ offline DSP, one segment of rows of different lengths
// The two pairs above put together for frames [ta, te) of a ragged batch (bsrnn_separate_long_ragged): a segment's bounds AND a row's own.
// Both kernels run the shared walks, so a frame or a hop that one of the other pairs computes too has the same bits; row and chunk belong
// to the workgroup, so every condition below is workgroup-uniform, and each walk is one loop over the real frames / hops (no branch inside
// it) and one over the padded ones.
//
// Analysis, on the Ri rows of the segment's alive prefix: frames t in [ta, min(te, T_r)) of row r come from wave + r * stride, reflected at
// 0 and at lens[r] - 1 (never at a segment edge or at the stride: nothing at or behind lens[r] is read); frames [T_r, te) are written as
// zeros in ALL ld columns.  Rows of X are segment-local: X[(r * (te - ta) + (t - ta)) * ld].
__global__ __launch_bounds__(256, FFT_OCC_STFT) void stft_ragged_segment_kernel(FftTables tb, const float* __restrict__ wave, float* __restrict__ X,
                                                                                int64_t stride, const int64_t* __restrict__ lens, int ta, int te, int sch)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int64_t n = lens[r];
    const int Tr = 1 + (int)(n / HOPS);
    const int t0 = ta + blockIdx.x * sch;
    const int tc = (t0 + sch < te) ? t0 + sch : te;                   // the chunk: frames [t0, tc) of the segment
    const int t1 = tc < Tr ? tc : Tr;                                 // its real frames: [t0, t1), none when t1 <= t0
    float* Xr = X + (size_t)r * (te - ta) * tb.ld;
    if (t0 < t1) {
        const float* src = wave + (size_t)r * stride;
        auto sample2 = [&](int t, int c) { return reflected_sample2(src, n, 0, t, c); };
        auto row = [&](int t) { return Xr + (size_t)(t - ta) * tb.ld; };
        stft_walk(tb, z0, z1, tid, t0, t1, sample2, row);
    }
    // the padded frames of the chunk (rows of X start 16-byte aligned and ld is a multiple of 4: commit_host.h, band_columns)
    for (int t = t0 > t1 ? t0 : t1; t < tc; ++t) zero_floats4(Xr + (size_t)(t - ta) * tb.ld, tb.ld / 4, tid);
}

// Synthesis, on ALL R rows of the call (every output sample of the segment's hops is written): Y = the spectra of the segment's L = te - ta
// frames of the Ri rows of the prefix, `out` points at the segment's first hop of row 0, carry_in / carry_out as istft_segment_kernel's
// (carry_in == null: the clip's first segment).  Local frame a = t - ta completes clip hop t - 1, which is real when t < T_r: those are
// computed as istft_segment_kernel computes them (the segment's first from carry_in[r]), every other hop of the segment is STORED as zeros.
// A workgroup with no real hop - a row at or beyond Ri, a chunk past the row's end - does no FFT and reads no row of Y.  The workgroup
// whose chunk ends the segment leaves carry_out[r]: the windowed second half of frame te - 1 when the row has a frame te to add it to,
// else zeros (nothing reads them; the buffer never holds stale values).
__global__ __launch_bounds__(256, FFT_OCC_ISTFT) void istft_ragged_segment_kernel(FftTables tb, const float* __restrict__ Y, float* __restrict__ out,
                                                                                  int64_t out_stride, const int64_t* __restrict__ lens,
                                                                                  const float* __restrict__ carry_in, float* __restrict__ carry_out,
                                                                                  int ta, int te, int Ri, int ich)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = blockIdx.y;
    const int L = te - ta;
    const int Tr = 1 + (int)(lens[r] / HOPS);
    const int f0 = carry_in ? 0 : 1;                                  // the first frame that completes a hop (local hop = frame - f0)
    const int a0 = f0 + blockIdx.x * ich;
    const int ac = (a0 + ich < L) ? a0 + ich : L;                     // the chunk: local frames [a0, ac) (a one-frame first segment: a0 = ac = 1)
    const int Lr = r < Ri ? (Tr - ta < L ? Tr - ta : L) : 0;          // the row's real frames of the segment: local [0, Lr), none when Lr <= 0
    const int a1 = ac < Lr ? ac : Lr;                                 // the chunk's real frames: [a0, a1), none when a1 <= a0
    const bool last = ac == L;                                        // this workgroup leaves the carry ...
    const bool onward = last && Tr > te;                              // ... and the row goes on behind the segment (then Lr = L and a1 = ac)
    float* o = out + (size_t)r * out_stride;
    float2 carry[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
    if (a0 < a1 || onward) {
        const float* Yr = Y + (size_t)r * L * tb.ld;
        auto spectrum = [&](int t) { return Yr + (size_t)t * tb.ld; };
        auto hop = [&](int t) { return o + (size_t)(t - f0) * HOPS; };
        if (a0 == 0) {
#pragma unroll
            for (int k = 0; k < 2; ++k) carry[k] = *reinterpret_cast<const float2*>(carry_in + (size_t)r * HOPS + 2 * (tid + 256 * k));
        }
        istft_walk(tb, z0, z1, tid, a0, a1, spectrum, hop, a0 > 0, carry);
    }
    // the padded hops of the chunk, at the addresses and with the 8-byte stores of the real ones
    for (int a = a0 > a1 ? a0 : a1; a < ac; ++a) zero_hop(o + (size_t)(a - f0) * HOPS, tid);
    if (last) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            *reinterpret_cast<float2*>(carry_out + (size_t)r * HOPS + 2 * (tid + 256 * k)) = onward ? carry[k] : make_float2(0.f, 0.f);
    }
}

// When the alive prefix shrinks from Ro to Rn rows between two segments: the surviving rows' time-axis state - eight slabs, each a prefix of
// n4 = Rn * K * 16 float4 at the old pitch of Ro * K * 16 - and their overlap-add tail (one prefix of c4 = Rn * 256 float4) move from the
// carry set the finished segment wrote into the one it read, packed at the new pitch.
__global__ __launch_bounds__(256) void long_compact_kernel(const float4* __restrict__ state_src, float4* __restrict__ state_dst, size_t pitch_src, size_t n4,
                                                           const float4* __restrict__ carry_src, float4* __restrict__ carry_dst, size_t c4)
{
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < 8 * n4 + c4; i += step) {
        if (i < 8 * n4) { const size_t slab = i / n4; state_dst[i] = state_src[slab * pitch_src + (i - slab * n4)]; }
        else carry_dst[i - 8 * n4] = carry_src[i - 8 * n4];
    }
}

void launch_stft_ragged_segment(const FftTables& tb, const float* wave, int64_t stride, const int64_t* lens, float* X, int Ri, int ta, int te, hipStream_t s)
{
    const Chunks ch = chunks_for<stft_ragged_segment_kernel>(te - ta, Ri, 0);
    hipLaunchKernelGGL(stft_ragged_segment_kernel, ch.grid, dim3(256), 0, s, tb, wave, X, stride, lens, ta, te, ch.len);
}
void launch_istft_ragged_segment(const FftTables& tb, const float* Y, float* out, int64_t out_stride, const int64_t* lens, const float* carry_in,
                                 float* carry_out, int R, int Ri, int ta, int te, hipStream_t s)
{
    const int hops = te - ta - (carry_in ? 0 : 1);                     // 0: a one-frame first segment (one workgroup per row leaves the carry)
    const Chunks ch = chunks_for<istft_ragged_segment_kernel>(hops > 0 ? hops : 1, R, 1);
    hipLaunchKernelGGL(istft_ragged_segment_kernel, ch.grid, dim3(256), 0, s, tb, Y, out, out_stride, lens, carry_in, carry_out, ta, te, Ri, ch.len);
}
void launch_long_compact(const float* state_src, float* state_dst, const float* carry_src, float* carry_dst, int R_old, int R_new, int K, hipStream_t s)
{
    const size_t n4 = (size_t)R_new * K * (HID / 4), c4 = (size_t)R_new * (HOPS / 4), total = 8 * n4 + c4;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(long_compact_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4*>(state_src), reinterpret_cast<float4*>(state_dst),
                       (size_t)R_old * K * (HID / 4), n4, reinterpret_cast<const float4*>(carry_src), reinterpret_cast<float4*>(carry_dst), c4);
}

// ------------------------------------------------------------------------------ long FIR convolution of ragged rows (bsrnn_convolve_ragged)
// Uniformly partitioned overlap-save on the 2048-point transform above (the definition and the plan: convolve_host.h): a rectangular-window
// analysis walk at hop 1024 with zeros outside the row, a complex multiply-accumulate per bin over the filter's partitions, and a synthesis
// walk that keeps the second half of every inverse frame.  Spectra are plain rows of 1025 (re, im) pairs (tb.colmap = null, CONV_LD floats).
// Every kernel finds its row in a table of ConvRow on the device; what a row computes depends on that entry alone, so a row has the same
// bits in every batch, group and launch shape.
//
// Analysis: stft_walk without the window.  sample2(t, c) = complex sample c of frame t, row(t) = where its spectrum goes.
template <class SAMPLE2, class ROW>
__device__ __forceinline__ void fir_analysis_walk(const FftTables& tb, float2* z0, float2* z1, int tid, int t0, int t1, SAMPLE2 sample2, ROW row)
{
    const Twiddles twd = load_twiddles<false>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, false);
    float2 raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = sample2(t0, tid + 256 * k);
    for (int t = t0; t < t1; ++t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) z0[tid + 256 * k] = raw[k];
        __syncthreads();
        raw[0] = raw[2]; raw[1] = raw[3];
        { const int tn = t + 1 < t1 ? t + 1 : t; raw[2] = sample2(tn, tid + 512); raw[3] = sample2(tn, tid + 768); }      // (after the last frame a dummy reload)
        const float2* Z = fft1024<false>(z0, z1, twd, tid);
        rfft_split_store(Z, spl, row(t), tid);
        __syncthreads();                          // Z (= z1) is overwritten by the next frame's first pass
    }
}

// frames [f0 + chunk, ...) of a row: frame t holds x[(t - 1) 1024, (t + 1) 1024), zeros outside [0, n)
__global__ __launch_bounds__(256, FFT_OCC_STFT) void fir_analysis_kernel(FftTables tb, const ConvRow* __restrict__ rows, int row0, const float* __restrict__ in,
                                                                         int64_t in_stride, float* __restrict__ X, int sch)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = row0 + blockIdx.y;
    const ConvRow q = rows[r];
    const int t0 = q.f0 + blockIdx.x * sch;
    const int t1 = (t0 + sch < q.f0 + q.nx) ? t0 + sch : q.f0 + q.nx;
    if (!q.H || t0 >= t1) return;                                     // (uniform over the workgroup, before any barrier)
    const float* src = in + (size_t)r * in_stride;
    const int64_t n = q.n;
    auto sample2 = [&](int t, int c) {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t idx = (int64_t)(t - 1) * HOPS + 2 * c + e;
            v[e] = (idx >= 0 && idx < n) ? src[idx] : 0.f;
        }
        return make_float2(v[0], v[1]);
    };
    auto row = [&](int t) { return X + (size_t)(q.xoff + (t - q.f0)) * CONV_LD; };
    fir_analysis_walk(tb, z0, z1, tid, t0, t1, sample2, row);
}

// The filter image: partition p of g[i] = h[k - 1 - i], zero-padded to 2048, through the same walk (one frame per workgroup: a partition's
// second half is zeros, not the next partition's first half).
__global__ __launch_bounds__(256, FFT_OCC_STFT) void fir_taps_kernel(FftTables tb, const float* __restrict__ h, int k, float* __restrict__ H)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    auto sample2 = [&](int t, int c) {
        float v[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = t * HOPS + 2 * c + e;
            v[e] = (c < 512 && i < k) ? h[k - 1 - i] : 0.f;
        }
        return make_float2(v[0], v[1]);
    };
    auto row = [&](int t) { return H + (size_t)t * CONV_LD; };
    fir_analysis_walk(tb, z0, z1, tid, p, p + 1, sample2, row);
}

// Multiply-accumulate: Y[u][f] = sum_p H[p][f] X[u - p][f] over the partitions whose frame the row has (conv_span), p ascending.  One thread
// owns one bin of TL consecutive blocks: their accumulators and the TL frames X[u - p] of the current p stay in registers, and a step to
// p + 1 brings one new frame in (the window moves down by one), so every H and X value fetched is used TL times; loads are coalesced along
// the bins.  The window is a ring whose phase is the unrolled step number - no register is moved.  The four fused multiply-adds of a complex
// product are spelled out, so a block's sum is the same chain of roundings wherever the block sits in a tile.
template <int TL>
__global__ __launch_bounds__(256) void fir_mac_kernel(const ConvRow* __restrict__ rows, int row0, const float* __restrict__ X, float* __restrict__ Y)
{
    const ConvRow q = rows[row0 + blockIdx.z];
    const int b0 = blockIdx.x * TL;                                   // the tile's first block, counted from u0
    const int f = blockIdx.y * 256 + threadIdx.x;
    if (!q.H || b0 >= q.nb || f > 1024) return;
    const int nt = q.nb - b0 < TL ? q.nb - b0 : TL;
    const int ut = q.u0 + b0, f1 = q.f0 + q.nx - 1;
    const int p_lo = ut - f1 > 0 ? ut - f1 : 0;
    const int p_hi = ut + nt - 1 < q.P - 1 ? ut + nt - 1 : q.P - 1;
    const float2* __restrict__ Xr = reinterpret_cast<const float2*>(X + (size_t)q.xoff * CONV_LD) + f;
    const float2* __restrict__ Hf = reinterpret_cast<const float2*>(q.H) + f;
    auto frame = [&](int v) {                                         // X[v][f], zero for a frame the row does not have (uniform)
        return (v >= q.f0 && v <= f1) ? Xr[(size_t)(v - q.f0) * (CONV_LD / 2)] : make_float2(0.f, 0.f);
    };
    float2 acc[TL], ring[TL];
#pragma unroll
    for (int j = 0; j < TL; ++j) { acc[j] = make_float2(0.f, 0.f); ring[j] = frame(ut + j - p_lo); }
    // step s of a pass: the frame of output j is ring[(j - s) mod TL]; the frame that enters replaces the one output TL - 1 used
    auto pass = [&](int p, auto full) {
#pragma unroll
        for (int s = 0; s < TL; ++s) {
            if (!decltype(full)::value && p + s > p_hi) break;
            const float2 h = Hf[(size_t)(p + s) * (CONV_LD / 2)];
            const float2 fresh = frame(ut - (p + s) - 1);
#pragma unroll
            for (int j = 0; j < TL; ++j) {
                const float2 w = ring[(j - s + TL) % TL];
                acc[j].x = fmaf(-h.y, w.y, fmaf(h.x, w.x, acc[j].x));
                acc[j].y = fmaf(h.y, w.x, fmaf(h.x, w.y, acc[j].y));
            }
            ring[(2 * TL - 1 - s) % TL] = fresh;
        }
    };
    int p = p_lo;
    for (; p + TL - 1 <= p_hi; p += TL) pass(p, std::true_type());
    if (p <= p_hi) pass(p, std::false_type());
    float2* __restrict__ Yr = reinterpret_cast<float2*>(Y + (size_t)(q.yoff + b0) * CONV_LD) + f;
#pragma unroll
    for (int j = 0; j < TL; ++j)
        if (j < nt) Yr[(size_t)j * (CONV_LD / 2)] = acc[j];
}

// Synthesis: istft_walk without window, envelope and overlap.  Block u of the row is the second half of irfft(Y[u]) and goes to
// out[u 1024 - shift ...], clipped to [0, n): 8-byte stores where the block lies inside the row at an 8-byte boundary (an odd shift, or a
// caller's row at an odd float, has none), single floats elsewhere.  A copied row (H = null) moves its pieces of 1024 samples instead.
__global__ __launch_bounds__(256, FFT_OCC_ISTFT) void fir_synthesis_kernel(FftTables tb, const ConvRow* __restrict__ rows, int row0, const float* __restrict__ Y,
                                                                           const float* __restrict__ in, int64_t in_stride, float* __restrict__ out,
                                                                           int64_t out_stride, int ich)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    const int tid = threadIdx.x;
    const int r = row0 + blockIdx.y;
    const ConvRow q = rows[r];
    const int b0 = blockIdx.x * ich;
    const int b1 = (b0 + ich < q.nb) ? b0 + ich : q.nb;
    if (b0 >= b1) return;                                             // (uniform over the workgroup, before any barrier)
    float* o = out + (size_t)r * out_stride;
    const int64_t n = q.n;
    if (!q.H) {
        const float* src = in + (size_t)r * in_stride;
        for (int b = b0; b < b1; ++b)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = (int64_t)b * HOPS + tid + 256 * k;
                if (i < n) o[i] = src[i];
            }
        return;
    }
    const Twiddles twd = load_twiddles<true>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, true);
    const float sc = 1.0f / 1024.0f;
    const float* Yr = Y + (size_t)q.yoff * CONV_LD;
    MergeRegs mr;
    irfft_load<false>(Yr + (size_t)b0 * CONV_LD, spl, mr, tid);
    for (int b = b0; b < b1; ++b) {
        irfft_store<true>(mr, spl, z0, tid);
        __syncthreads();
        irfft_load<false>(Yr + (size_t)(b + 1 < b1 ? b + 1 : b) * CONV_LD, spl, mr, tid);      // (after the last block: a dummy reload)
        const float2* z = fft1024<true>(z0, z1, twd, tid);
        const int64_t m0 = (int64_t)(q.u0 + b) * HOPS - q.shift;
        const bool pairs = m0 >= 0 && m0 + HOPS <= n && (reinterpret_cast<size_t>(o + m0) & 7) == 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = tid + 256 * k;
            const float2 v = make_float2(z[c + 512].x * sc, z[c + 512].y * sc);
            const int64_t m = m0 + 2 * c;
            if (pairs) *reinterpret_cast<float2*>(o + m) = v;
            else {
                if (m >= 0 && m < n) o[m] = v.x;
                if (m + 1 >= 0 && m + 1 < n) o[m + 1] = v.y;
            }
        }
        __syncthreads();                          // z (= z1) is overwritten by the next block's first pass
    }
}

static FftTables fir_tables(const FftTables& tb)
{
    FftTables t = tb;
    t.colmap = nullptr;
    t.ld = CONV_LD;
    return t;
}
void launch_fir_taps(const FftTables& tb, const float* taps, int k, float* H, hipStream_t s)
{
    hipLaunchKernelGGL(fir_taps_kernel, dim3(conv_partitions(k)), dim3(256), 0, s, fir_tables(tb), taps, k, H);
}
void launch_fir_group(const FftTables& tb, const ConvRow* rows, int row0, int n_rows, int max_nx, int max_nb, const float* in, int64_t in_stride,
                      float* out, int64_t out_stride, float* X, float* Y, hipStream_t s)
{
    const FftTables t = fir_tables(tb);
    if (max_nx > 0) {
        const Chunks ca = chunks_for<fir_analysis_kernel>(max_nx, n_rows, 0);
        hipLaunchKernelGGL(fir_analysis_kernel, ca.grid, dim3(256), 0, s, t, rows, row0, in, in_stride, X, ca.len);
        const dim3 grid((unsigned)((max_nb + CONV_TILE - 1) / CONV_TILE), 5, (unsigned)n_rows);      // 5 x 256 threads: the 1025 bins
        hipLaunchKernelGGL(fir_mac_kernel<CONV_TILE>, grid, dim3(256), 0, s, rows, row0, X, Y);
    }
    const Chunks cs = chunks_for<fir_synthesis_kernel>(max_nb, n_rows, 0);
    hipLaunchKernelGGL(fir_synthesis_kernel, cs.grid, dim3(256), 0, s, t, rows, row0, Y, in, in_stride, out, out_stride, cs.len);
}

// ------------------------------------------------------------------------------ the streaming form (bsrnn_fir_stream_*)
// The same scheme walked in stream order (convolve_stream_host.h): ONE launch per call, one workgroup per row, which walks the row's
// blocks [ub, ue) one after the other - the frame (the previous 1024 inputs, the FIFO, the call's input, zeros behind a flushed row's end)
// through fir_analysis_walk into slot u mod P of the row's ring, the multiply-accumulate over the ring with a thread per bin (bins
// tid + 256 i and, in every thread, bin 1024: no divergent tail), the sum through LDS into the synthesis of fir_synthesis_kernel, clipped
// stores, and at the end the tail and the FIFO brought up to date.  The fused multiply-adds are fir_mac_kernel's, partitions ascending from
// the first whose frame exists, so a block has the one-shot's bits (a frame the one-shot takes as zeros leaves its accumulator at +0).
// The hot case is a tick (many rows, one block each); a call that brings a row many blocks is correct and serial.
// The ring is read back by other threads of the workgroup than wrote it: the barrier that ends the analysis walk orders the two (no
// __restrict__ on ring, tail and FIFO).
__global__ __launch_bounds__(256) void fir_stream_kernel(FftTables tb, const FirStreamRow* __restrict__ rows, const float* __restrict__ in, int64_t in_stride,
                                                         float* __restrict__ out, int64_t out_stride, float* ring, int64_t ring_stride, float* state)
{
    __shared__ __attribute__((aligned(16))) float2 z0[1024], z1[1024];
    __shared__ __attribute__((aligned(16))) float2 ys[1028];
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const FirStreamRow q = rows[r];
    if (q.n_in == 0 && q.ub >= q.ue) return;                          // held (uniform over the workgroup, before any barrier)
    const float* src = in + (size_t)r * in_stride;
    float* o = out + (size_t)r * out_stride;
    if (!q.H) {                                                       // bypass: the samples it was given, in the same call
        for (int i = tid; i < q.n_in; i += 256) o[i] = src[i];
        return;
    }
    float* rg = ring + (size_t)r * ring_stride;
    float* tl = state + (size_t)r * FIR_STREAM_ROW_FLOATS;            // x[base - 1024, base)
    float* ff = tl + CONV_B;                                          // x[base, N0)
    const int64_t N0 = q.N0, N1 = q.N0 + q.n_in;
    const int64_t base = N0 / CONV_B * CONV_B;
    // sample i >= base - 1024 of the stream; zeros in front of it and behind what it has taken
    auto sample = [&](int64_t i) -> float {
        if (i < 0 || i >= N1) return 0.f;
        if (i >= N0) return src[i - N0];
        if (i >= base) return ff[i - base];
        return tl[i - (base - CONV_B)];
    };
    const Twiddles twd = load_twiddles<true>(tb.tw1024, tid);
    const SplitCtx spl = load_split(tb, tid, true);
    const float sc = 1.0f / 1024.0f;
    const int P = q.P;
    const float2* Hf = reinterpret_cast<const float2*>(q.H);
    const float2* Rf = reinterpret_cast<const float2*>(rg);
    for (int64_t u = q.ub; u < q.ue; ++u) {
        if (u <= q.f1) {
            auto sample2 = [&](int, int c) {
                const int64_t i = (u - 1) * CONV_B + 2 * c;
                return make_float2(sample(i), sample(i + 1));
            };
            auto row = [&](int) { return rg + (size_t)(u % P) * CONV_LD; };
            fir_analysis_walk(tb, z0, z1, tid, 0, 1, sample2, row);   // (ends with a barrier: the spectrum is in the ring for everyone)
        }
        if (u < q.u0) continue;
        const int p_lo = u - q.f1 > 0 ? (int)(u - q.f1) : 0;
        const int p_hi = u < P - 1 ? (int)u : P - 1;
        float2 acc[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) acc[i] = make_float2(0.f, 0.f);
        int slot = (int)((u - p_lo) % P);
#pragma unroll 2
        for (int p = p_lo; p <= p_hi; ++p) {
            const float2* hp = Hf + (size_t)p * (CONV_LD / 2);
            const float2* xp = Rf + (size_t)slot * (CONV_LD / 2);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int f = i < 4 ? tid + 256 * i : 1024;
                const float2 h = hp[f], w = xp[f];
                acc[i].x = fmaf(-h.y, w.y, fmaf(h.x, w.x, acc[i].x));
                acc[i].y = fmaf(h.y, w.x, fmaf(h.x, w.y, acc[i].y));
            }
            slot = slot == 0 ? P - 1 : slot - 1;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) ys[i < 4 ? tid + 256 * i : 1024] = acc[i];
        __syncthreads();
        MergeRegs mr;
        irfft_load<true>(reinterpret_cast<const float*>(ys), spl, mr, tid);
        irfft_store<true>(mr, spl, z0, tid);
        __syncthreads();
        const float2* z = fft1024<true>(z0, z1, twd, tid);
        const int64_t m0 = u * CONV_B - q.shift;
        float* ob = o + (m0 - q.E0);                                  // (dereferenced inside the clip only)
        const bool pairs = m0 >= 0 && m0 + CONV_B <= q.n_end && (reinterpret_cast<size_t>(ob) & 7) == 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = tid + 256 * k;
            const float2 v = make_float2(z[c + 512].x * sc, z[c + 512].y * sc);
            const int64_t m = m0 + 2 * c;
            if (pairs) *reinterpret_cast<float2*>(ob + 2 * c) = v;
            else {
                if (m >= 0 && m < q.n_end) ob[2 * c] = v.x;
                if (m + 1 >= 0 && m + 1 < q.n_end) ob[2 * c + 1] = v.y;
            }
        }
        __syncthreads();                          // z (= z1), z0 and ys are written again by the next block
    }
    if (!q.keep) return;
    // the state behind the call: everything is read before anything is written (the new tail may come out of the old FIFO)
    const int64_t base1 = N1 / CONV_B * CONV_B;
    float tv[4], fv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = tid + 256 * k;
        tv[k] = base1 != base ? sample(base1 - CONV_B + j) : 0.f;
        fv[k] = sample(base1 + j);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = tid + 256 * k;
        if (base1 != base) tl[j] = tv[k];
        ff[j] = fv[k];
    }
}

void launch_fir_stream(const FftTables& tb, const FirStreamRow* rows, int C, const float* in, int64_t in_stride, float* out, int64_t out_stride,
                       float* ring, int64_t ring_stride, float* state, hipStream_t s)
{
    hipLaunchKernelGGL(fir_stream_kernel, dim3((unsigned)C), dim3(256), 0, s, fir_tables(tb), rows, in, in_stride, out, out_stride, ring, ring_stride, state);
}

}  // namespace bsrnn
