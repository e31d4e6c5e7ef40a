// Validation arithmetic of the reference's `train_infer` / `infer.py` report on device-resident signals:
// L1 tri-loss, SDR, the reference's "input SDR", SI-SDR and the "Separation dB" figure
// (m_dataset.py:202-226, infer.py:44-47).  Pure HBM-bound reductions: every kernel reads its operands once
// with 16-byte loads, accumulates the fp32 products in double per thread, reduces wave-wide with DPP shuffles
// and leaves one partial per workgroup; the host adds the (few hundred) partials in a fixed order, so the
// result does not depend on the launch.
#include "kernels.h"

namespace bsrnn {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

// ADD: the workgroup's sums are added to what dst holds (read, add, store: dst is this workgroup's alone) instead of replacing it
template <int NQ, bool ADD = false>
__device__ __forceinline__ void block_reduce_store(double (&q)[NQ], double* dst)
{
    __shared__ double sh[4][NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) q[i] += __shfl_down(q[i], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NQ; ++i) sh[wave][i] = q[i];
    __syncthreads();
    if (threadIdx.x < NQ) {
        const double v = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
        dst[threadIdx.x] = ADD ? dst[threadIdx.x] + v : v;
    }
}

// ------------------------------------------------------------------------------ the validation sums of a batch of clips (bsrnn_evaluate*)
// One family for the three evaluate calls.  A batch is R rows inside the rectangle R x Tmax that the separation ran on: row r holds lens[r]
// samples and T_r = 1 + lens[r] / 1024 frames; a clip is a run of consecutive rows of one length, and nothing is summed across clips.
// bsrnn_evaluate's rectangle is the batch of one clip whose R lengths are equal.  The row (or the clip) belongs to the workgroup, so every
// bound below is workgroup-uniform and each loop runs over the real samples / frames only, with no length test inside it.  The two bodies
// below are shared by the whole-batch kernels, which leave one partial per workgroup (every slot of a grid's partials is written - a
// workgroup that starts past its row's end stores zeros - so the host adds whole arrays whatever an earlier call left there), and by the
// segment kernels further down, which add into the call's accumulators.

// This workgroup's share of the seven sums over n samples of one row (x the estimate, s the clean signal, m the mixture; n a multiple of
// 1024): q = sum s^2, sum (x-s)^2, sum x*s, sum x^2, sum |x-s|, sum m^2, sum (m-x)^2.  vec: the three pointers are 16-byte aligned and the
// samples go by 16-byte loads, otherwise by scalar loads; a thread visits its samples in index order either way.
__device__ __forceinline__ void time_sums(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ m, int64_t n,
                                          int vec, double (&q)[METRIC_TIME_Q])
{
    auto one = [&](float xv, float sv, float mv) {
        const float d = xv - sv, e = mv - xv;          // fp32 differences, as the reference forms them
        q[0] += (double)sv * sv; q[1] += (double)d * d; q[2] += (double)xv * sv; q[3] += (double)xv * xv;
        q[4] += (double)__builtin_fabsf(d); q[5] += (double)mv * mv; q[6] += (double)e * e;
    };
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const v4f xv = *reinterpret_cast<const v4f*>(x + 4 * i);
        const v4f sv = *reinterpret_cast<const v4f*>(s + 4 * i);
        const v4f mv = *reinterpret_cast<const v4f*>(m + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) one(xv[j], sv[j], mv[j]);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) one(x[i], s[i], m[i]);
}

// This workgroup's share of the spectral L1 terms over `frames` frame rows of two frame-major band-padded spectra (y, s: their first frame
// row, rows ld floats apart; bin k at columns colmap[k] (re), +1 (im)): q = sum |re diff|, sum |im diff|
__device__ __forceinline__ void freq_sums(const float* __restrict__ y0, const float* __restrict__ s0, const int* __restrict__ colmap, int ld,
                                          int frames, double (&q)[2])
{
    for (int t = blockIdx.x; t < frames; t += gridDim.x) {
        const float* y = y0 + (size_t)t * ld;
        const float* s = s0 + (size_t)t * ld;
        for (int k = threadIdx.x; k < NBINS; k += 256) {
            const int c = colmap[k];
            const float2 yv = *reinterpret_cast<const float2*>(y + c), sv = *reinterpret_cast<const float2*>(s + c);
            q[0] += (double)__builtin_fabsf(yv.x - sv.x);
            q[1] += (double)__builtin_fabsf(yv.y - sv.y);
        }
    }
}

// grid (chunks of Tmax, R).  est rows out_stride floats apart; speech, mix rows wave_stride floats apart, row r's first
// n_est_r = (lens[r] / 1024) * 1024 samples used (m_dataset.py:198).  part [R][chunks][7]
__global__ __launch_bounds__(256) void metric_time_ragged_kernel(const float* __restrict__ est, const float* __restrict__ speech,
                                                                 const float* __restrict__ mix, const int64_t* __restrict__ lens,
                                                                 int64_t out_stride, int64_t wave_stride, int vec, double* __restrict__ part)
{
    const int r = blockIdx.y;
    const int64_t n_est = lens[r] / HOPS * HOPS;
    double q[METRIC_TIME_Q] = {0, 0, 0, 0, 0, 0, 0};
    // vec: every row of the three signals starts 16-byte aligned (the host checks the bases and wave_stride % 4; out_stride and n_est are
    // multiples of 1024), otherwise scalar loads - an odd stride puts every other row off alignment
    time_sums(est + (size_t)r * out_stride, speech + (size_t)r * wave_stride, mix + (size_t)r * wave_stride, n_est, vec, q);
    block_reduce_store<METRIC_TIME_Q>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * METRIC_TIME_Q);
}

// SI-SDR second pass (torchmetrics scale_invariant_signal_distortion_ratio, zero_mean = False), grid as above: with the row's alpha,
// sum (alpha s)^2 and sum (alpha s - x)^2, the products formed in fp32 like the reference's tensors.  The row's alpha is formed here, by
// every workgroup of the row, from the row's time partials (time_part [R][chunks][7], the launch in front of this one on the stream): added
// in index order in double, then ((float) sum x s + eps) / ((float) sum s^2 + eps) in fp32, eps = float32 machine epsilon - what
// metrics_host.h::sisdr_sums_from_totals forms on the host - so no call needs a round trip in its middle.
// part [R][chunks][2]
__global__ __launch_bounds__(256) void metric_sisdr_ragged_kernel(const float* __restrict__ est, const float* __restrict__ speech,
                                                                  const int64_t* __restrict__ lens, int64_t out_stride, int64_t wave_stride,
                                                                  const double* __restrict__ time_part, double* __restrict__ part)
{
    const int r = blockIdx.y;
    const int64_t n_est = lens[r] / HOPS * HOPS;
    const float* x = est + (size_t)r * out_stride;
    const float* s = speech + (size_t)r * wave_stride;
    const double* tp = time_part + (size_t)r * gridDim.x * METRIC_TIME_Q;
    double ss = 0, xs = 0;
    for (unsigned ch = 0; ch < gridDim.x; ++ch) { ss += tp[ch * METRIC_TIME_Q + 0]; xs += tp[ch * METRIC_TIME_Q + 2]; }
    const float eps = 1.1920928955078125e-07f;
    const float a = ((float)xs + eps) / ((float)ss + eps);
    double q[2] = {0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_est; i += (int64_t)gridDim.x * 256) {
        const float ts = a * s[i], nz = ts - x[i];
        q[0] += (double)ts * ts; q[1] += (double)nz * nz;
    }
    block_reduce_store<2>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * 2);
}

// The reference's `sdr2` (m_dataset.py:219-222) per clip, grid (blocks, clips): its sample tensors still carry the DataLoader's batch
// dimension ([1, rows, n]), so `dim=1` sums over the ROWS, not over time - one ratio per sample position i < len of the clip, averaged over
// the positions.  Kept as written.  The two sums run over the clip's own rows (all of that length), never over another clip's.
// part [clips][blocks]
__global__ __launch_bounds__(256) void metric_input_sdr_ragged_kernel(const float* __restrict__ speech, const float* __restrict__ mix,
                                                                      const MetricClip* __restrict__ clips, int64_t wave_stride,
                                                                      double* __restrict__ part)
{
    const MetricClip k = clips[blockIdx.y];
    const float* sp = speech + (size_t)k.first * wave_stride;
    const float* mp = mix + (size_t)k.first * wave_stride;
    double q[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < k.len; i += (int64_t)gridDim.x * 256) {
        float a = 0.f, b = 0.f;
        for (int r = 0; r < k.rows; ++r) {
            const float sv = sp[(size_t)r * wave_stride + i], d = sv - mp[(size_t)r * wave_stride + i];
            a += sv * sv; b += d * d;
        }
        q[0] += 10.0 * log10((double)(a + 1e-9f) / (double)(b + 1e-9f));
    }
    block_reduce_store<1>(q, part + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// Spectral L1 terms per row, grid (blocks, R): frame rows m = r * Tmax + t, t < T_r only - the padded frames are zero rows in both spectra
// (stft_ragged_kernel writes them so, the mask stage returns them so) and are not read.  part [R][blocks][2]
__global__ __launch_bounds__(256) void metric_freq_ragged_kernel(const float* __restrict__ Yf, const float* __restrict__ Sf,
                                                                 const int* __restrict__ colmap, int ld, const int64_t* __restrict__ lens,
                                                                 int Tmax, double* __restrict__ part)
{
    const int r = blockIdx.y;
    const int Tr = 1 + (int)(lens[r] / HOPS);
    double q[2] = {0, 0};
    freq_sums(Yf + (size_t)r * Tmax * ld, Sf + (size_t)r * Tmax * ld, colmap, ld, Tr, q);
    block_reduce_store<2>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * 2);
}

// ------------------------------------------------------------------------------ the family's segment kernels (bsrnn_evaluate_long_ragged)
// time_sums and freq_sums over one segment.  A batch cut into segments of frames [ta, te) (plan_host.h: ragged_long_plan, segment_owned): a segment's estimate and its spectrum
// exist only until the next segment runs, so a row's sums are formed from one launch per segment.  acc [R][METRIC_SEG_SLOTS][NQ] are the
// call's accumulators, zeroed once at its start: workgroup (slot, row) of every segment's launch adds its sum into slot (row, slot), which
// is its alone - read, add, store, no atomics - and the segments follow each other on one stream, so the order of a slot's additions is
// fixed and a call gives the same bits every time.  A workgroup with nothing to do in a segment leaves its slot alone.  Row and slot belong
// to the workgroup: every bound is workgroup-uniform, and the loops run over the row's own samples / frames only.

// grid (METRIC_SEG_SLOTS, Ri).  est points at the segment's first hop of row 0 (rows est_stride floats apart: the call's result, or a buffer
// of one segment); speech, mix are the call's, read at the clip position.  The hops the segment completes and that are the row's own.
__global__ __launch_bounds__(256) void metric_time_ragged_segment_kernel(const float* __restrict__ est, int64_t est_stride,
                                                                         const float* __restrict__ speech, const float* __restrict__ mix,
                                                                         const int64_t* __restrict__ lens, int64_t wave_stride, int ta, int te,
                                                                         int vec, double* __restrict__ acc)
{
    const int r = blockIdx.y;
    const SegmentOwned own = segment_owned(ta, te, 1 + (int)(lens[r] / HOPS));
    const int64_t n = (int64_t)own.hops * HOPS;                       // a multiple of 1024: the 16-byte loads leave no tail
    const int64_t first = (int64_t)blockIdx.x * 256 * (vec ? 4 : 1);  // the first sample of this workgroup's first thread
    if (first >= n) return;
    double q[METRIC_TIME_Q] = {0, 0, 0, 0, 0, 0, 0};
    time_sums(est + (size_t)r * est_stride, speech + (size_t)r * wave_stride + (size_t)own.hop0 * HOPS,
              mix + (size_t)r * wave_stride + (size_t)own.hop0 * HOPS, n, vec, q);
    block_reduce_store<METRIC_TIME_Q, true>(q, acc + ((size_t)r * gridDim.x + blockIdx.x) * METRIC_TIME_Q);
}

// grid (METRIC_SEG_SLOTS, Ri).  Yf, Sf: the segment's spectra, segment-local rows (r * (te - ta) + (t - ta)) * ld; the row's own frames of
// the segment.
__global__ __launch_bounds__(256) void metric_freq_ragged_segment_kernel(const float* __restrict__ Yf, const float* __restrict__ Sf,
                                                                         const int* __restrict__ colmap, int ld, const int64_t* __restrict__ lens,
                                                                         int ta, int te, double* __restrict__ acc)
{
    const int r = blockIdx.y;
    const SegmentOwned own = segment_owned(ta, te, 1 + (int)(lens[r] / HOPS));
    if ((int)blockIdx.x >= own.frames) return;
    double q[2] = {0, 0};
    freq_sums(Yf + (size_t)r * (te - ta) * ld, Sf + (size_t)r * (te - ta) * ld, colmap, ld, own.frames, q);
    block_reduce_store<2, true>(q, acc + ((size_t)r * gridDim.x + blockIdx.x) * 2);
}

// ------------------------------------------------------------------------------ the tri-loss of a ragged training step, forward and backward
// bsrnn_train_loss_ragged: per clip, L1(x_time, s_time) + L1(Re Y, Re S) + L1(Im Y, Im S) and the `sdr` of train_infer (m_dataset.py:202-217),
// on the tensors autograd holds - y, s [R][2050][Tmax] in the reference layout (T innermost), x_time [R][(Tmax-1)*1024], speech rows
// wave_stride floats apart.  Row r has T_r frames and n_est_r samples of its own; what the rectangle holds behind them (zeros from the ragged
// DSP, or anything) may travel inside a 16-byte load but never reaches a sum or a gradient: it is SELECTED away, never multiplied by a mask.
// The row belongs to the workgroup, so the bounds are workgroup-uniform.  Partials as above: fp32 differences, double sums, one partial per
// workgroup in a fixed order; train_loss_finish_kernel adds them per clip in index order, so the values are bit-reproducible and stay on the
// device.

// Time terms, grid (chunks, R) as metric_time_ragged_kernel: part [R][chunks][3] = sum s^2, sum (x-s)^2, sum |x-s| over i < n_est_r
constexpr int TRAIN_TIME_Q = 3;
__global__ __launch_bounds__(256) void train_loss_time_ragged_kernel(const float* __restrict__ xtime, const float* __restrict__ speech,
                                                                     const int64_t* __restrict__ lens, int64_t out_stride, int64_t wave_stride,
                                                                     int vec, double* __restrict__ part)
{
    const int r = blockIdx.y;
    const int64_t n_est = lens[r] / HOPS * HOPS;
    const float* x = xtime + (size_t)r * out_stride;
    const float* s = speech + (size_t)r * wave_stride;
    double q[TRAIN_TIME_Q] = {0, 0, 0};
    auto one = [&](float xv, float sv) {
        const float d = xv - sv;
        q[0] += (double)sv * sv; q[1] += (double)d * d; q[2] += (double)__builtin_fabsf(d);
    };
    // vec: every row of both signals starts 16-byte aligned (the host checks the bases and wave_stride % 4; out_stride and n_est are
    // multiples of 1024, so no vector straddles a row's end)
    const int64_t n4 = vec ? n_est / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const v4f xv = *reinterpret_cast<const v4f*>(x + 4 * i);
        const v4f sv = *reinterpret_cast<const v4f*>(s + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) one(xv[j], sv[j]);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_est; i += (int64_t)gridDim.x * 256) one(x[i], s[i]);
    block_reduce_store<TRAIN_TIME_Q>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * TRAIN_TIME_Q);
}

// A workgroup's share of one row of a [R][2050][Tmax] tensor: the interleaved columns [f0, f0 + nf) - a contiguous span of n = nf * Tmax
// floats at `base`.  Visits every element once, in a fixed order per thread: scalars up to the first 16-byte boundary, then whole vectors
// (four(j): elements j .. j + 3), then the scalar tail.  vec = 0: scalars only.  n < 2^31 (the launcher picks nf so).
template <class F4, class F1>
__device__ __forceinline__ void walk_span(size_t base, int n, int vec, F4 four, F1 one)
{
    int head = vec ? (int)((4 - (base & 3)) & 3) : n;
    if (head > n) head = n;
    // (the loop vectorizer is kept off the scalar loops: it turns two iterations of a gradient into packed fp32, which a kernel without
    // MFMA must not contain - tests/test_code_audit.py)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int j = threadIdx.x; j < head; j += 256) one(j);
    const int n4 = (n - head) / 4;
    for (int i = threadIdx.x; i < n4; i += 256) four(head + 4 * i);
#pragma clang loop vectorize(disable) interleave(disable)
    for (int j = head + 4 * n4 + threadIdx.x; j < n; j += 256) one(j);
}

// Spectral terms, grid (FB, R), nf columns per workgroup: part [R][FB][2] = sum |Re Y - Re S|, sum |Im Y - Im S| over bins x frames t < T_r
// (an even interleaved column is a real part, an odd one an imaginary part)
__global__ __launch_bounds__(256) void train_loss_freq_ragged_kernel(const float* __restrict__ y, const float* __restrict__ s,
                                                                     const int64_t* __restrict__ lens, int Tmax, int nf, int vec,
                                                                     double* __restrict__ part)
{
    const int r = blockIdx.y;
    const int Tr = 1 + (int)(lens[r] / HOPS);
    const int f0 = blockIdx.x * nf;
    const int n = (F2 - f0 < nf ? F2 - f0 : nf) * Tmax;
    const size_t base = ((size_t)r * F2 + f0) * Tmax;
    const float* yp = y + base;
    const float* sp = s + base;
    double q[2] = {0, 0};
    auto acc = [&](float yv, float sv, int f, int t) {
        const double d = (double)__builtin_fabsf(yv - sv);
        const bool real = t < Tr, odd = (f0 + f) & 1;
        q[0] += (real && !odd) ? d : 0.0;
        q[1] += (real && odd) ? d : 0.0;
    };
    walk_span(base, n, vec,
              [&](int j) {
                  const v4f yv = *reinterpret_cast<const v4f*>(yp + j);
                  const v4f sv = *reinterpret_cast<const v4f*>(sp + j);
                  int f = j / Tmax, t = j - f * Tmax;
#pragma unroll
                  for (int k = 0; k < 4; ++k) { acc(yv[k], sv[k], f, t); if (++t == Tmax) { t = 0; ++f; } }
              },
              [&](int j) { const int f = j / Tmax; acc(yp[j], sp[j], f, j - f * Tmax); });
    block_reduce_store<2>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * 2);
}

// One thread per clip: the clip's rows in order, each row's partials in index order.  values [n_clips][TV_COUNT] by finish_clip_metrics'
// arithmetic (metrics_host.h); row_sums [R][2] = sum s^2, sum (x-s)^2 of each row, what the backward pass reads.
__global__ __launch_bounds__(64) void train_loss_finish_kernel(const TrainClip* __restrict__ clips, int n_clips, const double* __restrict__ p_time,
                                                               int chunks, const double* __restrict__ p_freq, int FB, double* __restrict__ values,
                                                               double* __restrict__ row_sums)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_clips) return;
    const TrainClip k = clips[c];
    double sdr = 0, l1 = 0, re = 0, im = 0;
    for (int r = 0; r < k.rows; ++r) {
        const size_t row = (size_t)(k.first + r);
        double q[TRAIN_TIME_Q] = {0, 0, 0};
        for (int ch = 0; ch < chunks; ++ch)
            for (int i = 0; i < TRAIN_TIME_Q; ++i) q[i] += p_time[(row * chunks + ch) * TRAIN_TIME_Q + i];
        row_sums[row * 2] = q[0];
        row_sums[row * 2 + 1] = q[1];
        sdr += 10.0 * log10((q[0] + 1e-9) / (q[1] + 1e-9));
        l1 += q[2];
        double a = 0, b = 0;
        for (int i = 0; i < FB; ++i) { a += p_freq[(row * FB + i) * 2]; b += p_freq[(row * FB + i) * 2 + 1]; }
        re += a; im += b;
    }
    const double l1_time = l1 / ((double)k.rows * (double)k.n_est);
    const double l1_re = re / ((double)k.rows * 1025.0 * (double)k.T);
    const double l1_im = im / ((double)k.rows * 1025.0 * (double)k.T);
    double* v = values + (size_t)c * TV_COUNT;
    v[TV_LOSS] = l1_time + l1_re + l1_im;
    v[TV_L1_TIME] = l1_time;
    v[TV_L1_RE] = l1_re;
    v[TV_L1_IM] = l1_im;
    v[TV_SDR] = sdr / k.rows;
}

// d LOSS_c / d y, grid and spans as train_loss_freq_ragged_kernel: dy = gL_c * sgn(y - s) / (rows_c * 1025 * T_c) for t < T_r, else 0
// (sgn(0) = 0, as torch's abs has it); every element of dy is written.  gclip [n_clips][2]: the upstream gradients of LOSS and SDR.
__global__ __launch_bounds__(256) void train_loss_freq_ragged_bwd_kernel(const float* __restrict__ y, const float* __restrict__ s,
                                                                         const int64_t* __restrict__ lens, const TrainClip* __restrict__ clips,
                                                                         const int32_t* __restrict__ row_clip, const float* __restrict__ gclip,
                                                                         int Tmax, int nf, int vec, float* __restrict__ dy)
{
    const int r = blockIdx.y;
    const int Tr = 1 + (int)(lens[r] / HOPS);
    const int c = row_clip[r];
    const float w = (float)((double)gclip[2 * c] * clips[c].inv_freq);
    const int f0 = blockIdx.x * nf;
    const int n = (F2 - f0 < nf ? F2 - f0 : nf) * Tmax;
    const size_t base = ((size_t)r * F2 + f0) * Tmax;
    const float* yp = y + base;
    const float* sp = s + base;
    float* dp = dy + base;
    auto grad = [&](float yv, float sv, int t) {
        const float d = yv - sv;
        const float g = d > 0.f ? w : (d < 0.f ? -w : 0.f);
        return t < Tr ? g : 0.f;
    };
    walk_span(base, n, vec,
              [&](int j) {
                  const v4f yv = *reinterpret_cast<const v4f*>(yp + j);
                  const v4f sv = *reinterpret_cast<const v4f*>(sp + j);
                  int t = j % Tmax;
                  float o[4];
#pragma unroll
                  for (int k = 0; k < 4; ++k) { o[k] = grad(yv[k], sv[k], t); if (++t == Tmax) t = 0; }
                  *reinterpret_cast<float4*>(dp + j) = make_float4(o[0], o[1], o[2], o[3]);
              },
              [&](int j) { dp[j] = grad(yp[j], sp[j], j % Tmax); });
}

// d (gL_c LOSS_c + gS_c SDR_c) / d x_time, grid (chunks, R): for i < n_est_r
//   gL_c sgn(x - s) / (rows_c n_est_c)  -  gS_c (10 / ln 10) 2 (x - s) / (rows_c (sum (x-s)^2_r + 1e-9)),
// zeros from n_est_r to the end of the row (stored, nothing is read there); the two weights are formed once per workgroup in double.
__global__ __launch_bounds__(256) void train_loss_time_ragged_bwd_kernel(const float* __restrict__ xtime, const float* __restrict__ speech,
                                                                         const int64_t* __restrict__ lens, const TrainClip* __restrict__ clips,
                                                                         const int32_t* __restrict__ row_clip, const float* __restrict__ gclip,
                                                                         const double* __restrict__ row_sums, int64_t out_stride,
                                                                         int64_t wave_stride, int vec, float* __restrict__ dx)
{
    const int r = blockIdx.y;
    const int64_t n_est = lens[r] / HOPS * HOPS;
    const int c = row_clip[r];
    const TrainClip k = clips[c];
    const float wl = (float)((double)gclip[2 * c] * k.inv_time);
    const float ws = (float)((double)gclip[2 * c + 1] * (10.0 / 2.302585092994046) * 2.0 / ((double)k.rows * (row_sums[2 * (size_t)r + 1] + 1e-9)));
    const float* x = xtime + (size_t)r * out_stride;
    const float* s = speech + (size_t)r * wave_stride;
    float* o = dx + (size_t)r * out_stride;
    auto grad = [&](float xv, float sv) {
        const float d = xv - sv;
        const float g = d > 0.f ? wl : (d < 0.f ? -wl : 0.f);
        return g - ws * d;
    };
    const int64_t n4 = vec ? n_est / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const v4f xv = *reinterpret_cast<const v4f*>(x + 4 * i);
        const v4f sv = *reinterpret_cast<const v4f*>(s + 4 * i);
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = grad(xv[j], sv[j]);
        *reinterpret_cast<float4*>(o + 4 * i) = make_float4(g[0], g[1], g[2], g[3]);
    }
#pragma clang loop vectorize(disable) interleave(disable)             // (as in walk_span)
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_est; i += (int64_t)gridDim.x * 256) o[i] = grad(x[i], s[i]);
    for (int64_t i = n_est + (int64_t)blockIdx.x * 256 + threadIdx.x; i < out_stride; i += (int64_t)gridDim.x * 256) o[i] = 0.f;
}

// ------------------------------------------------------------------------------ per-hop activity of a ragged batch (bsrnn_hop_activity)
// The two figures the reference's gendataset-separate.py:100-105 forms for every chunk of 1024 samples - mean(est^2 / (mix - est)^2) and
// mean(mix^2) - for hop h < hops[r] of every row r.  One WAVE per hop: 64 lanes x 16 samples of each signal, as four 16-byte loads per
// signal whose lanes lie side by side (load k of lane l: samples k * 256 + 4 l ... + 3).  The fp32 terms are rounded exactly where the
// reference's tensors are - the difference, the two squares, the IEEE division, the square of the mixture; no contraction - and added in
// double: a lane's sixteen in index order, then wave-wide as block_reduce_store's first stage does, and lane 0 stores the two means.
// No LDS and no barrier: a wave depends on nothing outside itself.  Every bound - the row, the hop, the row's hop count - is
// wave-uniform.  Slots from hops[r] to Hmax get (0, 0) and nothing is read for them; nothing is read behind hops[r] * 1024 samples.
// vec = 0: the same samples in the same order by scalar loads, so the two paths agree bit for bit.
// grid (hop groups of ACT_WAVES, rows); hops null: every row has Hmax hops.  act [R][Hmax][2]
constexpr int ACT_WAVES = 4;
__global__ __launch_bounds__(64 * ACT_WAVES) void hop_activity_kernel(const float* __restrict__ mix, int64_t mix_stride,
                                                                      const float* __restrict__ est, int64_t est_stride,
                                                                      const int32_t* __restrict__ hops, int R, int Hmax, int vec,
                                                                      double* __restrict__ act)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t h = (int64_t)blockIdx.x * ACT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (h >= Hmax) return;
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        double* dst = act + ((size_t)r * Hmax + h) * 2;
        const int Hr = hops ? hops[r] : Hmax;
        if (h >= Hr) {
            if (lane == 0) { dst[0] = 0.0; dst[1] = 0.0; }
            continue;
        }
        const float* w = mix + (size_t)r * mix_stride + (size_t)h * HOPS + 4 * lane;
        const float* e = est + (size_t)r * est_stride + (size_t)h * HOPS + 4 * lane;
        v4f wv[4], ev[4];
        if (vec) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { wv[k] = *reinterpret_cast<const v4f*>(w + 256 * k); ev[k] = *reinterpret_cast<const v4f*>(e + 256 * k); }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) { wv[k][j] = w[256 * k + j]; ev[k][j] = e[256 * k + j]; }
        }
        double q[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ww = wv[k][j], ee = ev[k][j];
                const float b = ww - ee;                   // the reference's `background` (:101)
                const float num = ee * ee, den = b * b;
                q[0] += (double)(num / den);               // (:103) x / 0 = inf, 0 / 0 = NaN: passed on
                q[1] += (double)(ww * ww);                 // (:105)
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) q[i] += __shfl_down(q[i], off, 64);
        if (lane == 0) { dst[0] = q[0] / (double)HOPS; dst[1] = q[1] / (double)HOPS; }
    }
}

}  // namespace

void launch_hop_activity(const float* mix, int64_t mix_stride, const float* est, int64_t est_stride, const int32_t* hops, int R, int Hmax,
                         double* act, hipStream_t s)
{
    // decided once per call: one row off alignment puts the whole call on scalar loads (a hop starts a multiple of 1024 floats into its row)
    const int vec = (mix_stride % 4 == 0) && (est_stride % 4 == 0) && (((uintptr_t)mix | (uintptr_t)est) & 15) == 0;
    hipLaunchKernelGGL(hop_activity_kernel, dim3((unsigned)(((int64_t)Hmax + ACT_WAVES - 1) / ACT_WAVES), R < 65535 ? R : 65535), dim3(64 * ACT_WAVES), 0, s, mix,
                       mix_stride, est, est_stride, hops, R, Hmax, vec, act);
}

// Interleaved columns per workgroup of the two spectral loss kernels: about 4096 floats of a row per workgroup, at most 129 columns (16
// workgroups per row) and never 2^31 floats
int train_loss_freq_columns(int Tmax)
{
    const int nf = (4096 + Tmax - 1) / Tmax;
    return nf < 1 ? 1 : (nf > 129 ? 129 : nf);
}
int train_loss_freq_blocks(int Tmax) { const int nf = train_loss_freq_columns(Tmax); return (F2 + nf - 1) / nf; }

void launch_train_loss_ragged(const float* y, const float* sfreq, const float* xtime, const float* speech, const int64_t* lens,
                              const TrainClip* clips, int n_clips, int R, int Tmax, int64_t wave_stride, double* part, double* values,
                              double* row_sums, hipStream_t s)
{
    const int64_t out_stride = (int64_t)(Tmax - 1) * HOPS;
    const int chunks = metric_time_chunks(out_stride), nf = train_loss_freq_columns(Tmax), FB = train_loss_freq_blocks(Tmax);
    double *p_time = part, *p_freq = part + (size_t)R * chunks * TRAIN_TIME_Q;
    // decided once per call: one row off alignment puts the whole call on scalar loads
    const int vec_t = (wave_stride % 4 == 0) && (((uintptr_t)xtime | (uintptr_t)speech) & 15) == 0;
    const int vec_f = (((uintptr_t)y | (uintptr_t)sfreq) & 15) == 0;
    hipLaunchKernelGGL(train_loss_time_ragged_kernel, dim3(chunks, R), dim3(256), 0, s, xtime, speech, lens, out_stride, wave_stride, vec_t, p_time);
    hipLaunchKernelGGL(train_loss_freq_ragged_kernel, dim3(FB, R), dim3(256), 0, s, y, sfreq, lens, Tmax, nf, vec_f, p_freq);
    hipLaunchKernelGGL(train_loss_finish_kernel, dim3((n_clips + 63) / 64), dim3(64), 0, s, clips, n_clips, p_time, chunks, p_freq, FB, values, row_sums);
}
size_t train_loss_partials(int R, int Tmax)
{
    return (size_t)R * ((size_t)metric_time_chunks((int64_t)(Tmax - 1) * HOPS) * TRAIN_TIME_Q + (size_t)train_loss_freq_blocks(Tmax) * 2);
}
void launch_train_loss_ragged_backward(const float* y, const float* sfreq, const float* xtime, const float* speech, const int64_t* lens,
                                       const TrainClip* clips, const int32_t* row_clip, const float* gclip, const double* row_sums, int R,
                                       int Tmax, int64_t wave_stride, float* dy, float* dxtime, hipStream_t s)
{
    const int64_t out_stride = (int64_t)(Tmax - 1) * HOPS;
    const int chunks = metric_time_chunks(out_stride), nf = train_loss_freq_columns(Tmax), FB = train_loss_freq_blocks(Tmax);
    const int vec_t = (wave_stride % 4 == 0) && (((uintptr_t)xtime | (uintptr_t)speech | (uintptr_t)dxtime) & 15) == 0;
    const int vec_f = (((uintptr_t)y | (uintptr_t)sfreq | (uintptr_t)dy) & 15) == 0;
    hipLaunchKernelGGL(train_loss_freq_ragged_bwd_kernel, dim3(FB, R), dim3(256), 0, s, y, sfreq, lens, clips, row_clip, gclip, Tmax, nf, vec_f, dy);
    hipLaunchKernelGGL(train_loss_time_ragged_bwd_kernel, dim3(chunks, R), dim3(256), 0, s, xtime, speech, lens, clips, row_clip, gclip, row_sums,
                       out_stride, wave_stride, vec_t, dxtime);
}

int metric_time_chunks(int64_t n_est) { int64_t c = (n_est + 16383) / 16384; return (int)(c < 1 ? 1 : (c > 256 ? 256 : c)); }

// The one rule of the input-SDR grid: a clip's sample positions go to this many workgroups, however many clips the call has
int metric_input_sdr_blocks(int /* n_clips */) { return 64; }

void launch_metric_time_ragged(const float* est, const float* speech, const float* mix, const int64_t* lens, int R, int Tmax,
                               int64_t out_stride, int64_t wave_stride, double* part, hipStream_t s)
{
    // decided once per call: one row off alignment puts the whole call on scalar loads
    const int vec = (wave_stride % 4 == 0) && (((uintptr_t)est | (uintptr_t)speech | (uintptr_t)mix) & 15) == 0;
    hipLaunchKernelGGL(metric_time_ragged_kernel, dim3(metric_time_chunks((int64_t)(Tmax - 1) * HOPS), R), dim3(256), 0, s, est, speech, mix, lens,
                       out_stride, wave_stride, vec, part);
}
void launch_metric_sisdr_ragged(const float* est, const float* speech, const int64_t* lens, int R, int Tmax, int64_t out_stride,
                                int64_t wave_stride, const double* time_part, double* part, hipStream_t s)
{
    hipLaunchKernelGGL(metric_sisdr_ragged_kernel, dim3(metric_time_chunks((int64_t)(Tmax - 1) * HOPS), R), dim3(256), 0, s, est, speech, lens,
                       out_stride, wave_stride, time_part, part);
}
void launch_metric_input_sdr_ragged(const float* speech, const float* mix, const MetricClip* clips, int n_clips, int64_t wave_stride,
                                    double* part, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(metric_input_sdr_ragged_kernel, dim3(blocks, n_clips), dim3(256), 0, s, speech, mix, clips, wave_stride, part);
}
void launch_metric_freq_ragged(const FftTables& tb, const float* Yf, const float* Sf, const int64_t* lens, int R, int Tmax, double* part,
                               int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(metric_freq_ragged_kernel, dim3(blocks, R), dim3(256), 0, s, Yf, Sf, tb.colmap, tb.ld, lens, Tmax, part);
}

void launch_metric_ragged_segment(const FftTables& tb, const float* est, int64_t est_stride, const float* speech, const float* mix,
                                  const int64_t* lens, int64_t wave_stride, const float* Yf, const float* Sf, int Ri, int ta, int te,
                                  double* acc_time, double* acc_freq, hipStream_t s)
{
    // decided once per launch: one row off alignment puts it on scalar loads (a hop starts a multiple of 1024 floats into its row)
    const int vec = (wave_stride % 4 == 0) && (est_stride % 4 == 0) && (((uintptr_t)est | (uintptr_t)speech | (uintptr_t)mix) & 15) == 0;
    if (segment_owned(ta, te, te).hops > 0)                           // (a row that reaches the segment's end; a one-frame first segment completes no hop)
        hipLaunchKernelGGL(metric_time_ragged_segment_kernel, dim3(METRIC_SEG_SLOTS, Ri), dim3(256), 0, s, est, est_stride, speech, mix, lens,
                           wave_stride, ta, te, vec, acc_time);
    hipLaunchKernelGGL(metric_freq_ragged_segment_kernel, dim3(METRIC_SEG_SLOTS, Ri), dim3(256), 0, s, Yf, Sf, tb.colmap, tb.ld, lens, ta, te, acc_freq);
}

}  // namespace bsrnn
