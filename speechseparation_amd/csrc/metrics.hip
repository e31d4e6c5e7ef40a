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

template <int NQ>
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
    if (threadIdx.x < NQ) dst[threadIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

// grid (chunks, R).  est [R][n_est]; speech, mix [R][n_in], only their first n_est samples are used (m_dataset.py:198).
// part [R][chunks][7]: sum s^2, sum (x-s)^2, sum x*s, sum x^2, sum |x-s|, sum m^2, sum (m-x)^2
__global__ __launch_bounds__(256) void metric_time_kernel(const float* __restrict__ est, const float* __restrict__ speech,
                                                          const float* __restrict__ mix, int64_t n_est, int64_t n_in,
                                                          int vec, double* __restrict__ part)
{
    const int r = blockIdx.y;
    const float* x = est + (size_t)r * n_est;
    const float* s = speech + (size_t)r * n_in;
    const float* m = mix + (size_t)r * n_in;
    double q[METRIC_TIME_Q] = {0, 0, 0, 0, 0, 0, 0};
    auto one = [&](float xv, float sv, float mv) {
        const float d = xv - sv, e = mv - xv;          // fp32 differences, as the reference forms them
        q[0] += (double)sv * sv; q[1] += (double)d * d; q[2] += (double)xv * sv; q[3] += (double)xv * xv;
        q[4] += (double)__builtin_fabsf(d); q[5] += (double)mv * mv; q[6] += (double)e * e;
    };
    // vec: every row of the three signals starts 16-byte aligned (the host checks bases and n_in % 4; n_est is
    // a multiple of 1024), otherwise scalar loads
    const int64_t n4 = vec ? n_est / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const v4f xv = *reinterpret_cast<const v4f*>(x + 4 * i);
        const v4f sv = *reinterpret_cast<const v4f*>(s + 4 * i);
        const v4f mv = *reinterpret_cast<const v4f*>(m + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) one(xv[j], sv[j], mv[j]);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_est; i += (int64_t)gridDim.x * 256) one(x[i], s[i], m[i]);
    block_reduce_store<METRIC_TIME_Q>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * METRIC_TIME_Q);
}

// SI-SDR second pass (torchmetrics scale_invariant_signal_distortion_ratio, zero_mean = False): with the row's
// alpha, sum (alpha s)^2 and sum (alpha s - x)^2, the products formed in fp32 like the reference's tensors.
// part [R][chunks][2]
__global__ __launch_bounds__(256) void metric_sisdr_kernel(const float* __restrict__ est, const float* __restrict__ speech,
                                                           const float* __restrict__ alpha, int64_t n_est, int64_t n_in,
                                                           double* __restrict__ part)
{
    const int r = blockIdx.y;
    const float* x = est + (size_t)r * n_est;
    const float* s = speech + (size_t)r * n_in;
    const float a = alpha[r];
    double q[2] = {0, 0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_est; i += (int64_t)gridDim.x * 256) {
        const float ts = a * s[i], nz = ts - x[i];
        q[0] += (double)ts * ts; q[1] += (double)nz * nz;
    }
    block_reduce_store<2>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * 2);
}

// The reference's `sdr2` (m_dataset.py:219-222): its sample tensors still carry the DataLoader's batch dimension
// ([1, rows, n]), so `dim=1` sums over the ROWS, not over time: one ratio per sample position, averaged over
// the n positions.  Kept as written.  part [gridDim.x]
__global__ __launch_bounds__(256) void metric_input_sdr_kernel(const float* __restrict__ speech, const float* __restrict__ mix,
                                                               int R, int64_t n, double* __restrict__ part)
{
    double q[1] = {0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float a = 0.f, b = 0.f;
        for (int r = 0; r < R; ++r) {
            const float sv = speech[(size_t)r * n + i], d = sv - mix[(size_t)r * n + i];
            a += sv * sv; b += d * d;
        }
        q[0] += 10.0 * log10((double)(a + 1e-9f) / (double)(b + 1e-9f));
    }
    block_reduce_store<1>(q, part + blockIdx.x);
}

// Spectral L1 terms: Yf, Sf frame-major band-padded spectra [M][ld]; bin k at columns colmap[k] (re), +1 (im).
// part [gridDim.x][2]: sum |re diff|, sum |im diff|
__global__ __launch_bounds__(256) void metric_freq_kernel(const float* __restrict__ Yf, const float* __restrict__ Sf,
                                                          const int* __restrict__ colmap, int ld, int M, double* __restrict__ part)
{
    double q[2] = {0, 0};
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const float* y = Yf + (size_t)m * ld;
        const float* s = Sf + (size_t)m * ld;
        for (int k = threadIdx.x; k < NBINS; k += 256) {
            const int c = colmap[k];
            const float2 yv = *reinterpret_cast<const float2*>(y + c), sv = *reinterpret_cast<const float2*>(s + c);
            q[0] += (double)__builtin_fabsf(yv.x - sv.x);
            q[1] += (double)__builtin_fabsf(yv.y - sv.y);
        }
    }
    block_reduce_store<2>(q, part + (size_t)blockIdx.x * 2);
}

// ------------------------------------------------------------------------------ rows and clips of different lengths (bsrnn_evaluate_ragged)
// The same four reductions for a ragged batch: row r holds lens[r] samples and T_r = 1 + lens[r] / 1024 frames inside the rectangle R x Tmax
// that bsrnn_separate_ragged ran on; a clip is a run of consecutive rows of one length, and nothing is summed across clips.  The row (or the
// clip) belongs to the workgroup, so every bound below is workgroup-uniform and each loop runs over the real samples / frames only, with no
// length test inside it.  Every slot of a grid's partials is written - a workgroup that starts past its row's end stores zeros - so the host
// adds whole arrays whatever an earlier call left there.

// grid (chunks of Tmax, R).  est rows out_stride floats apart; speech, mix rows wave_stride floats apart, row r's first
// n_est_r = (lens[r] / 1024) * 1024 samples used.  part [R][chunks][7] as metric_time_kernel's.
__global__ __launch_bounds__(256) void metric_time_ragged_kernel(const float* __restrict__ est, const float* __restrict__ speech,
                                                                 const float* __restrict__ mix, const int64_t* __restrict__ lens,
                                                                 int64_t out_stride, int64_t wave_stride, int vec, double* __restrict__ part)
{
    const int r = blockIdx.y;
    const int64_t n_est = lens[r] / HOPS * HOPS;
    const float* x = est + (size_t)r * out_stride;
    const float* s = speech + (size_t)r * wave_stride;
    const float* m = mix + (size_t)r * wave_stride;
    double q[METRIC_TIME_Q] = {0, 0, 0, 0, 0, 0, 0};
    auto one = [&](float xv, float sv, float mv) {
        const float d = xv - sv, e = mv - xv;          // fp32 differences, as the reference forms them
        q[0] += (double)sv * sv; q[1] += (double)d * d; q[2] += (double)xv * sv; q[3] += (double)xv * xv;
        q[4] += (double)__builtin_fabsf(d); q[5] += (double)mv * mv; q[6] += (double)e * e;
    };
    // vec: every row of the three signals starts 16-byte aligned (the host checks the bases and wave_stride % 4; out_stride and n_est are
    // multiples of 1024), otherwise scalar loads - an odd stride puts every other row off alignment
    const int64_t n4 = vec ? n_est / 4 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const v4f xv = *reinterpret_cast<const v4f*>(x + 4 * i);
        const v4f sv = *reinterpret_cast<const v4f*>(s + 4 * i);
        const v4f mv = *reinterpret_cast<const v4f*>(m + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) one(xv[j], sv[j], mv[j]);
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_est; i += (int64_t)gridDim.x * 256) one(x[i], s[i], m[i]);
    block_reduce_store<METRIC_TIME_Q>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * METRIC_TIME_Q);
}

// SI-SDR second pass, grid as above.  The row's alpha is formed here, by every workgroup of the row, from the row's time partials
// (time_part [R][chunks][7], the launch in front of this one on the stream): added in index order in double, then
// ((float) sum x s + eps) / ((float) sum s^2 + eps) in fp32 - bsrnn_evaluate's host arithmetic - so the call needs no round trip in its middle.
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

// The reference's `sdr2` per clip, grid (blocks, clips): one ratio per sample position i < len of the clip, its two sums over the clip's own
// rows (all of that length), never over another clip's.  part [clips][blocks]
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
    for (int t = blockIdx.x; t < Tr; t += gridDim.x) {
        const float* y = Yf + ((size_t)r * Tmax + t) * ld;
        const float* s = Sf + ((size_t)r * Tmax + t) * ld;
        for (int k = threadIdx.x; k < NBINS; k += 256) {
            const int c = colmap[k];
            const float2 yv = *reinterpret_cast<const float2*>(y + c), sv = *reinterpret_cast<const float2*>(s + c);
            q[0] += (double)__builtin_fabsf(yv.x - sv.x);
            q[1] += (double)__builtin_fabsf(yv.y - sv.y);
        }
    }
    block_reduce_store<2>(q, part + ((size_t)r * gridDim.x + blockIdx.x) * 2);
}

}  // namespace

int metric_time_chunks(int64_t n_est) { int64_t c = (n_est + 16383) / 16384; return (int)(c < 1 ? 1 : (c > 256 ? 256 : c)); }

void launch_metric_time(const float* est, const float* speech, const float* mix, int R, int64_t n_est, int64_t n_in,
                        double* part, hipStream_t s)
{
    const int vec = (n_in % 4 == 0) && (((uintptr_t)est | (uintptr_t)speech | (uintptr_t)mix) & 15) == 0;
    hipLaunchKernelGGL(metric_time_kernel, dim3(metric_time_chunks(n_est), R), dim3(256), 0, s, est, speech, mix, n_est, n_in, vec, part);
}
void launch_metric_sisdr(const float* est, const float* speech, const float* alpha, int R, int64_t n_est, int64_t n_in,
                         double* part, hipStream_t s)
{
    hipLaunchKernelGGL(metric_sisdr_kernel, dim3(metric_time_chunks(n_est), R), dim3(256), 0, s, est, speech, alpha, n_est, n_in, part);
}
void launch_metric_input_sdr(const float* speech, const float* mix, int R, int64_t n, double* part, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(metric_input_sdr_kernel, dim3(blocks), dim3(256), 0, s, speech, mix, R, n, part);
}
void launch_metric_freq(const FftTables& tb, const float* Yf, const float* Sf, int M, double* part, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(metric_freq_kernel, dim3(blocks), dim3(256), 0, s, Yf, Sf, tb.colmap, tb.ld, M, part);
}

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

}  // namespace bsrnn
