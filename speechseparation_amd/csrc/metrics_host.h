// The host end of the validation metrics (bsrnn_evaluate, bsrnn_evaluate_ragged, bsrnn_evaluate_long_ragged): from the sums the metric
// kernels leave - per row, per clip - to the eight numbers of include/bsrnn_hip.h (BSRNN_M_*) of every CLIP, by the arithmetic bsrnn_evaluate
// documents: m_dataset.py:202-226, infer.py:44-47.  The one tail of the three entry points.
// Host arithmetic only, in a fixed order, so tests run it without a GPU (tests/cpp/metrics_finish_check.cpp).
#pragma once
#include "descriptors.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsrnn {

// A clip as the metric kernels and this file see it: its first row, its rows, their common length (the rectangular call: {0, R, n})
struct MetricClip { int first, rows; int64_t len; };

// the order of BSRNN_M_* (api.hip asserts that the two agree)
enum ClipMetric { CM_LOSS, CM_SDR, CM_INPUT_SDR, CM_SISDR, CM_L1_TIME, CM_L1_RE, CM_L1_IM, CM_SEPARATION_DB, CM_COUNT };

// Sums of one row over its n_est samples (x the estimate, s the clean signal, m the mixture): the seven of the time kernel -
// s^2, (x-s)^2, x*s, x^2, |x-s|, m^2, (m-x)^2 - then the SI-SDR pass's (alpha s)^2 and (alpha s - x)^2
constexpr int METRIC_TIME_Q = 7;
constexpr int CLIP_ROW_Q = METRIC_TIME_Q + 2;
constexpr double SISDR_EPS = 1.1920928955078125e-07;          // float32 machine epsilon (torchmetrics)

// Partial sums p[0], p[stride], ... added in index order
inline double add_in_order(const double* p, size_t count, size_t stride)
{
    double a = 0.0;
    for (size_t i = 0; i < count; ++i) a += p[i * stride];
    return a;
}

// The SI-SDR pass's two sums of one row, q[7] and q[8], from the row's totals q[0] = sum s^2, q[2] = sum x s, q[3] = sum x^2 - for a caller
// that no longer holds the estimate when the row's alpha is known (bsrnn_evaluate_long_ragged: a segment's estimate is gone when the next
// one starts).  alpha in fp32 exactly as the SI-SDR kernels form it; then sum (a s)^2 = a^2 sum s^2 and sum (a s - x)^2 = a^2 sum s^2 -
// 2 a sum x s + sum x^2 in double.  What the two-pass form has and this has not is the fp32 rounding of a * s[i]; what this has and that has not is a
// cancellation that magnifies the rounding of the double sums by 10^(SI-SDR / 10) (the two agree to 4e-7 dB up to 40 dB and to
// 2e-4 dB at 80 dB).  The clamp keeps rounding in the cancellation (x == a s) from producing a negative noise power.
inline void sisdr_sums_from_totals(double q[CLIP_ROW_Q])
{
    const float eps = 1.1920928955078125e-07f;
    const float af = ((float)q[2] + eps) / ((float)q[0] + eps);
    const double a = (double)af;
    q[7] = a * a * q[0];
    const double nz = a * a * q[0] - 2.0 * a * q[2] + q[3];
    q[8] = nz > 0.0 ? nz : 0.0;
}

// One clip of `rows` rows, n samples each, T = 1 + n / 1024 frames, n_est = (T - 1) * 1024 estimated samples per row.
// row_sums [rows][CLIP_ROW_Q]; re_sum, im_sum: sum |Re Y - Re S|, sum |Im Y - Im S| over the clip's rows * T frames * 1025 bins;
// in_sdr_sum: sum over the clip's n sample positions of 10 log10 of the reference's `sdr2` ratio (its sums run over the clip's rows).
inline void finish_clip_metrics(const double* row_sums, int rows, double re_sum, double im_sum, double in_sdr_sum, int64_t n, int64_t T,
                                int64_t n_est, double out[CM_COUNT])
{
    double sdr = 0, sisdr = 0, l1_time = 0, m2 = 0, md2 = 0;
    for (int r = 0; r < rows; ++r) {
        const double* q = row_sums + (size_t)r * CLIP_ROW_Q;
        sdr += 10.0 * std::log10((q[0] + 1e-9) / (q[1] + 1e-9));                               // m_dataset.py:214-217
        sisdr += 10.0 * std::log10((q[7] + SISDR_EPS) / (q[8] + SISDR_EPS));
        l1_time += q[4]; m2 += q[5]; md2 += q[6];
    }
    l1_time /= (double)rows * (double)n_est;                                                   // L1Loss(reduction='mean'), train.py:54
    const double l1_re = re_sum / ((double)rows * 1025.0 * (double)T);
    const double l1_im = im_sum / ((double)rows * 1025.0 * (double)T);
    out[CM_LOSS] = l1_time + l1_re + l1_im;                                                    // m_dataset.py:211-213
    out[CM_SDR] = sdr / rows;
    out[CM_INPUT_SDR] = in_sdr_sum / (double)n;
    out[CM_SISDR] = sisdr / rows;
    out[CM_L1_TIME] = l1_time;
    out[CM_L1_RE] = l1_re;
    out[CM_L1_IM] = l1_im;
    out[CM_SEPARATION_DB] = 10.0 * std::log(m2 / md2);                                         // natural log, infer.py:47
}

// The downloaded sums of a call to metrics [n_clips][CM_COUNT]: per clip, its rows in order, every row's partials added in index order.
// time [R][slots][7]; si [R][slots][2], the SI-SDR pass's partials, or null: the row's two sums come from its totals (sisdr_sums_from_totals);
// freq [R][freq_blocks][2]; in_sdr [n_clips][in_blocks].  R = all clips' rows.
inline void clip_metrics_from_partials(const MetricClip* clips, int n_clips, const double* time, const double* si, int slots, const double* freq,
                                       int freq_blocks, const double* in_sdr, int in_blocks, double* metrics)
{
    std::vector<double> rows;
    for (int i = 0; i < n_clips; ++i) {
        const MetricClip& k = clips[i];
        rows.assign((size_t)k.rows * CLIP_ROW_Q, 0.0);
        double re = 0, im = 0;
        for (int r = 0; r < k.rows; ++r) {
            const size_t row = (size_t)(k.first + r);
            double* q = &rows[(size_t)r * CLIP_ROW_Q];
            for (int j = 0; j < METRIC_TIME_Q; ++j) q[j] = add_in_order(time + row * slots * METRIC_TIME_Q + j, slots, METRIC_TIME_Q);
            if (si)
                for (int j = 0; j < 2; ++j) q[METRIC_TIME_Q + j] = add_in_order(si + row * slots * 2 + j, slots, 2);
            else
                sisdr_sums_from_totals(q);
            re += add_in_order(freq + row * freq_blocks * 2, freq_blocks, 2);
            im += add_in_order(freq + row * freq_blocks * 2 + 1, freq_blocks, 2);
        }
        const int64_t T = 1 + k.len / HOPS;
        finish_clip_metrics(rows.data(), k.rows, re, im, add_in_order(in_sdr + (size_t)i * in_blocks, in_blocks, 1), k.len, T, (T - 1) * HOPS,
                            metrics + (size_t)i * CM_COUNT);
    }
}

}  // namespace bsrnn
