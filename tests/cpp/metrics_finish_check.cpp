// Test helper: checks the clip arithmetic of a ragged evaluate (speechseparation_amd/csrc/plan_host.h: clip_shape) against literals and the
// per-clip finalisation of the metrics (metrics_host.h: finish_clip_metrics) against closed forms and the gather in front of it
// (clip_metrics_from_partials) against plain loops, and prints "ok"; every mismatch is printed and the exit status is 1.  Host code only.
#include "metrics_host.h"
#include "plan_host.h"

#include <cmath>
#include <cstdio>
using namespace bsrnn;

static int g_bad = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

static bool same(const ClipShape& q, int64_t R, int64_t Tmax, int64_t out_stride, int bad_clip, int64_t bad_value, int why)
{
    return q.R == R && q.Tmax == Tmax && q.out_stride == out_stride && q.bad_clip == bad_clip && q.bad_value == bad_value && q.why == why;
}
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static void check_clip_shape()
{
    std::vector<int64_t> rl;
    std::vector<int> fr;
    // the five clips of tests/test_gpu_evaluate_ragged.py: T_c = 10, 4, 5, 8, 2; R = 10
    const int64_t lens[5] = {9 * 1024 + 77, 3 * 1024 + 5, 4 * 1024, 7 * 1024 + 1023, 1500};
    const int32_t rows[5] = {2, 1, 2, 2, 3};
    const int64_t stride = 9 * 1024 + 77;
    EXPECT(same(clip_shape(lens, rows, 5, stride, rl, fr), 10, 10, 9 * 1024, -1, 0, CLIPS_OK));
    const int first[5] = {0, 2, 3, 5, 7};
    const int64_t expanded[10] = {lens[0], lens[0], lens[1], lens[2], lens[2], lens[3], lens[3], lens[4], lens[4], lens[4]};
    EXPECT(fr.size() == 5 && rl.size() == 10);
    for (size_t c = 0; c < fr.size() && c < 5; ++c) EXPECT(fr[c] == first[c]);
    for (size_t r = 0; r < rl.size() && r < 10; ++r) EXPECT(rl[r] == expanded[r]);
    // the per-row lengths are a valid ragged batch of the same rectangle
    const RaggedShape rs = ragged_shape(rl.data(), (int)rl.size(), stride);
    EXPECT(rs.why == RAGGED_OK && rs.Tmax == 10 && rs.out_stride == 9 * 1024);
    // no row counts: one row per clip
    EXPECT(same(clip_shape(lens, nullptr, 5, stride, rl, fr), 5, 10, 9 * 1024, -1, 0, CLIPS_OK));
    EXPECT(fr.size() == 5 && rl.size() == 5 && fr[4] == 4 && rl[4] == 1500 && rl[0] == lens[0]);
    // without the longest clip: Tmax is the largest T_c left
    EXPECT(same(clip_shape(lens + 1, rows + 1, 4, stride, rl, fr), 8, 8, 7 * 1024, -1, 0, CLIPS_OK));
    EXPECT(fr.size() == 4 && fr[0] == 0 && fr[3] == 5);

    // refused at the FIRST offending clip, its rows before its length; nothing is expanded
    const int32_t rows0[5] = {2, 0, 2, 2, 3}, rowsneg[5] = {2, 1, 2, -4, 3};
    EXPECT(same(clip_shape(lens, rows0, 5, stride, rl, fr), 0, 0, 0, 1, 0, CLIPS_ROWS));
    EXPECT(rl.empty() && fr.empty());
    EXPECT(same(clip_shape(lens, rowsneg, 5, stride, rl, fr), 0, 0, 0, 3, -4, CLIPS_ROWS));
    const int64_t shorty[5] = {lens[0], lens[1], 1024, 5, lens[4]};
    EXPECT(same(clip_shape(shorty, rows, 5, stride, rl, fr), 0, 0, 0, 2, 1024, CLIPS_SHORT));
    EXPECT(same(clip_shape(shorty, rowsneg, 5, stride, rl, fr), 0, 0, 0, 2, 1024, CLIPS_SHORT));     // clip 2's length comes before clip 3's rows
    EXPECT(same(clip_shape(shorty, rows0, 5, stride, rl, fr), 0, 0, 0, 1, 0, CLIPS_ROWS));
    const int64_t longer[5] = {lens[0], lens[1], lens[2], stride + 1, 1024};
    EXPECT(same(clip_shape(longer, rows, 5, stride, rl, fr), 0, 0, 0, 3, stride + 1, CLIPS_LONG));
    EXPECT(same(clip_shape(lens, rows, 5, stride - 1, rl, fr), 0, 0, 0, 0, stride, CLIPS_LONG));
    const int64_t one_bad[1] = {-7};
    const int32_t one_row0[1] = {0};
    EXPECT(same(clip_shape(one_bad, one_row0, 1, 4096, rl, fr), 0, 0, 0, 0, 0, CLIPS_ROWS));
    EXPECT(same(clip_shape(one_bad, nullptr, 1, 4096, rl, fr), 0, 0, 0, 0, -7, CLIPS_SHORT));
    // too many frame rows for one call: by the frames, and by the rows (nothing that large is expanded)
    const int64_t huge[1] = {(int64_t)1 << 40};
    ClipShape q = clip_shape(huge, nullptr, 1, (int64_t)1 << 40, rl, fr);
    EXPECT(q.why == CLIPS_MANY && q.bad_clip == -1 && rl.empty() && fr.empty());
    const int64_t two[2] = {2048, 2048};
    const int32_t many_rows[2] = {INT32_MAX, INT32_MAX};
    q = clip_shape(two, many_rows, 2, 2048, rl, fr);
    EXPECT(q.why == CLIPS_MANY && q.R == 2 * (int64_t)INT32_MAX && rl.empty() && fr.empty());
    EXPECT(!ragged_too_many(64, 126) && ragged_too_many(1, ((int64_t)1 << 30)) && !ragged_too_many(1, ((int64_t)1 << 30) - 1));
}

static void check_finish()
{
    double out[CM_COUNT];
    // a target equal to the estimate (alpha = 1): a zero time-domain L1 term and the epsilon-limited SDR and SI-SDR
    {
        const double e2 = 37.5;
        const double row[CLIP_ROW_Q] = {e2, 0.0, e2, e2, 0.0, 50.0, 12.5, e2, 0.0};
        finish_clip_metrics(row, 1, 0.0, 0.0, 0.0, 2048, 3, 2048, out);
        EXPECT(out[CM_L1_TIME] == 0.0 && out[CM_L1_RE] == 0.0 && out[CM_L1_IM] == 0.0 && out[CM_LOSS] == 0.0);
        EXPECT(near(out[CM_SDR], 10.0 * std::log10((e2 + 1e-9) / 1e-9), 1e-12));
        EXPECT(near(out[CM_SISDR], 10.0 * std::log10((e2 + SISDR_EPS) / SISDR_EPS), 1e-12));
        EXPECT(near(out[CM_SEPARATION_DB], 10.0 * std::log(4.0), 1e-12));                      // natural log
        EXPECT(out[CM_INPUT_SDR] == 0.0);
    }
    // known noise levels: signal energy 100 and 1000 against noise energy 1 are 20 and 30 dB (the epsilons move them by < 1e-8 dB)
    {
        const double row[CLIP_ROW_Q] = {100.0, 1.0, 0, 0, 0, 1.0, 1.0, 1000.0, 1.0};
        finish_clip_metrics(row, 1, 0.0, 0.0, 0.0, 4096, 5, 4096, out);
        EXPECT(near(out[CM_SDR], 20.0, 1e-7) && near(out[CM_SISDR], 30.0, 1e-5));
        EXPECT(out[CM_SEPARATION_DB] == 0.0);
    }
    // per-clip divisors: 3 rows of n = 5000 samples, T = 5, n_est = 4096; SDR and SI-SDR are means over the rows, the separation figure
    // and the L1 terms run over all of them
    {
        const int rows = 3;
        const int64_t n = 5000, T = 5, n_est = 4096;
        double q[3 * CLIP_ROW_Q] = {0};
        const double sdr_db[3] = {10.0, 30.0, 50.0}, si_db[3] = {0.0, 20.0, 10.0};
        for (int r = 0; r < rows; ++r) {
            double* p = q + r * CLIP_ROW_Q;
            p[1] = 2.0; p[0] = 2.0 * std::pow(10.0, sdr_db[r] / 10.0);
            p[8] = 4.0; p[7] = 4.0 * std::pow(10.0, si_db[r] / 10.0);
            p[4] = 0.5 * (double)n_est;                    // mean |x - s| = 0.5 in every row
            p[5] = 3.0 * (r + 1); p[6] = 1.0 + r;          // sum m^2 = 18, sum (m - x)^2 = 6
        }
        finish_clip_metrics(q, rows, 0.25 * rows * 1025 * T, 0.125 * rows * 1025 * T, 3.0 * (double)n, n, T, n_est, out);
        EXPECT(near(out[CM_L1_TIME], 0.5, 1e-15) && near(out[CM_L1_RE], 0.25, 1e-15) && near(out[CM_L1_IM], 0.125, 1e-15));
        EXPECT(near(out[CM_LOSS], 0.875, 1e-15));
        EXPECT(near(out[CM_SDR], 30.0, 1e-7) && near(out[CM_SISDR], 10.0, 1e-5));
        EXPECT(near(out[CM_INPUT_SDR], 3.0, 1e-15));
        EXPECT(near(out[CM_SEPARATION_DB], 10.0 * std::log(3.0), 1e-12));
        // one row of the same clip alone: its own divisors, its own figures
        finish_clip_metrics(q + CLIP_ROW_Q, 1, 0.25 * 1025 * T, 0.125 * 1025 * T, 3.0 * (double)n, n, T, n_est, out);
        EXPECT(near(out[CM_L1_TIME], 0.5, 1e-15) && near(out[CM_L1_RE], 0.25, 1e-15) && near(out[CM_SDR], 30.0, 1e-7));
        EXPECT(near(out[CM_SEPARATION_DB], 10.0 * std::log(6.0 / 2.0), 1e-12));
    }
    // partial sums are added in index order, with a stride
    {
        const double p[6] = {1.0, 100.0, 2.0, 200.0, 4.0, 400.0};
        EXPECT(add_in_order(p, 3, 2) == 7.0 && add_in_order(p + 1, 3, 2) == 700.0 && add_in_order(p, 0, 1) == 0.0);
        const double big[3] = {1e16, 1.0, -1e16};
        EXPECT(add_in_order(big, 3, 1) == 0.0);            // (1e16 + 1) - 1e16 in that order, not 1
    }
}

// clip_metrics_from_partials against the plain loops it took the place of, on synthetic partial arrays: two clips of 2 and 1 rows, time
// slot counts 1 and 3, spectral block counts 1 and 16, the SI-SDR sums from the second pass's partials and from the row's totals.  Exact.
static void check_gather()
{
    const MetricClip clips[2] = {{0, 2, 5000}, {2, 1, 3 * 1024 + 5}};
    const int R = 3, IB = 4;
    unsigned seed = 12345u;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return 0.25 + (double)(seed >> 8) / 16777216.0; };   // in [0.25, 1.25)
    for (int slots : {1, 3})
        for (int FB : {1, 16})
            for (int two_pass : {1, 0}) {
                std::vector<double> time((size_t)R * slots * METRIC_TIME_Q), si((size_t)R * slots * 2), freq((size_t)R * FB * 2), in(2 * IB);
                for (double& v : time) v = next();
                for (double& v : si) v = next();
                for (double& v : freq) v = next();
                for (double& v : in) v = next() - 0.75;
                double got[2 * CM_COUNT], want[2 * CM_COUNT];
                clip_metrics_from_partials(clips, 2, time.data(), two_pass ? si.data() : nullptr, slots, freq.data(), FB, in.data(), IB, got);
                for (int i = 0; i < 2; ++i) {
                    std::vector<double> rows((size_t)clips[i].rows * CLIP_ROW_Q, 0.0);
                    double re = 0, im = 0;
                    for (int r = 0; r < clips[i].rows; ++r) {
                        const size_t row = (size_t)(clips[i].first + r);
                        double* q = &rows[(size_t)r * CLIP_ROW_Q];
                        for (int s = 0; s < slots; ++s)
                            for (int j = 0; j < METRIC_TIME_Q; ++j) q[j] += time[(row * slots + s) * METRIC_TIME_Q + j];
                        if (two_pass)
                            for (int s = 0; s < slots; ++s) { q[7] += si[(row * slots + s) * 2]; q[8] += si[(row * slots + s) * 2 + 1]; }
                        else
                            sisdr_sums_from_totals(q);
                        double a = 0, b = 0;
                        for (int k = 0; k < FB; ++k) { a += freq[(row * FB + k) * 2]; b += freq[(row * FB + k) * 2 + 1]; }
                        re += a; im += b;
                    }
                    double sdr2 = 0;
                    for (int k = 0; k < IB; ++k) sdr2 += in[(size_t)i * IB + k];
                    const int64_t n = clips[i].len, T = 1 + n / 1024;
                    finish_clip_metrics(rows.data(), clips[i].rows, re, im, sdr2, n, T, (T - 1) * 1024, want + i * CM_COUNT);
                }
                for (int k = 0; k < 2 * CM_COUNT; ++k) {
                    if (got[k] != want[k]) printf("slots %d FB %d two_pass %d: number %d is %.17g, the plain loops give %.17g\n", slots, FB, two_pass, k, got[k], want[k]);
                    EXPECT(got[k] == want[k] && std::isfinite(got[k]));
                }
            }
}

int main()
{
    check_clip_shape();
    check_finish();
    check_gather();
    if (!g_bad) printf("ok\n");
    return g_bad ? 1 : 0;
}
