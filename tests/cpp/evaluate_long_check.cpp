// Test helper: checks what the ragged long-form evaluate (bsrnn_evaluate_long_ragged) does on the host.  (1) plan_host.h, segment_owned:
// over the segments of ragged_long_plan's cut every real hop and every real frame of a row is owned exactly once, nothing else is, and
// only by segments whose alive prefix holds the row.  (2) metrics_host.h, sisdr_sums_from_totals: the SI-SDR sums derived from a row's
// totals against the two-pass arithmetic of the SI-SDR kernels (alpha in fp32, alpha * s[i] and the difference rounded to fp32, double
// sums) on seeded fp32 pairs, and the clamp.  Prints the largest SI-SDR difference seen and "ok"; the first mismatch is printed and the
// exit status is 1.  Host code only.
#include "metrics_host.h"
#include "plan_host.h"

#include <cmath>
#include <cstdio>
#include <random>
using namespace bsrnn;

static int g_bad = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

// every row length 2..13 beside every other one (the second row decides how long the first one stays inside the prefix, and the other
// way round), every segment length 1..14
static void check_coverage()
{
    for (int Ta = 2; Ta <= 13; ++Ta)
        for (int Tb = 2; Tb <= 13; ++Tb)
            for (int seg = 1; seg <= 14; ++seg) {
                const int64_t lens[2] = {(int64_t)(Ta - 1) * HOPS + 5, (int64_t)(Tb - 1) * HOPS + (Tb == 2 ? 1 : 0)};
                const int Tr[2] = {Ta, Tb};
                const RaggedLongPlan q = ragged_long_plan(lens, 2, (int64_t)14 * HOPS, seg);
                const int Tmax = (int)q.shape.Tmax;
                EXPECT(q.shape.why == RAGGED_OK && !q.too_many && Tmax == std::max(Ta, Tb) && q.nseg == (Tmax + seg - 1) / seg);
                if (g_bad) return;
                for (int r = 0; r < 2; ++r) {
                    std::vector<int> hop(Tmax + 2, 0), frame(Tmax + 2, 0);
                    for (int i = 0; i < q.nseg; ++i) {
                        const int ta = i * seg, te = std::min(Tmax, ta + seg);
                        const SegmentOwned own = segment_owned(ta, te, Tr[r]);
                        EXPECT(own.hops >= 0 && own.frames >= 0);
                        // what the segment's launches can reach at all: the hops it completes, its own frames
                        EXPECT(own.hop0 == std::max(ta - 1, 0) && (own.hops == 0 || own.hop0 + own.hops <= te - 1));
                        EXPECT(own.frame0 == ta && own.frames <= te - ta);
                        // the metric launches run on the rows of the alive prefix only: a row outside it must own nothing
                        if (r >= q.rows[i]) EXPECT(own.hops == 0 && own.frames == 0);
                        for (int h = own.hop0; h < own.hop0 + own.hops; ++h) ++hop[h];
                        for (int t = own.frame0; t < own.frame0 + own.frames; ++t) ++frame[t];
                    }
                    for (int h = 0; h < Tmax + 2; ++h) EXPECT(hop[h] == (h < Tr[r] - 1 ? 1 : 0));
                    for (int t = 0; t < Tmax + 2; ++t) EXPECT(frame[t] == (t < Tr[r] ? 1 : 0));
                    if (g_bad) { printf("T = %d beside %d, seg = %d, row %d\n", Ta, Tb, seg, r); return; }
                }
            }
    // literals: a one-frame first segment completes no hop; later one-frame segments one each; a row that ends at / one past an edge
    SegmentOwned o = segment_owned(0, 1, 10);
    EXPECT(o.hops == 0 && o.frames == 1);
    o = segment_owned(1, 2, 10);
    EXPECT(o.hop0 == 0 && o.hops == 1 && o.frame0 == 1 && o.frames == 1);
    o = segment_owned(0, 4, 4);
    EXPECT(o.hop0 == 0 && o.hops == 3 && o.frames == 4);
    o = segment_owned(4, 8, 4);
    EXPECT(o.hops == 0 && o.frames == 0);
    o = segment_owned(4, 8, 5);
    EXPECT(o.hop0 == 3 && o.hops == 1 && o.frame0 == 4 && o.frames == 1);
    o = segment_owned(3, 6, 4);
    EXPECT(o.hop0 == 2 && o.hops == 1 && o.frames == 1);
    o = segment_owned(6, 9, 4);
    EXPECT(o.hops == 0 && o.frames == 0);
}

// The two-pass arithmetic (metrics.hip: metric_time_ragged_kernel's sums, then metric_sisdr_ragged_kernel) for one row
static void two_pass(const std::vector<float>& x, const std::vector<float>& s, double q[CLIP_ROW_Q])
{
    for (int i = 0; i < CLIP_ROW_Q; ++i) q[i] = 0.0;
    for (size_t i = 0; i < x.size(); ++i) {
        q[0] += (double)s[i] * s[i]; q[2] += (double)x[i] * s[i]; q[3] += (double)x[i] * x[i];
    }
    const float eps = 1.1920928955078125e-07f;
    const float a = ((float)q[2] + eps) / ((float)q[0] + eps);
    for (size_t i = 0; i < x.size(); ++i) {
        const volatile float ts = a * s[i];            // (volatile: each product and difference rounded to fp32, no contraction)
        const volatile float nz = ts - x[i];
        q[7] += (double)ts * ts; q[8] += (double)nz * nz;
    }
}
static double sisdr_db(const double q[CLIP_ROW_Q]) { return 10.0 * std::log10((q[7] + SISDR_EPS) / (q[8] + SISDR_EPS)); }

static double g_worst = 0.0;
// x = gain * (s + noise): SI-SDR ~ -20 log10(noise_rms / s_rms)
static void check_pair(unsigned seed, size_t n, double target_db, double bound_db)
{
    std::mt19937 gen(seed);
    std::normal_distribution<float> normal(0.f, 1.f);
    std::vector<float> x(n), s(n);
    const float noise = (float)std::pow(10.0, -target_db / 20.0) * 0.07f;
    for (size_t i = 0; i < n; ++i) { s[i] = 0.07f * normal(gen); x[i] = 0.8f * (s[i] + noise * normal(gen)); }
    double two[CLIP_ROW_Q], alg[CLIP_ROW_Q];
    two_pass(x, s, two);
    for (int i = 0; i < CLIP_ROW_Q; ++i) alg[i] = two[i];
    alg[7] = alg[8] = -1.0;
    sisdr_sums_from_totals(alg);
    const double a = sisdr_db(two), b = sisdr_db(alg), d = std::fabs(a - b);
    printf("n = %8zu  SI-SDR two-pass %+10.6f dB  from the totals %+10.6f dB  difference %.2e dB\n", n, a, b, d);
    EXPECT(std::fabs(a - target_db) < 1.0);            // the pair is where it was meant to be
    EXPECT(alg[8] >= 0.0 && d <= bound_db);
    for (int i = 0; i < 7; ++i) EXPECT(alg[i] == two[i]);                 // the seven totals are left alone
    g_worst = std::max(g_worst, d);
}

static void check_sisdr()
{
    unsigned seed = 1;
    for (size_t n : {(size_t)1024, (size_t)65536, (size_t)1 << 20, (size_t)1 << 22})
        for (double db : {-4.0, 1.0, 40.0}) check_pair(seed++, n, db, 1e-5);
    // 80 dB, beyond the figures any validation set shows.  The three totals cancel to 1e-8 of their size there, so the rounding of the double
    // sums themselves (about 1e-13 relative for a million terms added one after the other, as here) is what remains: held to the
    // project's bound on a decibel figure, 2e-3 dB.
    check_pair(seed++, (size_t)1 << 20, 80.0, 2e-3);
    // the clamp: x == a * s exactly (a = 0.5: every product is exact), so the noise power cancels to zero or to rounding of either sign
    {
        std::mt19937 gen(99);
        std::normal_distribution<float> normal(0.f, 1.f);
        double q[CLIP_ROW_Q] = {0};
        for (int i = 0; i < 4096; ++i) {
            const float s = 0.07f * normal(gen), x = 0.5f * s;
            q[0] += (double)s * s; q[2] += (double)x * s; q[3] += (double)x * x;
        }
        sisdr_sums_from_totals(q);
        EXPECT(q[8] >= 0.0 && q[8] <= 1e-12 * q[7] && q[7] > 0.0);
        EXPECT(std::isfinite(sisdr_db(q)) && sisdr_db(q) > 60.0);
        // totals that cancel to a negative value by construction: clamped to exactly zero
        double z[CLIP_ROW_Q] = {4.0, 0, 2.0, 1.0 - 1e-9, 0, 0, 0, 0, 0};       // a = 0.5: 0.25 * 4 - 2 * 0.5 * 2 + (1 - 1e-9) < 0
        sisdr_sums_from_totals(z);
        EXPECT(z[8] == 0.0 && std::fabs(z[7] - 1.0) < 1e-6);
        // silence: alpha = eps / eps = 1, both sums zero, 0 dB as the two-pass form gives
        double e[CLIP_ROW_Q] = {0};
        sisdr_sums_from_totals(e);
        EXPECT(e[7] == 0.0 && e[8] == 0.0 && sisdr_db(e) == 0.0);
    }
    printf("largest SI-SDR difference, totals against two passes: %.2e dB\n", g_worst);
}

int main()
{
    check_coverage();
    check_sisdr();
    if (!g_bad) printf("ok\n");
    return g_bad ? 1 : 0;
}
