// Sample-rate conversion (bsrnn_resample, bsrnn_resampler_*): the definition, as index arithmetic and a filter design.
// The operation IS scipy.signal.resample_poly(x, up, down) with its defaults - zero phase, zeros outside the clip:
//   g = gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g, M = max(up, down), half = 10 * M,
//   h = firwin(2 * half + 1, 1 / M, window = ('kaiser', 5.0)) * up            (designed in double, rounded to fp32 once),
//   n_out = ceil(n_in * up / down), and for 0 <= j < n_out with c = j * down
//   y[j] = sum over i in [max(0, ceil((c - half) / up)), min(n_in - 1, floor((c + half) / up))] of x[i] * h[c - i * up + half].
// Polyphase form: with c = i0 * up + p (p the phase, 0 <= p < up) and Kh = half / up, output j reads the L inputs
// x[i0 - Kh + t], t = 0 .. L - 1, against row p of a table [up][L] whose entry t is h[p + half + (Kh - t) * up], or zero where that
// index leaves [0, 2 * half]: every tap sits in the table exactly once, rows are padded with zeros to the common L, the loop over t
// has no branch.  Inputs outside [0, n_in) count as zeros.
// Index arithmetic is 64-bit throughout (j * down passes 2^31 a minute into a 192 kHz clip).  No HIP types: resample.hip uses the
// index helpers on the device, api_resample.hip designs and lays out the table, tests/cpp/resample_check.cpp checks all of it with g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define BSRNN_RS_HD __host__ __device__
#else
#define BSRNN_RS_HD
#endif

namespace bsrnn {

constexpr int RESAMPLE_MAX_FACTOR = 1024;      // the reduced max(up, down) a conversion may have
constexpr int RESAMPLE_HALF_PER_M = 10;        // half = 10 * max(up, down): resample_poly's default filter length
constexpr double RESAMPLE_KAISER_BETA = 5.0;

enum ResampleWhy { RESAMPLE_OK = 0, RESAMPLE_BAD_RATE, RESAMPLE_TOO_FINE };

struct ResampleRatio {
    int64_t up = 1, down = 1, half = RESAMPLE_HALF_PER_M;
    int Kh = RESAMPLE_HALF_PER_M;      // half / up: inputs a output reads in front of i0 = floor(j * down / up)
    int L = 2 * RESAMPLE_HALF_PER_M + 1;   // taps per phase
    int why = RESAMPLE_OK;
};

inline int64_t resample_gcd(int64_t a, int64_t b)
{
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// The reduced ratio and the sizes that follow from it.  why: RESAMPLE_BAD_RATE for a rate < 1, RESAMPLE_TOO_FINE when the reduced
// max(up, down) is beyond RESAMPLE_MAX_FACTOR (up and down are then still the reduced pair, for the error text).
inline ResampleRatio resample_ratio(int64_t rate_in, int64_t rate_out)
{
    ResampleRatio q;
    if (rate_in < 1 || rate_out < 1) { q.why = RESAMPLE_BAD_RATE; return q; }
    const int64_t g = resample_gcd(rate_in, rate_out);
    q.up = rate_out / g; q.down = rate_in / g;
    const int64_t M = q.up > q.down ? q.up : q.down;
    if (M > RESAMPLE_MAX_FACTOR) { q.why = RESAMPLE_TOO_FINE; return q; }
    q.half = RESAMPLE_HALF_PER_M * M;
    q.Kh = (int)(q.half / q.up);
    q.L = q.Kh + (int)((q.half + q.up - 1) / q.up) + 1;
    return q;
}

// ceil(n_in * up / down)
BSRNN_RS_HD inline int64_t resample_n_out(int64_t n_in, int64_t up, int64_t down) { return (n_in * up + down - 1) / down; }

// First and last input index output j reads (the closed form above); first > last when the clip holds none of them.
BSRNN_RS_HD inline int64_t resample_first(int64_t j, int64_t up, int64_t down, int64_t half)
{
    const int64_t a = j * down - half;
    return a <= 0 ? 0 : (a + up - 1) / up;
}
BSRNN_RS_HD inline int64_t resample_last(int64_t j, int64_t up, int64_t down, int64_t half, int64_t n_in)
{
    const int64_t b = (j * down + half) / up;
    return b < n_in - 1 ? b : n_in - 1;
}

// Polyphase form: output j reads x[resample_base(j) + t] * table[resample_phase(j)][t], t = 0 .. L - 1 (the base may be negative).
BSRNN_RS_HD inline int64_t resample_phase(int64_t j, int64_t up, int64_t down) { return (j * down) % up; }
BSRNN_RS_HD inline int64_t resample_base(int64_t j, int64_t up, int64_t down, int64_t Kh) { return (j * down) / up - Kh; }
// Index into h of entry t of phase p's row, or -1 where the row is padding
BSRNN_RS_HD inline int64_t resample_tap_index(int64_t p, int64_t t, int64_t up, int64_t half, int64_t Kh)
{
    const int64_t idx = p + half + (Kh - t) * up;
    return idx >= 0 && idx <= 2 * half ? idx : -1;
}

// Streaming: the number of output samples fully determined once N input samples have arrived - the j whose last input,
// floor((j * down + half) / up), is at most N - 1 - and never more than the N samples' final length.  (With half = 10 * max(up, down)
// the count is always below that length, so the cap never binds; it is kept as the definition words it.)
BSRNN_RS_HD inline int64_t resample_ready(int64_t N, int64_t up, int64_t down, int64_t half)
{
    if (N < 1) return 0;
    const int64_t a = N * up - half - 1;                     // j * down <= a
    const int64_t n = a < 0 ? 0 : a / down + 1, cap = resample_n_out(N, up, down);
    return n < cap ? n : cap;
}
// Floats per row a streaming resampler keeps: the inputs that outputs not yet determined still need (at most
// Kh + half / up + 1 of them between two calls).
inline int64_t resample_carry_floats(const ResampleRatio& q) { return 2 * q.half / q.up + q.down / q.up + 2; }

// I0(x), x >= 0: the power series sum (x^2 / 4)^k / (k!)^2.  All terms are positive, so nothing cancels; at beta = 5 it needs 25 terms.
inline double resample_bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// h [2 * half + 1] in double: the windowed sinc with cutoff 1 / M of Nyquist, Kaiser window (beta 5, symmetric), unit DC gain, times up.
// The arithmetic follows firwin's step by step - sinc of (1 / M) * m, not of m / M - because the taps at multiples of M, zeros on
// paper, are in firwin what sin() makes of the rounded argument (about 1e-17): to agree with resample_poly to fp32 rounding on a
// signal that meets only those taps, they have to be the same small numbers, not better ones.  That much is a property of the libm
// this is compiled against and the one numpy uses - sin() of the same rounded argument near a multiple of pi, equal to a few ulp - not
// of the mathematics; tests/test_resample_host.py reports those taps apart from the rest.  Equal rates (M = 1) design nothing in
// scipy - resample_poly returns its input - and give the unit impulse here: the conversion is a copy.
inline std::vector<double> resample_design(const ResampleRatio& q)
{
    const double PI = 3.14159265358979323846;
    const int64_t n = 2 * q.half + 1, M = q.up > q.down ? q.up : q.down;
    std::vector<double> h((size_t)n, 0.0);
    if (M == 1) { h[(size_t)q.half] = 1.0; return h; }
    const double fc = 1.0 / (double)M, i0b = resample_bessel_i0(RESAMPLE_KAISER_BETA);
    double sum = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const double m = (double)(k - q.half), a = PI * (fc * m);
        const double s = k == q.half ? 1.0 : std::sin(a) / a;
        const double r = m / (double)q.half, u = 1.0 - r * r;
        const double w = resample_bessel_i0(RESAMPLE_KAISER_BETA * std::sqrt(u > 0.0 ? u : 0.0)) / i0b;
        h[(size_t)k] = fc * s * w;
        sum += h[(size_t)k];
    }
    for (double& v : h) v = v / sum * (double)q.up;
    return h;
}

// The polyphase table [up][ld], ld >= L (rows padded with zeros), taps rounded to fp32 here, once.
inline std::vector<float> resample_table(const ResampleRatio& q, const std::vector<double>& h, int ld)
{
    std::vector<float> tab((size_t)q.up * ld, 0.0f);
    for (int64_t p = 0; p < q.up; ++p)
        for (int t = 0; t < q.L; ++t) {
            const int64_t idx = resample_tap_index(p, t, q.up, q.half, q.Kh);
            if (idx >= 0) tab[(size_t)p * ld + t] = (float)h[(size_t)idx];
        }
    return tab;
}

// The same taps as the kernel reads them, [ld][up]: column jj = j mod up holds the row of j's phase, (jj * down) mod up (a bijection:
// up and down are coprime), so the lanes of a wave - consecutive j - read consecutive floats for each t instead of one row each.
inline std::vector<float> resample_table_by_output(const ResampleRatio& q, const std::vector<double>& h, int ld)
{
    const std::vector<float> tab = resample_table(q, h, ld);
    std::vector<float> out((size_t)ld * q.up);
    for (int64_t jj = 0; jj < q.up; ++jj)
        for (int t = 0; t < ld; ++t) out[(size_t)t * q.up + jj] = tab[(size_t)resample_phase(jj, q.up, q.down) * ld + t];
    return out;
}

// How the kernel cuts its work (resample.hip): a workgroup owns `tile` consecutive outputs of one row and walks the ld taps of a row
// (ld = L rounded up to 4: four partial sums) in chunks of `chunk` taps, staging for each chunk the inputs its tile needs in
// RESAMPLE_SPAN floats of LDS: (tile - 1) * down / up + chunk + 1 <= RESAMPLE_SPAN.  One chunk and 1024 outputs for every
// audio pair; the chunks and the short tiles are for ratios near 1024 : 1, whose rows have up to 20481 taps.
constexpr int RESAMPLE_SPAN = 8192, RESAMPLE_CHUNK_MAX = 4096, RESAMPLE_TILE_MAX = 1024;
struct ResampleTiling { int ld, chunk, tile; };
inline ResampleTiling resample_tiling(const ResampleRatio& q)
{
    ResampleTiling g;
    g.ld = (q.L + 3) & ~3;
    g.chunk = g.ld < RESAMPLE_CHUNK_MAX ? g.ld : RESAMPLE_CHUNK_MAX;
    const int64_t room = RESAMPLE_SPAN - g.chunk - 1;                  // (tile - 1) * down / up may take this much
    int64_t tile = 1 + room * q.up / q.down;
    if (tile >= 256) tile = tile / 256 * 256;
    g.tile = (int)(tile < RESAMPLE_TILE_MAX ? tile : RESAMPLE_TILE_MAX);
    return g;
}

}  // namespace bsrnn
