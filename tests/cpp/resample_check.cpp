// Host check of csrc/resample_host.h: the definition of the sample-rate conversion (bsrnn_resample, bsrnn_resampler_*).
// Build: g++ -O1 -std=c++17 -Wall -Werror -I speechseparation_amd/csrc tests/cpp/resample_check.cpp -o resample_check
//   resample_check self                          the checks that need no outside reference; prints "ok"
//   resample_check taps RATE_IN RATE_OUT         "up down half Kh L", then the 2 * half + 1 taps in double, one per line
//   resample_check ranges RATE_IN RATE_OUT N_IN  n_out, then "first last" of every output
//   resample_check apply RATE_IN RATE_OUT FILE   FILE: float64 samples; prints the closed form evaluated in double, one sample per line
//   resample_check index UP DOWN HALF N_IN J     "first last phase base n_out(J) ready(J)" by the header's 64-bit helpers
//   resample_check ready RATE_IN RATE_OUT N ...  ready(N) for every N given
// tests/test_resample_host.py compares the last five with scipy and with Python's integers.
#include "resample_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace bsrnn;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static const int PAIRS[][2] = {{48000, 44100}, {44100, 48000}, {16000, 44100}, {192000, 44100}, {22050, 44100}, {44100, 22050},
                               {44100, 44100}, {44100, 8000}, {1024, 1}, {1, 1024}, {1023, 2}, {3, 1024}};

// the closed form of the header's first lines, in double
static double closed_form(const std::vector<double>& x, const std::vector<double>& h, const ResampleRatio& q, int64_t j)
{
    const int64_t n = (int64_t)x.size(), c = j * q.down;
    double y = 0.0;
    for (int64_t i = resample_first(j, q.up, q.down, q.half); i <= resample_last(j, q.up, q.down, q.half, n); ++i)
        y += x[(size_t)i] * h[(size_t)(c - i * q.up + q.half)];
    return y;
}

static uint64_t lcg(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static void self_check()
{
    for (const auto& pr : PAIRS) {
        const ResampleRatio q = resample_ratio(pr[0], pr[1]);
        CHECK(q.why == RESAMPLE_OK);
        CHECK(q.up * pr[0] == q.down * pr[1] && resample_gcd(q.up, q.down) == 1);
        CHECK(q.half == 10 * (q.up > q.down ? q.up : q.down) && q.Kh == q.half / q.up);
        const std::vector<double> h = resample_design(q);
        CHECK((int64_t)h.size() == 2 * q.half + 1);
        for (int64_t k = 0; k < q.half; ++k)
            if (h[(size_t)k] != h[(size_t)(2 * q.half - k)]) { CHECK(!"taps are symmetric"); break; }
        // the table holds every tap exactly once and zeros elsewhere, at the bare L and at the kernel's padded row length
        const ResampleTiling g = resample_tiling(q);
        CHECK(g.ld >= q.L && g.ld % 4 == 0 && g.ld < q.L + 4 && g.chunk % 4 == 0 && g.chunk >= 4 && g.chunk <= g.ld && g.tile >= 1);
        CHECK(g.tile <= RESAMPLE_TILE_MAX && (g.tile - 1) * q.down / q.up + 1 + g.chunk <= RESAMPLE_SPAN);
        const int lds[2] = {q.L, g.ld};
        for (int ld : lds) {
            std::vector<int> seen(h.size(), 0);
            const std::vector<float> tab = resample_table(q, h, ld);
            CHECK((int64_t)tab.size() == q.up * ld);
            bool good = true;
            for (int64_t p = 0; p < q.up; ++p)
                for (int t = 0; t < ld; ++t) {
                    const int64_t idx = t < q.L ? resample_tap_index(p, t, q.up, q.half, q.Kh) : -1;
                    const float v = tab[(size_t)p * ld + t];
                    if (idx < 0) good = good && v == 0.0f;
                    else { good = good && v == (float)h[(size_t)idx]; ++seen[(size_t)idx]; }
                }
            CHECK(good);
            for (int s : seen)
                if (s != 1) { CHECK(!"every tap once"); break; }
        }
        // the layout the kernel reads is a permutation of it: column j mod up holds the row of j's phase
        {
            const std::vector<float> tab = resample_table(q, h, g.ld), by_out = resample_table_by_output(q, h, g.ld);
            CHECK(by_out.size() == tab.size());
            bool good = true;
            for (int64_t j = 1000; j < 1000 + 2 * q.up; ++j)
                for (int t = 0; t < g.ld; ++t)
                    good = good && by_out[(size_t)t * q.up + j % q.up] == tab[(size_t)resample_phase(j, q.up, q.down) * g.ld + t];
            CHECK(good);
        }
        // L is tight: some phase uses the first column and some phase the last
        bool first = false, last = false;
        for (int64_t p = 0; p < q.up; ++p) {
            first = first || resample_tap_index(p, 0, q.up, q.half, q.Kh) >= 0;
            last = last || resample_tap_index(p, q.L - 1, q.up, q.half, q.Kh) >= 0;
        }
        CHECK(first && last);
        // the polyphase form reads the closed form's inputs against the closed form's taps
        const int64_t sizes[] = {1, 5, 1023, 3000};
        uint64_t seed = 7;
        for (int64_t n : sizes) {
            if (resample_n_out(n, q.up, q.down) * q.L > 4000000) continue;          // (the extreme ratios: the small sizes only)
            std::vector<double> x((size_t)n);
            for (double& v : x) v = (double)lcg(seed) / 2147483648.0 - 1.0;
            const int64_t n_out = resample_n_out(n, q.up, q.down);
            CHECK(n_out == (n * q.up + q.down - 1) / q.down && n_out >= 1);
            double worst = 0.0;
            for (int64_t j = 0; j < n_out; ++j) {
                const int64_t p = resample_phase(j, q.up, q.down), b = resample_base(j, q.up, q.down, q.Kh);
                double y = 0.0;
                for (int t = 0; t < q.L; ++t) {
                    const int64_t i = b + t, idx = resample_tap_index(p, t, q.up, q.half, q.Kh);
                    if (idx < 0) continue;
                    CHECK(idx == j * q.down - i * q.up + q.half);
                    const bool inside = i >= resample_first(j, q.up, q.down, q.half) && i <= resample_last(j, q.up, q.down, q.half, n);
                    CHECK(inside == (i >= 0 && i < n));
                    if (inside) y += x[(size_t)i] * h[(size_t)idx];
                }
                worst = std::fmax(worst, std::fabs(y - closed_form(x, h, q, j)));
                if (failures) return;
            }
            CHECK(worst == 0.0);
        }
        // streaming: ready() is monotone, never beyond the final length, and any split of a clip into blocks (empty ones included)
        // followed by a flush gives n_out samples; between calls the carry holds what is still needed
        for (int64_t n : {(int64_t)1, (int64_t)5, (int64_t)1023, (int64_t)1024, (int64_t)20000}) {
            int64_t prev = 0;
            for (int64_t N = 0; N <= n; N += (n > 2000 ? 37 : 1)) {
                const int64_t r = resample_ready(N, q.up, q.down, q.half);
                CHECK(r >= prev && r <= resample_n_out(N, q.up, q.down));
                // r is exactly the count of outputs whose last input has arrived
                if (r > 0) CHECK((((r - 1) * q.down + q.half) / q.up) <= N - 1);
                if (r < resample_n_out(N, q.up, q.down)) CHECK(((r * q.down + q.half) / q.up) > N - 1);
                prev = r;
            }
            for (int trial = 0; trial < 20; ++trial) {
                int64_t N = 0, J = 0, total = 0;
                while (N < n) {
                    int64_t blk = (int64_t)(lcg(seed) % 4 == 0 ? 0 : lcg(seed) % (uint64_t)(n / 3 + 2));
                    if (blk > n - N) blk = n - N;
                    const int64_t J1 = resample_ready(N + blk, q.up, q.down, q.half);
                    CHECK(J1 >= J);
                    total += J1 - J;
                    N += blk; J = J1;
                    const int64_t b = resample_base(J, q.up, q.down, q.Kh), keep = b > 0 ? b : 0;
                    CHECK(N - keep <= resample_carry_floats(q) && keep <= N);
                }
                total += resample_n_out(n, q.up, q.down) - J;
                CHECK(total == resample_n_out(n, q.up, q.down));
            }
        }
    }
    // limits
    CHECK(resample_ratio(0, 44100).why == RESAMPLE_BAD_RATE && resample_ratio(44100, -1).why == RESAMPLE_BAD_RATE);
    CHECK(resample_ratio(44100, 48001).why == RESAMPLE_TOO_FINE && resample_ratio(1025, 1).why == RESAMPLE_TOO_FINE);
    CHECK(resample_ratio(2050, 2).why == RESAMPLE_TOO_FINE && resample_ratio(2048, 2).why == RESAMPLE_OK);
    // equal rates: the unit impulse, so the formula is a copy
    {
        const ResampleRatio q = resample_ratio(44100, 44100);
        const std::vector<double> h = resample_design(q);
        CHECK(q.up == 1 && q.down == 1 && q.half == 10);
        for (int64_t k = 0; k < 21; ++k) CHECK(h[(size_t)k] == (k == 10 ? 1.0 : 0.0));
    }
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "self") {
        self_check();
        if (failures) return 1;
        printf("ok\n");
        return 0;
    }
    if (mode == "index" && argc == 7) {
        const int64_t up = atoll(argv[2]), down = atoll(argv[3]), half = atoll(argv[4]), n_in = atoll(argv[5]), j = atoll(argv[6]);
        printf("%lld %lld %lld %lld %lld %lld\n", (long long)resample_first(j, up, down, half), (long long)resample_last(j, up, down, half, n_in),
               (long long)resample_phase(j, up, down), (long long)resample_base(j, up, down, half / up), (long long)resample_n_out(j, up, down),
               (long long)resample_ready(j, up, down, half));
        return 0;
    }
    if (argc < 4) return 2;
    const ResampleRatio q = resample_ratio(atoll(argv[2]), atoll(argv[3]));
    if (q.why != RESAMPLE_OK) { printf("refused %d\n", q.why); return 0; }
    if (mode == "taps") {
        printf("%lld %lld %lld %d %d\n", (long long)q.up, (long long)q.down, (long long)q.half, q.Kh, q.L);
        for (double v : resample_design(q)) printf("%.17g\n", v);
        return 0;
    }
    if (mode == "ranges" && argc == 5) {
        const int64_t n = atoll(argv[4]), n_out = resample_n_out(n, q.up, q.down);
        printf("%lld\n", (long long)n_out);
        for (int64_t j = 0; j < n_out; ++j)
            printf("%lld %lld\n", (long long)resample_first(j, q.up, q.down, q.half), (long long)resample_last(j, q.up, q.down, q.half, n));
        return 0;
    }
    if (mode == "apply" && argc == 5) {
        FILE* f = fopen(argv[4], "rb");
        if (!f) return 3;
        std::vector<double> x;
        double v;
        while (fread(&v, sizeof v, 1, f) == 1) x.push_back(v);
        fclose(f);
        const std::vector<double> h = resample_design(q);
        const int64_t n_out = resample_n_out((int64_t)x.size(), q.up, q.down);
        for (int64_t j = 0; j < n_out; ++j) printf("%.17g\n", closed_form(x, h, q, j));
        return 0;
    }
    if (mode == "ready") {
        for (int i = 4; i < argc; ++i) printf("%lld\n", (long long)resample_ready(atoll(argv[i]), q.up, q.down, q.half));
        return 0;
    }
    return 2;
}
