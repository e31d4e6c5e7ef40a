// The plan of the long FIR convolution (csrc/convolve_host.h) as a stand-alone program: tests/test_convolve_host.py compares its output
// with a brute-force restatement in Python, and runs `self` plain and under the address and undefined-behaviour sanitizers.
//   ranges K N              "P shift u0 u1 f0 f1", then one line "u m0 m1 p_lo p_hi" per block
//   groups BUDGET NX:NB...  one line "first rows x_frames y_frames" per row group
//   limits                  the header's constants
//   self                    the header's own invariants over a sweep of (k, n); prints "ok"
#include "convolve_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bsrnn;

static int fail(const char* what, long long k, long long n, long long u)
{
    printf("FAILED %s at k = %lld, n = %lld, u = %lld\n", what, k, n, u);
    return 1;
}

static int self_check()
{
    const int ks[] = {1, 2, 3, 511, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 9300, 44101, CONV_MAX_TAPS};
    const long long ns[] = {1, 2, 3, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2500, 9221, 20000, 100000};
    for (int k : ks)
        for (long long n : ns) {
            const ConvPlan q = conv_plan(n, k);
            if (q.P != (k + 1023) / 1024 || q.shift != k / 2 || conv_left(k) + conv_shift(k) != k - 1) return fail("sizes", k, n, -1);
            if (q.nb < 1 || q.nx < 1 || q.f0 < 0 || q.f0 > q.u0 || q.f1 > q.u1) return fail("ranges", k, n, -1);
            if (conv_image_floats(k) != (long long)q.P * CONV_LD) return fail("image", k, n, -1);
            long long next = 0;                                  // the stores tile [0, n) in order
            std::vector<char> read(q.nx, 0);
            for (long long u = q.u0; u <= q.u1; ++u) {
                const ConvStore st = conv_store(q, n, u);
                if (st.m0 != next || st.m1 <= st.m0 || st.m1 > n) return fail("stores", k, n, u);
                next = st.m1;
                const ConvSpan sp = conv_span(q, u);
                if (sp.p_lo > sp.p_hi || sp.p_lo < 0 || sp.p_hi > q.P - 1) return fail("span", k, n, u);
                for (long long p = sp.p_lo; p <= sp.p_hi; ++p) {
                    const long long v = u - p;
                    if (v < q.f0 || v > q.f1) return fail("frame of a partition", k, n, u);
                    read[v - q.f0] = 1;
                }
            }
            if (next != n) return fail("coverage", k, n, -1);
            for (char c : read)
                if (!c) return fail("a frame nobody reads", k, n, -1);
        }
    // row groups: every row once, in order, budgets kept except by a single row
    for (long long budget : {1LL, 7LL, 100LL, (long long)CONV_FRAME_BUDGET}) {
        std::vector<int64_t> nx, nb;
        unsigned s = 12345u;
        for (int r = 0; r < 300; ++r) {
            s = s * 1664525u + 1013904223u;
            const int64_t a = (s >> 8) % (2 * budget + 3);
            nx.push_back(r % 5 == 0 ? 0 : a + 1);
            nb.push_back(r % 5 == 0 ? 0 : a);
        }
        const std::vector<ConvGroup> g = conv_groups(nx.data(), nb.data(), (int)nx.size(), budget);
        int at = 0;
        for (const ConvGroup& x : g) {
            if (x.first != at || x.rows < 1 || x.rows > CONV_GROUP_ROWS) return fail("group rows", budget, at, -1);
            int64_t sx = 0, sy = 0;
            for (int r = x.first; r < x.first + x.rows; ++r) { sx += nx[r]; sy += nb[r]; }
            if (sx != x.x_frames || sy != x.y_frames) return fail("group sums", budget, at, -1);
            if (x.rows > 1 && (sx > budget || sy > budget)) return fail("group budget", budget, at, -1);
            at += x.rows;
        }
        if (at != (int)nx.size()) return fail("group coverage", budget, at, -1);
    }
    printf("ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "self")) return self_check();
    if (argc == 2 && !strcmp(argv[1], "limits")) {
        printf("%d %d %d %lld %lld %d %d\n", CONV_B, CONV_LD, CONV_MAX_TAPS, (long long)CONV_MAX_LEN, (long long)CONV_FRAME_BUDGET, CONV_GROUP_ROWS, CONV_TILE);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "ranges")) {
        const int k = atoi(argv[2]);
        const long long n = atoll(argv[3]);
        const ConvPlan q = conv_plan(n, k);
        printf("%d %lld %lld %lld %lld %lld\n", q.P, (long long)q.shift, (long long)q.u0, (long long)q.u1, (long long)q.f0, (long long)q.f1);
        for (long long u = q.u0; u <= q.u1; ++u) {
            const ConvStore st = conv_store(q, n, u);
            const ConvSpan sp = conv_span(q, u);
            printf("%lld %lld %lld %lld %lld\n", u, (long long)st.m0, (long long)st.m1, (long long)sp.p_lo, (long long)sp.p_hi);
        }
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "groups")) {
        const long long budget = atoll(argv[2]);
        std::vector<int64_t> nx, nb;
        for (int i = 3; i < argc; ++i) {
            long long a = 0, b = 0;
            if (sscanf(argv[i], "%lld:%lld", &a, &b) != 2) return 2;
            nx.push_back(a); nb.push_back(b);
        }
        for (const ConvGroup& g : conv_groups(nx.data(), nb.data(), (int)nx.size(), budget))
            printf("%d %d %lld %lld\n", g.first, g.rows, (long long)g.x_frames, (long long)g.y_frames);
        return 0;
    }
    fprintf(stderr, "usage: convolve_plan_check ranges K N | groups BUDGET NX:NB... | limits | self\n");
    return 2;
}
