// The arithmetic of the streaming FIR convolution (csrc/convolve_stream_host.h) as a stand-alone program: tests/test_convolve_stream_host.py
// compares its output with a brute-force restatement in Python, and runs `self` plain and under the address and undefined-behaviour
// sanitizers.
//   cut K ALIGN N...   one row under K taps fed N... samples call by call: per call "first count ready emitted_before", then the flush
//                      "shift u0 u1 f1 first count n_out m0 m1"
//   rows K ALIGN N...  the same calls as the kernel's descriptors: per call "N0 E0 shift n_end ub ue u0 f1 n_in P keep", the flush last
//   limits             the header's constants
//   self               the header's own invariants over a sweep of (k, align, cutting); prints "ok"
#include "convolve_stream_host.h"

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

// One row fed `cuts` and flushed: the counts sum to N, ready is what the call reports, the blocks walked are consecutive, every output
// sample is stored exactly once and in order, the plan is conv_plan's, and no ring slot is written before its last reader has read it.
static int walk(int k, int align, const std::vector<long long>& cuts)
{
    const int P = conv_partitions(k);
    const int64_t shift = fir_stream_shift(k, align);
    int64_t N = 0, handed = 0, next_block = 0, next_store = 0;
    std::vector<int64_t> slot_frame(P, -1);          // the frame whose spectrum a ring slot holds
    auto run = [&](const FirStreamRow& q, int64_t count) -> int {
        if (q.ub != next_block && q.ue > q.ub) return fail("blocks are not consecutive", k, N, q.ub);
        for (int64_t u = q.ub; u < q.ue; ++u) {
            if (u <= q.f1) slot_frame[fir_stream_slot(u, P)] = u;
            if (u < q.u0) continue;
            const int64_t p_lo = u - q.f1 > 0 ? u - q.f1 : 0, p_hi = u < P - 1 ? u : P - 1;
            for (int64_t p = p_lo; p <= p_hi; ++p)
                if (slot_frame[fir_stream_slot(u - p, P)] != u - p) return fail("a ring slot was overwritten before its last reader", k, N, u);
            int64_t a = u * CONV_B - shift, b = a + CONV_B;
            if (a < 0) a = 0;
            if (b > q.n_end) b = q.n_end;
            if (a != next_store || b <= a) return fail("stores", k, N, u);
            if (a - q.E0 < 0 || b - q.E0 > count) return fail("a store outside the call's count", k, N, u);
            next_store = b;
        }
        if (q.ue > q.ub) next_block = q.ue;
        return 0;
    };
    for (long long n_in : cuts) {
        const int64_t ready = fir_stream_ready(N, n_in, shift);
        if (fir_stream_emitted(N, shift) != handed || ready < 0) return fail("emitted", k, N, -1);
        const FirStreamBlocks b = fir_stream_blocks(N, n_in);
        if (b.first != N / CONV_B || b.count != (N + n_in) / CONV_B - b.first) return fail("blocks", k, N, -1);
        const FirStreamRow q = n_in > 0 ? fir_stream_row_process(nullptr, k, align, N, n_in) : fir_stream_row_held();
        if (n_in > 0 && (q.ub != b.first || q.ue != b.first + b.count || q.E0 != handed || q.P != P || !q.keep)) return fail("descriptor", k, N, -1);
        if (int rc = run(q, ready)) return rc;
        N += n_in; handed += ready;
        if (next_store != handed) return fail("a call stored another count than it reported", k, N, -1);
    }
    const FirFlushPlan f = fir_stream_flush_plan(N, k, align);
    if (f.n_out != N - handed) return fail("flush count", k, N, -1);
    if (N > 0) {
        if (f.u1 != (N - 1 + shift) / CONV_B || f.first != N / CONV_B) return fail("flush plan", k, N, -1);
        if (align == FIR_ALIGN_SAME) {
            const ConvPlan c = conv_plan(N, k);
            if (f.shift != c.shift || f.u0 != c.u0 || f.u1 != c.u1 || f.f1 != c.f1) return fail("flush plan against conv_plan", k, N, -1);
            const ConvStore st = conv_store(c, N, c.u1);
            if (f.m0 != st.m0 || f.m1 != st.m1) return fail("last store against conv_store", k, N, -1);
        }
        // blocks formed before the flush only read frames within f1
        if (next_block - 1 > f.f1) return fail("an earlier block read a frame behind f1", k, N, next_block - 1);
    }
    const FirStreamRow q = fir_stream_row_flush(nullptr, k, align, N);
    if ((q.ue > q.ub) != (f.count > 0)) return fail("flush descriptor", k, N, -1);
    if (int rc = run(q, f.n_out)) return rc;
    if (next_store != N) return fail("the counts do not sum to N", k, N, -1);
    return 0;
}

static int self_check()
{
    const int ks[] = {1, 2, 3, 511, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 9300, 44101, CONV_MAX_TAPS};
    const long long ns[] = {0, 1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 2500, 9221, 20000, 300000};
    const long long draw[] = {0, 1, 1023, 1024, 1025, 3000};
    unsigned s = 2463534242u;
    for (int k : ks)
        for (int align : {FIR_ALIGN_SAME, FIR_ALIGN_CAUSAL})
            for (long long n : ns) {
                std::vector<long long> once{n}, hops, ragged;
                for (long long at = 0; at < n; at += CONV_B) hops.push_back(n - at < CONV_B ? n - at : CONV_B);
                for (long long at = 0; at < n;) {
                    s = s * 1664525u + 1013904223u;
                    long long c = draw[(s >> 10) % 6];
                    if (c > n - at) c = n - at;
                    ragged.push_back(c);
                    at += c;
                }
                for (const std::vector<long long>* cut : {&once, &hops, &ragged})
                    if (int rc = walk(k, align, *cut)) return rc;
            }
    if (fir_stream_ring_floats(3, 2049) != 3LL * 3 * CONV_LD || fir_stream_slot(7, 3) != 1) return fail("sizes", -1, -1, -1);
    printf("ok\n");
    return 0;
}

static void print_row(const FirStreamRow& q)
{
    printf("%lld %lld %lld %lld %lld %lld %lld %lld %d %d %d\n", (long long)q.N0, (long long)q.E0, (long long)q.shift, (long long)q.n_end, (long long)q.ub,
           (long long)q.ue, (long long)q.u0, (long long)q.f1, q.n_in, q.P, q.keep);
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "self")) return self_check();
    if (argc == 2 && !strcmp(argv[1], "limits")) {
        printf("%d %d %lld %lld %d\n", FIR_ALIGN_SAME, FIR_ALIGN_CAUSAL, (long long)FIR_STREAM_COUNT_MAX, (long long)FIR_STREAM_NO_CAP, FIR_STREAM_ROW_FLOATS);
        return 0;
    }
    if (argc >= 4 && (!strcmp(argv[1], "cut") || !strcmp(argv[1], "rows"))) {
        const bool rows = !strcmp(argv[1], "rows");
        const int k = atoi(argv[2]), align = atoi(argv[3]);
        const int64_t shift = fir_stream_shift(k, align);
        int64_t N = 0;
        for (int i = 4; i < argc; ++i) {
            const long long n_in = atoll(argv[i]);
            if (rows) print_row(n_in > 0 ? fir_stream_row_process(nullptr, k, align, N, n_in) : fir_stream_row_held());
            else {
                const FirStreamBlocks b = fir_stream_blocks(N, n_in);
                printf("%lld %lld %lld %lld\n", (long long)b.first, (long long)b.count, (long long)fir_stream_ready(N, n_in, shift),
                       (long long)fir_stream_emitted(N, shift));
            }
            N += n_in;
        }
        if (rows) print_row(fir_stream_row_flush(nullptr, k, align, N));
        else {
            const FirFlushPlan f = fir_stream_flush_plan(N, k, align);
            printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)f.shift, (long long)f.u0, (long long)f.u1, (long long)f.f1, (long long)f.first,
                   (long long)f.count, (long long)f.n_out, (long long)f.m0, (long long)f.m1);
        }
        return 0;
    }
    fprintf(stderr, "usage: convolve_stream_check cut K ALIGN N... | rows K ALIGN N... | limits | self\n");
    return 2;
}
