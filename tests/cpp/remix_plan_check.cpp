// The host side of the re-mix (csrc/remix_host.h) as a stand-alone program: tests/test_remix_host.py compares its output with a
// brute-force restatement in Python, and runs it plain and under the address and undefined-behaviour sanitizers.
//   check R N_TERMS MIX_STRIDE TARGET_STRIDE WIDTH [norows] [noterms] r:N:FIRST:COUNT... t:LEN:AT:HAS_SRC...
//                           "why index tiles read written" (tiles, read, written: -1 unless the call is valid)
//   limits                  the header's constants and the sizes of the two descriptors
//   self                    the header's own invariants over a sweep; prints "ok"
#include "remix_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace bsrnn;

static int fail(const char* what, long long a, long long b, long long c)
{
    printf("FAILED %s at %lld, %lld, %lld\n", what, a, b, c);
    return 1;
}

static int self_check()
{
    // a term's reads against a count of the samples, every placement around a short row
    for (long long n = 0; n <= 9; ++n)
        for (long long at = -12; at <= 12; ++at)
            for (long long len = 0; len <= 12; ++len) {
                long long want = 0;
                for (long long i = 0; i < n; ++i) want += (i - at >= 0 && i - at < len);
                if (remix_term_reads(n, at, len) != want) return fail("reads", n, at, len);
            }
    // tiles cover [0, width) and no more
    const long long widths[] = {0, 1, REMIX_TILE - 1, REMIX_TILE, REMIX_TILE + 1, 3 * REMIX_TILE + 5, 2205000, (long long)REMIX_MAX_LEN};
    for (long long w : widths) {
        const long long t = remix_tiles(w);
        if (t * REMIX_TILE < w || (t > 0 && (t - 1) * REMIX_TILE >= w) || t > (1LL << 29)) return fail("tiles", w, t, -1);
    }
    if (REMIX_TILE != REMIX_THREADS * REMIX_PER_LANE) return fail("tile", REMIX_TILE, REMIX_THREADS, REMIX_PER_LANE);
    // a valid call and each way of spoiling it
    static float src[8];
    RemixTerm terms[3] = {{src, 8, -2, 1.0f, 0}, {src, 3, 4, 0.5f, 0}, {nullptr, 0, 0, 0.25f, 0}};
    RemixRow rows[2] = {{5, 0, 3}, {0, 2, 1}};
    if (remix_check(rows, 2, terms, 3, 6, 7, 6).why != REMIX_OK) return fail("valid call", 0, 0, 0);
    const RemixTraffic q = remix_traffic(rows, 2, terms, 6);
    if (q.read != 4 * (5 + 1 + 0) || q.written != 8 * 6 * 2) return fail("traffic", q.read, q.written, 0);
    if (remix_check(nullptr, 2, terms, 3, 6, 7, 6).why != REMIX_NULL_TABLE || remix_check(rows, 2, nullptr, 3, 6, 7, 6).why != REMIX_NULL_TABLE)
        return fail("null tables", 0, 0, 0);
    if (remix_check(rows, 0, terms, 3, 6, 7, 6).why != REMIX_BAD_COUNT || remix_check(rows, 2, terms, 0, 6, 7, 6).why != REMIX_BAD_COUNT)
        return fail("counts", 0, 0, 0);
    if (remix_check(rows, 2, terms, 3, 5, 7, 6).why != REMIX_MIX_STRIDE || remix_check(rows, 2, terms, 3, 6, 5, 6).why != REMIX_TARGET_STRIDE)
        return fail("strides", 0, 0, 0);
    if (remix_check(rows, 2, terms, 2, 6, 7, 6).why != REMIX_ROW_TERMS || remix_check(rows, 2, terms, 2, 6, 7, 6).index != 0)
        return fail("term range", 0, 0, 0);
    // (R - 1) * stride at the bound and one row beyond it
    if (!remix_stride_ok(REMIX_MAX_LEN, 20, (1 << 20) + 1) || remix_stride_ok(REMIX_MAX_LEN, 20, (1 << 20) + 2)) return fail("extent", 0, 0, 0);
    printf("ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "self")) return self_check();
    if (argc == 2 && !strcmp(argv[1], "limits")) {
        printf("%d %d %d %lld %lld %zu %zu\n", REMIX_THREADS, REMIX_PER_LANE, REMIX_TILE, (long long)REMIX_MAX_LEN, (long long)REMIX_MAX_EXTENT,
               sizeof(RemixTerm), sizeof(RemixRow));
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "check")) {
        const int R = atoi(argv[2]), n_terms = atoi(argv[3]);
        const long long mix_stride = atoll(argv[4]), target_stride = atoll(argv[5]), width = atoll(argv[6]);
        static float one = 0.f;                                  // a source pointer that is not null; nothing here reads through it
        std::vector<RemixRow> rows;
        std::vector<RemixTerm> terms;
        bool norows = false, noterms = false;
        for (int i = 7; i < argc; ++i) {
            long long a = 0, b = 0, c = 0;
            if (!strcmp(argv[i], "norows")) norows = true;
            else if (!strcmp(argv[i], "noterms")) noterms = true;
            else if (sscanf(argv[i], "r:%lld:%lld:%lld", &a, &b, &c) == 3) rows.push_back(RemixRow{a, (int32_t)b, (int32_t)c});
            else if (sscanf(argv[i], "t:%lld:%lld:%lld", &a, &b, &c) == 3) terms.push_back(RemixTerm{c ? &one : nullptr, a, b, 1.0f, 0});
            else return 2;
        }
        if ((long long)rows.size() < R || (long long)terms.size() < n_terms) return 2;      // the tables hold what the counts promise
        const RemixVerdict v = remix_check(norows ? nullptr : rows.data(), R, noterms ? nullptr : terms.data(), n_terms, mix_stride, target_stride, width);
        long long tiles = -1, rd = -1, wr = -1;
        if (v.why == REMIX_OK) {
            const RemixTraffic q = remix_traffic(rows.data(), R, terms.data(), width);
            tiles = remix_tiles(width); rd = q.read; wr = q.written;
        }
        printf("%d %lld %lld %lld %lld\n", v.why, (long long)v.index, tiles, rd, wr);
        return 0;
    }
    fprintf(stderr, "usage: remix_plan_check check R N_TERMS MIX_STRIDE TARGET_STRIDE WIDTH [norows] [noterms] r:N:FIRST:COUNT... t:LEN:AT:HAS_SRC... | limits | self\n");
    return 2;
}
