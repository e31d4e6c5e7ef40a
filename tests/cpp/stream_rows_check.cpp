// Host check of csrc/stream_rows_host.h: the bitset that carries the rows of a streaming rows call by value.
// Build: g++ -O2 -std=c++17 -Wall -I speechseparation_amd/csrc tests/cpp/stream_rows_check.cpp -o stream_rows_check ; prints "ok".
#include "stream_rows_host.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace bsrnn;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// every bit of the set against the flags it was packed from; bits at and above C must be zero
static void check_set(const RowSet& s, const std::vector<uint8_t>& flags, int C)
{
    for (int r = 0; r < STREAM_ROWS_MAX; ++r) {
        const bool want = r < C && flags[r] != 0;
        if (row_set_has(s, r) != want) { printf("FAILED: C = %d, row %d: %d, want %d\n", C, r, (int)row_set_has(s, r), (int)want); ++failures; return; }
    }
}

int main()
{
    static_assert(sizeof(RowSet) == STREAM_ROWS_MAX / 8, "one bit per row, nothing else");
    static_assert(STREAM_ROWS_MAX == 2048, "BSRNN_STREAM_ROWS_MAX");
    const int sizes[] = {1, 63, 64, 65, 2048};
    for (int C : sizes) {
        RowSet s;
        memset(&s, 0xff, sizeof(s));                                     // (packing must not depend on what the struct held)
        std::vector<uint8_t> f(STREAM_ROWS_MAX, 0);
        // empty
        CHECK(pack_row_set(f.data(), C, s) == 0);
        check_set(s, f, C);
        // full, by flags (any nonzero byte counts) and by null
        for (int r = 0; r < C; ++r) f[r] = (uint8_t)(r % 3 == 0 ? 1 : (r % 3 == 1 ? 0x80 : 0xff));
        CHECK(pack_row_set(f.data(), C, s) == C);
        check_set(s, f, C);
        memset(&s, 0xff, sizeof(s));
        CHECK(pack_row_set(nullptr, C, s) == C);
        check_set(s, f, C);
        // alternating, both phases; flags behind C are not read as rows
        for (int phase = 0; phase < 2; ++phase) {
            for (int r = 0; r < STREAM_ROWS_MAX; ++r) f[r] = (uint8_t)((r & 1) == phase);
            int want = 0;
            for (int r = 0; r < C; ++r) want += f[r];
            CHECK(pack_row_set(f.data(), C, s) == want);
            check_set(s, f, C);
        }
        // one row: the last
        std::fill(f.begin(), f.end(), 0);
        f[C - 1] = 1;
        CHECK(pack_row_set(f.data(), C, s) == 1);
        check_set(s, f, C);
        // the same set from a list (a row named twice is one row)
        RowSet l;
        const int32_t rows[3] = {C - 1, 0, C - 1};
        CHECK(pack_row_list(rows, 3, C, l) == -1);
        f[0] = 1;
        check_set(l, f, C);
        // a bad entry is reported by its index
        const int32_t bad_hi[2] = {0, C}, bad_lo[3] = {0, 0, -1};
        CHECK(pack_row_list(bad_hi, 2, C, l) == 1);
        CHECK(pack_row_list(bad_lo, 3, C, l) == 2);
    }
    // more rows than the set holds, and none
    {
        RowSet s;
        std::vector<uint8_t> f(STREAM_ROWS_MAX + 1, 1), none(STREAM_ROWS_MAX, 0);
        CHECK(pack_row_set(f.data(), STREAM_ROWS_MAX + 1, s) == -1);
        check_set(s, none, STREAM_ROWS_MAX);                             // (left empty)
        CHECK(pack_row_set(nullptr, STREAM_ROWS_MAX + 1, s) == -1);
        CHECK(pack_row_set(f.data(), 0, s) == -1);
        const int32_t rows[1] = {0};
        CHECK(pack_row_list(rows, 1, STREAM_ROWS_MAX + 1, s) == 1);
        CHECK(pack_row_list(rows, 1, 0, s) == 1);
    }
    CHECK(stream_row_floats(12) == 2 * 2048 + 8 * 12 * 64);
    CHECK(stream_row_floats(42) == 2 * 2048 + 8 * 42 * 64);
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
