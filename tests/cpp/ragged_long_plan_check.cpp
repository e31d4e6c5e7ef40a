// Test helper: checks the plan of a ragged long-form call (speechseparation_amd/csrc/plan_host.h: ragged_long_plan) against a brute-force
// restatement over random lengths and orders, and prints every case as one line
//     seg stride len_0 ... len_{R-1} | rows_0 ... rows_{nseg-1} | frame_rows
// for tests/test_separate_long_ragged_host.py to hold spec.long_plan to, then "ok"; the first mismatches are printed as "BAD ..." lines and
// the exit status is 1.  Host code only.
#include "plan_host.h"

#include <cstdio>
#include <set>
using namespace bsrnn;

static int g_bad = 0;
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { if (g_bad < 20) printf("BAD %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)          // 0 .. n - 1
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_seed >> 33) % n;
}

// One case: the plan against the definition, row by row and frame by frame
static void check(const std::vector<int64_t>& lens, int64_t stride, int seg)
{
    const int R = (int)lens.size();
    const RaggedLongPlan q = ragged_long_plan(lens.data(), R, stride, seg);
    EXPECT(q.shape.why == RAGGED_OK && !q.too_many);
    std::vector<int64_t> T((size_t)R);
    int64_t Tmax = 0;
    for (int r = 0; r < R; ++r) { T[r] = 1 + lens[r] / 1024; Tmax = std::max(Tmax, T[r]); }
    EXPECT(q.shape.Tmax == Tmax && q.shape.out_stride == (Tmax - 1) * 1024);
    EXPECT(q.nseg == (int)((Tmax + seg - 1) / seg) && (int)q.rows.size() == q.nseg);
    if ((int)q.rows.size() != q.nseg) return;
    int64_t sum = 0, real = 0;
    std::set<int> ms;
    for (int i = 0; i < q.nseg; ++i) {
        const int64_t ta = (int64_t)i * seg, te = std::min<int64_t>(Tmax, ta + seg);
        int last = -1;
        for (int r = 0; r < R; ++r)
            if (T[r] > ta) last = r;
        EXPECT(last >= 0 && q.rows[i] == last + 1);                              // the alive prefix, by its definition
        for (int r = 0; r < R; ++r)
            if (T[r] > ta) EXPECT(r < q.rows[i]);                                // every row with a frame in the segment is inside it
        if (i) EXPECT(q.rows[i] <= q.rows[i - 1]);                               // rows only retire
        sum += (int64_t)(last + 1) * (te - ta);
        ms.insert((int)((last + 1) * (te - ta)));
    }
    for (int r = 0; r < R; ++r) real += T[r];
    EXPECT(q.rows[0] == R);
    EXPECT(q.frame_rows == sum && sum >= real && sum <= (int64_t)R * Tmax);
    if (seg >= Tmax) EXPECT(q.nseg == 1 && sum == (int64_t)R * Tmax);
    // the distinct frame-row counts, each once, all of them
    EXPECT(std::set<int>(q.ms.begin(), q.ms.end()) == ms && q.ms.size() == ms.size());
    printf("%d %lld", seg, (long long)stride);
    for (int r = 0; r < R; ++r) printf(" %lld", (long long)lens[r]);
    printf(" |");
    for (int i = 0; i < q.nseg; ++i) printf(" %d", q.rows[i]);
    printf(" | %lld\n", (long long)q.frame_rows);
}

int main()
{
    // the five rows of tests/test_gpu_separate_long_ragged.py, T_r = 10, 10, 7, 4, 2: sorted and with ended rows inside the prefix
    const std::vector<int64_t> sorted = {9293, 9216, 7167, 3077, 1025}, mixed = {9293, 1025, 7167, 9216, 3077};
    {
        const RaggedLongPlan a = ragged_long_plan(sorted.data(), 5, 9293, 3), b = ragged_long_plan(mixed.data(), 5, 9293, 3);
        EXPECT(a.rows == (std::vector<int>{5, 4, 3, 2}) && a.frame_rows == 38 && a.ms == (std::vector<int>{15, 12, 9, 2}));
        EXPECT(b.rows == (std::vector<int>{5, 5, 4, 4}) && b.frame_rows == 46);
        const RaggedLongPlan c = ragged_long_plan(sorted.data(), 5, 9293, 1);
        EXPECT(c.frame_rows == 33 && c.nseg == 10 && c.rows == (std::vector<int>{5, 5, 4, 4, 3, 3, 3, 2, 2, 2}));
        EXPECT(ragged_long_plan(sorted.data(), 5, 9293, 10).frame_rows == 50 && ragged_long_plan(sorted.data(), 5, 9293, 400).nseg == 1);
    }
    for (int seg : {1, 2, 3, 4, 9, 10, 11}) { check(sorted, 9293, seg); check(mixed, 9300, seg); }

    // random lengths and orders; every seg from 1 to beyond Tmax; lengths that are multiples of 1024, one below and one above them
    for (int it = 0; it < 60; ++it) {
        const int R = 1 + (int)rnd(9);
        std::vector<int64_t> lens((size_t)R);
        int64_t stride = 0;
        for (int r = 0; r < R; ++r) {
            const int64_t hops = 1 + rnd(14);
            const uint32_t k = rnd(4);
            lens[r] = k == 0 ? hops * 1024 + 1 + rnd(1023) : k == 1 ? (hops + 1) * 1024 : k == 2 ? hops * 1024 + 1023 : hops * 1024 + 1;
            stride = std::max(stride, lens[r]);
        }
        if (it % 3 == 0) std::sort(lens.begin(), lens.end(), [](int64_t a, int64_t b) { return a > b; });      // longest first
        if (it % 3 == 1) stride += rnd(5);
        const int Tmax = (int)(1 + stride / 1024);
        for (int seg = 1; seg <= Tmax + 2; ++seg) check(lens, stride, seg);
    }

    // refusals: ragged_shape's, passed through with nothing else filled; R * min(seg, Tmax) beyond one segment's limit
    {
        const int64_t shorty[3] = {2000, 1024, 5}, longer[2] = {4096, 4097};
        RaggedLongPlan q = ragged_long_plan(shorty, 3, 4096, 2);
        EXPECT(q.shape.why == RAGGED_SHORT && q.shape.bad_row == 1 && q.shape.bad_len == 1024 && q.nseg == 0 && q.rows.empty());
        q = ragged_long_plan(longer, 2, 4096, 2);
        EXPECT(q.shape.why == RAGGED_LONG && q.shape.bad_row == 1 && q.shape.bad_len == 4097 && q.nseg == 0);
        const int64_t huge[2] = {((int64_t)1 << 40), 2048};
        q = ragged_long_plan(huge, 2, (int64_t)1 << 40, 1 << 30);
        EXPECT(q.shape.why == RAGGED_OK && q.too_many && q.rows.empty());
        q = ragged_long_plan(huge, 2, (int64_t)1 << 40, 1 << 29);                 // 2 * 2^29 = 2^30 > INT32_MAX / 2
        EXPECT(q.too_many);
    }

    if (!g_bad) printf("ok\n");
    return g_bad ? 1 : 0;
}
