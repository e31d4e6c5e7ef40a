// Test helper: checks the shape arithmetic of a ragged batch (speechseparation_amd/csrc/plan_host.h: ragged_frames, ragged_shape) against
// literals and prints "ok"; the first mismatch is printed and the exit status is 1.  Host code only.
#include "plan_host.h"

#include <cstdio>
using namespace bsrnn;

static int g_bad = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

static bool same(const RaggedShape& q, int64_t Tmax, int64_t out_stride, int bad_row, int64_t bad_len, int why)
{
    return q.Tmax == Tmax && q.out_stride == out_stride && q.bad_row == bad_row && q.bad_len == bad_len && q.why == why;
}

int main()
{
    // frames of one row: T = 1 + n / 1024 (torch.stft, center = True)
    EXPECT(ragged_frames(1025) == 2 && ragged_frames(2047) == 2 && ragged_frames(2048) == 3 && ragged_frames(4 * 1024) == 5);
    EXPECT(ragged_frames(9 * 1024 + 77) == 10 && ragged_frames((int64_t)1 << 40) == ((int64_t)1 << 30) + 1);

    // the six lengths of tests/test_gpu_separate_ragged.py: T_r = 10, 4, 5, 8, 9, 2
    const int64_t lens[6] = {9 * 1024 + 77, 3 * 1024 + 5, 4 * 1024, 7 * 1024 + 1023, 8 * 1024 + 1, 1025};
    const int T[6] = {10, 4, 5, 8, 9, 2};
    for (int r = 0; r < 6; ++r) EXPECT(ragged_frames(lens[r]) == T[r]);
    EXPECT(same(ragged_shape(lens, 6, 9 * 1024 + 77), 10, 9 * 1024, -1, 0, RAGGED_OK));
    EXPECT(same(ragged_shape(lens, 6, 9 * 1024 + 80), 10, 9 * 1024, -1, 0, RAGGED_OK));      // a stride beyond the longest row
    // the longest row last, and a batch without it
    const int64_t rev[6] = {1025, 8 * 1024 + 1, 7 * 1024 + 1023, 4 * 1024, 3 * 1024 + 5, 9 * 1024 + 77};
    EXPECT(same(ragged_shape(rev, 6, 9 * 1024 + 77), 10, 9 * 1024, -1, 0, RAGGED_OK));
    EXPECT(same(ragged_shape(rev, 5, 9 * 1024 + 77), 9, 8 * 1024, -1, 0, RAGGED_OK));

    // a multiple of 1024 (the last frame starts at the clip's last sample + 1), and the two-frame minimum alone
    const int64_t mult[2] = {4 * 1024, 2048};
    EXPECT(same(ragged_shape(mult, 2, 4 * 1024), 5, 4 * 1024, -1, 0, RAGGED_OK));
    const int64_t least[1] = {1025};
    EXPECT(same(ragged_shape(least, 1, 1025), 2, 1024, -1, 0, RAGGED_OK));

    // refused: no reflect padding at 1024 samples and below; a row longer than the stride; the FIRST offending row is reported
    const int64_t shorty[3] = {2000, 1024, 5};
    EXPECT(same(ragged_shape(shorty, 3, 4096), 0, 0, 1, 1024, RAGGED_SHORT));
    const int64_t zero[1] = {0}, neg[1] = {-7};
    EXPECT(same(ragged_shape(zero, 1, 4096), 0, 0, 0, 0, RAGGED_SHORT));
    EXPECT(same(ragged_shape(neg, 1, 4096), 0, 0, 0, -7, RAGGED_SHORT));
    const int64_t longer[4] = {4096, 3000, 4097, 1024};
    EXPECT(same(ragged_shape(longer, 4, 4096), 0, 0, 2, 4097, RAGGED_LONG));
    EXPECT(same(ragged_shape(longer, 2, 4096), 5, 4 * 1024, -1, 0, RAGGED_OK));                //(the rows in front of it are fine)
    EXPECT(same(ragged_shape(lens, 6, 9 * 1024 + 76), 0, 0, 0, 9 * 1024 + 77, RAGGED_LONG));

    if (!g_bad) printf("ok\n");
    return g_bad ? 1 : 0;
}
