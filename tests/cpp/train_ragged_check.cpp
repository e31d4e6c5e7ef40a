// Test helper: checks the clip table of a ragged training step (speechseparation_amd/csrc/train_ragged_host.h: train_clip_table) against
// literals and prints "ok"; the first mismatch is printed and the exit status is 1.  Host code only.
#include "train_ragged_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>
using namespace bsrnn;

static int g_bad = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

static bool clip_is(const TrainClip& k, int first, int rows, int64_t len, int64_t T, int64_t n_est)
{
    return k.first == first && k.rows == rows && k.len == len && k.T == T && k.n_est == n_est &&
           k.inv_time == 1.0 / ((double)rows * (double)n_est) && k.inv_freq == 1.0 / ((double)rows * 1025.0 * (double)T);
}

int main()
{
    // the rectangle of tests/test_gpu_train_ragged.py: clips of [2, 1, 1] rows, T = 6, 4, 2 (rows 0-1 share a length)
    {
        const int64_t lens[3] = {5 * 1024 + 300, 3 * 1024 + 77, 1025};
        const int32_t rows[3] = {2, 1, 1};
        const int64_t stride = 6 * 1024 + 3;
        const TrainClipTable t = train_clip_table(lens, rows, 3, stride);
        EXPECT(t.shape.why == CLIPS_OK && t.shape.R == 4 && t.shape.Tmax == 6 && t.shape.out_stride == 5 * 1024 && t.shape.bad_clip == -1);
        EXPECT(t.clips.size() == 3 && t.row_lens.size() == 4 && t.row_clip.size() == 4);
        if (t.clips.size() == 3 && t.row_lens.size() == 4 && t.row_clip.size() == 4) {
            EXPECT(clip_is(t.clips[0], 0, 2, lens[0], 6, 5 * 1024));
            EXPECT(clip_is(t.clips[1], 2, 1, lens[1], 4, 3 * 1024));
            EXPECT(clip_is(t.clips[2], 3, 1, 1025, 2, 1024));                 // a clip of 1 025 samples: two frames, one hop
            const int64_t rl[4] = {lens[0], lens[0], lens[1], lens[2]};
            const int32_t rc[4] = {0, 0, 1, 2};
            EXPECT(!memcmp(t.row_lens.data(), rl, sizeof rl) && !memcmp(t.row_clip.data(), rc, sizeof rc));
        }
        // the per-row lengths are a valid ragged batch of the same rectangle
        const RaggedShape rs = ragged_shape(t.row_lens.data(), (int)t.row_lens.size(), stride);
        EXPECT(rs.why == RAGGED_OK && rs.Tmax == 6 && rs.out_stride == 5 * 1024);
        // how the table travels: every part 8-byte aligned, the map behind the clips
        EXPECT(sizeof(TrainClip) == 48 && train_table_clips_at(4) == 32 && train_table_map_at(4, 3) == 32 + 3 * 48 && train_table_bytes(4, 3) == 32 + 3 * 48 + 16);
        EXPECT(train_table_bytes(3, 3) == 24 + 3 * 48 + 16 && train_table_bytes(1, 1) % 8 == 0);
        // no row counts: one row per clip
        const TrainClipTable u = train_clip_table(lens, nullptr, 3, stride);
        EXPECT(u.shape.why == CLIPS_OK && u.shape.R == 3 && u.clips.size() == 3 && u.row_clip.size() == 3);
        if (u.clips.size() == 3) EXPECT(clip_is(u.clips[0], 0, 1, lens[0], 6, 5 * 1024) && clip_is(u.clips[2], 2, 1, 1025, 2, 1024) && u.row_clip[2] == 2);
    }
    // a length equal to the stride is the longest a row takes; one more is refused
    {
        const int64_t lens[2] = {6 * 1024, 2000};
        const TrainClipTable t = train_clip_table(lens, nullptr, 2, 6 * 1024);
        EXPECT(t.shape.why == CLIPS_OK && t.shape.Tmax == 7 && t.clips.size() == 2);
        if (t.clips.size() == 2) EXPECT(clip_is(t.clips[0], 0, 1, 6 * 1024, 7, 6 * 1024) && clip_is(t.clips[1], 1, 1, 2000, 2, 1024));
        const TrainClipTable v = train_clip_table(lens, nullptr, 2, 6 * 1024 - 1);
        EXPECT(v.shape.why == CLIPS_LONG && v.shape.bad_clip == 0 && v.shape.bad_value == 6 * 1024 && v.clips.empty() && v.row_lens.empty() && v.row_clip.empty());
    }
    // refusals: a bad row count, a length of 1 024 (no reflect padding); the first offending clip is named and nothing is filled
    {
        const int64_t lens[3] = {5000, 1024, 3000};
        const int32_t rows0[3] = {2, 1, 0}, rowsneg[3] = {-2, 1, 1}, rows[3] = {2, 1, 1};
        TrainClipTable t = train_clip_table(lens, rows, 3, 5000);
        EXPECT(t.shape.why == CLIPS_SHORT && t.shape.bad_clip == 1 && t.shape.bad_value == 1024 && t.clips.empty() && t.row_clip.empty());
        t = train_clip_table(lens, rows0, 3, 5000);
        EXPECT(t.shape.why == CLIPS_SHORT && t.shape.bad_clip == 1);           // clip 1's length comes before clip 2's rows
        t = train_clip_table(lens, rowsneg, 3, 5000);
        EXPECT(t.shape.why == CLIPS_ROWS && t.shape.bad_clip == 0 && t.shape.bad_value == -2 && t.clips.empty());
        const int64_t good[3] = {5000, 1025, 3000};
        t = train_clip_table(good, rows0, 3, 5000);
        EXPECT(t.shape.why == CLIPS_ROWS && t.shape.bad_clip == 2 && t.shape.bad_value == 0 && t.clips.empty() && t.row_lens.empty());
        const int64_t huge[1] = {(int64_t)1 << 40};
        t = train_clip_table(huge, nullptr, 1, (int64_t)1 << 40);
        EXPECT(t.shape.why == CLIPS_MANY && t.clips.empty());
    }
    if (!g_bad) printf("ok\n");
    return g_bad ? 1 : 0;
}
