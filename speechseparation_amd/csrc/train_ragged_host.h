// The clip table of a ragged training step (bsrnn_train_loss_ragged and its backward): which rows a clip owns, its length, frames and
// estimated samples, the reciprocals of the two element counts its L1 means divide by, and the row -> clip map.  The loss of clip c is
// what the reference's `train_infer` gives for that clip alone (m_dataset.py:202-217): its means run over the clip's own rows * n_est
// samples and rows * 1025 * T bins, never over the padding of the rectangle R x Tmax or over another clip.  Validation is clip_shape's
// (plan_host.h): the first clip that breaks a bound is refused.  Host arithmetic only (api.hip uploads the table and launches), so tests
// run it without a GPU (tests/cpp/train_ragged_check.cpp).
#pragma once
#include "plan_host.h"

#include <cstdint>
#include <vector>

namespace bsrnn {

// The order of BSRNN_TV_* (api.hip asserts that the two agree)
enum TrainValue { TV_LOSS, TV_L1_TIME, TV_L1_RE, TV_L1_IM, TV_SDR, TV_COUNT };

// One clip as the loss kernels read it (by value from the uploaded table): rows [first, first + rows) of `len` samples each,
// T = 1 + len / 1024 frames, n_est = (T - 1) * 1024 samples of the estimate; inv_time = 1 / (rows * n_est), inv_freq = 1 / (rows * 1025 * T)
struct TrainClip {
    int32_t first, rows;
    int64_t len, T, n_est;
    double inv_time, inv_freq;
};

struct TrainClipTable {
    ClipShape shape;                      // clip_shape's answer, refusals included (nothing else is filled then)
    std::vector<TrainClip> clips;
    std::vector<int64_t> row_lens;        // [R]: the per-clip lengths expanded to rows
    std::vector<int32_t> row_clip;        // [R]: the clip a row belongs to
};

inline TrainClipTable train_clip_table(const int64_t* lens, const int32_t* rows, int n_clips, int64_t stride)
{
    TrainClipTable t;
    std::vector<int> first;
    t.shape = clip_shape(lens, rows, n_clips, stride, t.row_lens, first);
    if (t.shape.why != CLIPS_OK) return t;
    t.clips.reserve((size_t)n_clips);
    t.row_clip.reserve((size_t)t.shape.R);
    for (int c = 0; c < n_clips; ++c) {
        const int32_t nr = rows ? rows[c] : 1;
        const int64_t T = ragged_frames(lens[c]), n_est = (T - 1) * HOPS;
        t.clips.push_back(TrainClip{first[(size_t)c], nr, lens[c], T, n_est, 1.0 / ((double)nr * (double)n_est),
                                    1.0 / ((double)nr * (double)NBINS * (double)T)});
        t.row_clip.insert(t.row_clip.end(), (size_t)nr, (int32_t)c);
    }
    return t;
}

// Bytes of the table as it travels: [R int64 row lengths | n_clips TrainClip | R int32 row -> clip], every part 8-byte aligned
inline size_t train_table_clips_at(int64_t R) { return (size_t)R * sizeof(int64_t); }
inline size_t train_table_map_at(int64_t R, int n_clips) { return train_table_clips_at(R) + (size_t)n_clips * sizeof(TrainClip); }
inline size_t train_table_bytes(int64_t R, int n_clips) { return train_table_map_at(R, n_clips) + (((size_t)R * sizeof(int32_t) + 7) & ~size_t(7)); }

}  // namespace bsrnn
