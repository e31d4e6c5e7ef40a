// The committed critic on a padded batch (bsrnn_critic_score_ragged / _score_grad_ragged): x is a rectangle [R][I][Tmax] whose rows belong
// to clips of different lengths - clip c owns clip_rows[c] consecutive rows of frames[c] frames each, CRITIC_MIN_T <= frames[c] <= Tmax -
// and every clip gets its own score (and gscale[c] * d score_c / d x in the rectangle's own layout).  The per-row chain lengths, the
// row -> clip table, the live tiles of the two fp16x2 kernels, the workspace and the argument verdicts, as integer arithmetic on the
// host.  HIP-free: api_critic.hip checks and plans a call with it, the kernels take the plan by value and the tables by pointer,
// tests/cpp/critic_ragged_check.cpp compiles it alone.
//
// THE DEFINITION.  score_c = sigmoid(Linear(mean over the clip's rows of mean over t < T4_r of layers(x_r)))  (reference bsrnn.py:531-536
// on the clip alone, as m_dataset.py:205-213 scores one clip at a time); the layers are per row and local in time, the two means run
// over the clip's own frames and rows.
//
// THE ORDER OF EVERY SUM.  The K-slab plan of the first layer is csc_plan(I, R, Tmax)'s - a function of the rectangle, not of the
// lengths - and the layers above run on the rectangle with critic_layout(R, ., len(Tmax), .).  So the order of every sum is a function of
// (I, R, Tmax) and the row's own length, and one clip that owns all R rows at frames = Tmax gets bsrnn_critic_score's bits.
//
// WHAT IS SKIPPED.  Row r has T_r frames and the chain T1_r .. T4_r (critic_chain of T_r).  A frame tile of the first layer's forward
// (128 frames from 128 bt) is LIVE when 128 bt < T1_r; a dead tile returns before it stages anything, a live one loads x[r][.][3 t + k]
// only for t < T1_r, i.e. below T_r.  A position tile of the first layer's dx (369 positions from 369 bs) is live when 369 bs < T_r; a
// dead one writes zeros.  What the forward leaves behind a row's frames in y1 .. y4 is unspecified (never read for a result, below).
//
// WHY LAYERS 4 .. 2 RUN ON THE RECTANGLE UNCHANGED.  Forward: y_l[r][.][t] for t < T_l_r reads y_(l-1)[r][.][3 t .. 3 t + 15], and
// 3 (T_l_r - 1) + 15 <= T_(l-1)_r - 1 by the definition of T_l_r: a valid frame reads valid frames only, whatever stands behind them (an
// output column of the products depends on its own input column alone).  Backward: the tail's gradient writes ZEROS into dp4[r][.][t] for
// T4_r <= t < T4max.  A frame t < T_out_r of a layer reaches the positions 3 t .. 3 t + 15 <= len_r - 1 only, so a position s >= len_r
// collects frames >= T_out_r alone: its dy is a sum of products with zeros, a zero; dp = y > 0 ? dy : 0.01 dy of a zero dy is zero
// whatever y holds there; by induction dp3, dp2 and dp1 are zero behind the row's lengths, and a position s < len_r gets exactly the
// terms it gets in the clip alone plus zeros.  (tests/cpp/critic_ragged_check.cpp checks the reach statement for every row and layer.)
#pragma once
#include "critic_grad_host.h"

namespace bsrnn {

// One layer's output length, for host and kernel alike (T >= 16 wherever it is called: every row holds CRITIC_MIN_T frames)
constexpr int crg_t_out(int T) { return (T - CRITIC_TAPS) / CRITIC_STRIDE + 1; }
constexpr int crg_t4(int T) { return crg_t_out(crg_t_out(crg_t_out(crg_t_out(T)))); }

// The tables of a call, as the kernels read them: per row its frames and its clip; per clip its first row, its rows and its frames
struct CrgRow { int32_t frames, clip; };
struct CrgClip { int32_t row0, rows, frames, pad; };

constexpr bool crg_fwd_tile_live(int T_r, int bt) { return bt * CSC_TILE_T < crg_t_out(T_r); }
constexpr bool crg_dx_tile_live(int T_r, int bs) { return cgd_tile_first(bs) < T_r; }

struct CrgPlan {
    CgdPlan g;                       // the rectangle (I, R, Tmax): slabs, tiles, y1 .. y4, the shared block and dp1 .. dp4
    int n_clips;
    // Workspace in floats: [g.f.ws_floats (a score needs no more) | dp1 .. dp4 at g.off_dp | pooled gradients [n_clips][32] | max words
    // [n_clips]], and behind them what only the exact chain of an INTERLEAVED input needs: the planar copy of x and the planar dx,
    // R * I * Tmax each (a score alone: the planar copy at g.f.ws_floats, as bsrnn_critic_score lays it out).
    int64_t off_pool, off_max, ws_floats, off_xp, off_dxp, ws_exact_floats;
    int64_t table_bytes;             // [R CrgRow | n_clips CrgClip]
};

inline CrgPlan crg_plan(int I, int R, int Tmax, int n_clips)
{
    CrgPlan p{};
    p.g = cgd_plan(I, R, Tmax);
    p.n_clips = n_clips;
    int64_t at = p.g.off_pool;       // (dp4 ends where the rectangle's own pooled gradient would stand)
    p.off_pool = at; at += (int64_t)n_clips * CRITIC_WIDTHS[CRITIC_LAYERS - 1];
    p.off_max = at; at += csc_round4(n_clips);
    p.ws_floats = at;
    p.off_xp = at; at += csc_round4((int64_t)R * I * Tmax);
    p.off_dxp = at; at += csc_round4((int64_t)R * I * Tmax);
    p.ws_exact_floats = at;
    p.table_bytes = (int64_t)R * (int64_t)sizeof(CrgRow) + (int64_t)n_clips * (int64_t)sizeof(CrgClip);
    return p;
}

// rows [R] and clips [n_clips] of checked arguments (crg_check below)
inline void crg_tables(const int32_t* frames, const int32_t* clip_rows, int n_clips, CrgRow* rows, CrgClip* clips)
{
    int r = 0;
    for (int c = 0; c < n_clips; ++c) {
        clips[c] = CrgClip{r, clip_rows[c], frames[c], 0};
        for (int j = 0; j < clip_rows[c]; ++j) rows[r++] = CrgRow{frames[c], c};
    }
}

// Live tiles of a call, summed over the rows (the layout call reports them; the kernels decide per workgroup by the same two predicates)
inline void crg_live_tiles(const CrgPlan& p, const int32_t* frames, const int32_t* clip_rows, int64_t* fwd, int64_t* dx)
{
    *fwd = 0; *dx = 0;
    for (int c = 0; c < p.n_clips; ++c) {
        *fwd += (int64_t)clip_rows[c] * critic_ceil(crg_t_out(frames[c]), CSC_TILE_T);
        *dx += (int64_t)clip_rows[c] * critic_ceil(frames[c], CGD_TILE_S);
    }
}

enum CrgWhy {
    CRG_OK = 0,
    CRG_BAD_CHANNELS,        // in_channels < 1
    CRG_NO_CLIPS,            // n_clips < 1
    CRG_BAD_CLIP_ROWS,       // a clip with fewer than 1 row                                   (*bad_clip names it)
    CRG_CLIP_TOO_SHORT,      // a clip with fewer than CRITIC_MIN_T frames                     (*bad_clip names it)
    CRG_CLIP_TOO_LONG,       // a clip with more than Tmax frames                              (*bad_clip names it)
    CRG_ROWS_MISMATCH,       // the clips' rows do not sum to R
    CRG_BAD_ORDER,           // x_order outside {planar, interleaved}
    CRG_ODD_INTERLEAVED,     // an interleaved input has an even number of channels
    CRG_TOO_LARGE,           // a tensor of the call, an image, the workspace or a grid would pass 2^31 - 1 elements
};
// grad: the call also forms dx (the dx image, dp1 .. dp4 and the planar dx count).  frames and clip_rows are not null.
inline int crg_check(int64_t I, int64_t R, int64_t Tmax, const int32_t* frames, const int32_t* clip_rows, int64_t n_clips, int64_t x_order,
                     bool grad, int* bad_clip)
{
    *bad_clip = -1;
    if (I < 1) return CRG_BAD_CHANNELS;
    if (n_clips < 1) return CRG_NO_CLIPS;
    if (n_clips > CRITIC_MAX_ELEMS) return CRG_TOO_LARGE;
    int64_t sum = 0;
    for (int c = 0; c < (int)n_clips; ++c) {
        *bad_clip = c;
        if (clip_rows[c] < 1) return CRG_BAD_CLIP_ROWS;
        if (frames[c] < CRITIC_MIN_T) return CRG_CLIP_TOO_SHORT;
        if (frames[c] > Tmax) return CRG_CLIP_TOO_LONG;
        sum += clip_rows[c];
    }
    *bad_clip = -1;
    if (sum != R) return CRG_ROWS_MISMATCH;
    switch (grad ? cgd_check(I, R, Tmax, x_order) : csc_check(I, R, Tmax, x_order)) {      // (the two enums share their first six values)
    case CSC_OK: break;
    case CSC_BAD_ORDER: return CRG_BAD_ORDER;
    case CSC_ODD_INTERLEAVED: return CRG_ODD_INTERLEAVED;
    default: return CRG_TOO_LARGE;
    }
    if (grad && crg_plan((int)I, (int)R, (int)Tmax, (int)n_clips).ws_exact_floats > CRITIC_MAX_ELEMS) return CRG_TOO_LARGE;
    return CRG_OK;
}
static_assert((int)CSC_OK == (int)CGD_OK && (int)CSC_BAD_ORDER == (int)CGD_BAD_ORDER && (int)CSC_ODD_INTERLEAVED == (int)CGD_ODD_INTERLEAVED,
              "crg_check reads both verdicts through one switch");

}  // namespace bsrnn
