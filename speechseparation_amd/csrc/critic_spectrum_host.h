// The critic's input as the reference forms it (bsrnn_critic_spectrum; reference train-discriminator.py:62-68: torch.stft(w * scale,
// n_fft = 4096, hop_length = 1024, window = hann_window(4096)), then cat(real, imag)): the frame count, the reflected sample index, the
// slabs a call runs in, the scratch that follows from them and the verdict on a call's arguments, as integer arithmetic on the host.
// HIP-free: api_critic.hip checks and plans a call with it, stft4096.hip holds the kernels, tests/cpp/critic_spectrum_check.cpp compiles
// it alone.
//
// THE DEFINITION.  wave [R] rows of n > 2048 samples, `stride` floats apart; T = 1 + n / 1024 frames.  Frame t holds the padded samples
// t * 1024 + i - 2048, i < 4096, reflected at 0 and at n - 1 (cs_reflect: one reflection per sample is enough for n > 2048, a frame may
// need both ends); each sample is multiplied by `scale`, the product by the periodic Hann(4096) window, and the one-sided real DFT of the
// frame gives bins 0 .. 2048.  x [R][4098][T], T contiguous: rows 0 .. 2048 the real parts, rows 2049 .. 4097 the imaginary parts; rows
// 2049 and 4097 (bins 0 and 2048) are exactly zero.
//
// THE SLAB RULE.  A frame's 4098 values go to 4098 rows of x, so the transform writes frame-major records of CS_CHANNELS floats into the
// context's training scratch and a tiled transpose moves them into x.  The scratch does not grow with the clip: a call runs in slabs of
// at most CS_CAP_UNITS units of CS_TILE_T frames of one row (128 x 32 x 4098 floats = 67 MB).  Rows go in blocks of
// rows_per_block = min(R, CS_CAP_UNITS); a block's frames go in slabs of frames_per_slab = CS_TILE_T * (CS_CAP_UNITS / rows_per_block)
// frames (1 row: 4096 frames, 4 rows: 1024, 80 rows: 32, 128 rows and more: 32).  Slab s = (row block s / frame_slabs, frame slab
// s % frame_slabs) owns rows [r0, r1) x frames [t0, t1) (cs_slab); every (row, frame) belongs to exactly one slab.  Inside a slab one
// workgroup walks CS_CHUNK consecutive frames of one row from the slab's first frame on (at most 1024 workgroups per launch: one round of
// four per CU), and the transpose moves tiles of CS_TILE_B bins x CS_TILE_T frames.  Slab and chunk starts are multiples of CS_CHUNK, and a
// frame's arithmetic does not depend on where in a chunk, slab or launch it sits.
#pragma once
#include <math.h>
#include <stdint.h>

namespace bsrnn {

constexpr int CS_NFFT = 4096;                         // points of the real transform
constexpr int CS_HOP = 1024;
constexpr int CS_BINS = CS_NFFT / 2 + 1;              // 2049 one-sided bins
constexpr int CS_CHANNELS = 2 * CS_BINS;              // 4098 rows of x per wave row: the critic's in_channels
constexpr int CS_CHUNK = 4;                           // consecutive frames of one row per workgroup
constexpr int CS_TILE_T = 32, CS_TILE_B = 64;         // frames x bins of a transpose tile
constexpr int CS_CAP_UNITS = 128;                     // units of CS_TILE_T frames of one row the scratch holds at most
constexpr int64_t CS_MAX_ELEMS = ((int64_t)1 << 31) - 1;      // elements of x (grid sizes and frame counts are 32-bit)

inline int64_t cs_frames(int64_t n) { return 1 + n / CS_HOP; }

// Clip sample behind padded index idx (= t * 1024 + i - 2048), for n > 2048 and every frame t < cs_frames(n): in [0, n)
inline int64_t cs_reflect(int64_t idx, int64_t n)
{
    if (idx < 0) idx = -idx;
    if (idx >= n) idx = 2 * (n - 1) - idx;
    return idx;
}
inline int64_t cs_sample(int64_t t, int i, int64_t n) { return cs_reflect(t * CS_HOP + i - CS_NFFT / 2, n); }

struct CsPlan {
    int T;                           // frames per row
    int rows_per_block, row_blocks;
    int frames_per_slab, frame_slabs;
    int slabs;                       // row_blocks * frame_slabs launches of the transform and of the transpose
    int64_t scratch_floats;          // rows_per_block * min(T, frames_per_slab) * CS_CHANNELS, at most CS_CAP_UNITS * CS_TILE_T * CS_CHANNELS
};
struct CsSlab { int r0, r1, t0, t1; };

// (for arguments cs_check accepts)
inline CsPlan cs_plan(int R, int64_t n)
{
    CsPlan p{};
    p.T = (int)cs_frames(n);
    p.rows_per_block = R < CS_CAP_UNITS ? R : CS_CAP_UNITS;
    p.row_blocks = (R + p.rows_per_block - 1) / p.rows_per_block;
    p.frames_per_slab = CS_TILE_T * (CS_CAP_UNITS / p.rows_per_block);
    p.frame_slabs = (p.T + p.frames_per_slab - 1) / p.frames_per_slab;
    p.slabs = p.row_blocks * p.frame_slabs;
    p.scratch_floats = (int64_t)p.rows_per_block * (p.T < p.frames_per_slab ? p.T : p.frames_per_slab) * CS_CHANNELS;
    return p;
}
inline CsSlab cs_slab(const CsPlan& p, int R, int s)
{
    const int rb = s / p.frame_slabs, fs = s % p.frame_slabs;
    CsSlab q;
    q.r0 = rb * p.rows_per_block;
    q.r1 = q.r0 + p.rows_per_block < R ? q.r0 + p.rows_per_block : R;
    q.t0 = fs * p.frames_per_slab;
    q.t1 = q.t0 + p.frames_per_slab < p.T ? q.t0 + p.frames_per_slab : p.T;
    return q;
}

enum CsWhy {
    CS_OK = 0,
    CS_BAD_ROWS,             // R < 1
    CS_TOO_SHORT,            // n <= 2048: a reflection would leave the clip
    CS_BAD_STRIDE,           // wave_stride < n
    CS_BAD_SCALE,            // scale is not finite
    CS_TOO_LARGE,            // R * 4098 * T > CS_MAX_ELEMS
};
// bsrnn_critic_spectrum_layout asks without a wave: stride = n, scale = 1
inline int cs_check(int64_t R, int64_t n, int64_t stride, float scale)
{
    if (R < 1) return CS_BAD_ROWS;
    if (n <= CS_NFFT / 2) return CS_TOO_SHORT;
    if (stride < n) return CS_BAD_STRIDE;
    if (!isfinite(scale)) return CS_BAD_SCALE;
    // (T <= CS_MAX_ELEMS / 4098 first: the product below then fits int64 for every R)
    const int64_t T = cs_frames(n);
    if (R > CS_MAX_ELEMS || T > CS_MAX_ELEMS / CS_CHANNELS || R * CS_CHANNELS * T > CS_MAX_ELEMS) return CS_TOO_LARGE;
    return CS_OK;
}

}  // namespace bsrnn
