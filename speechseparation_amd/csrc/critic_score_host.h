// The committed critic (bsrnn_critic_*; reference bsrnn.py:512-536 under no_grad): the layout of the first layer's fp16x2 weight image,
// the channel map of an interleaved input, the tiling and K slabs of the fp16x2 forward, the workspace of a score and the argument
// verdicts, as integer arithmetic on the host.  HIP-free: api_critic.hip checks and plans a call with it, critic_score.hip takes the plan
// by value, tests/cpp/critic_score_check.cpp compiles it alone.  Everything is a function of (in_channels, C, T) only, so the order of
// every sum - and with it every bit of a score - is the same from run to run.
//
// THE PRODUCT.  Layer 1 of the critic (critic_host.h, "THE DEFINITION", O = 1024) with M = o, N = t, K = (i, k) on
// v_mfma_f32_32x32x16_f16: one MFMA consumes the 16 taps of one input channel.  Both operands are fp16x2 (gemm.hip, Piece<2>):
// a ~ a1 + 2^-11 a2, hi += a1 b1, lo += a1 b2 + a2 b1, result hi + 2^-11 lo.
//
// THE IMAGE.  W [1024][I][16] is split once (critic_commit_kernel) and stored in the order the forward's A fragments are read.  The A
// operand of the MFMA: lane (r = l & 31, h = l >> 5) holds the 8 halves A[r][8 h .. 8 h + 7].  One block of the image is what a
// workgroup (a tile of CSC_TILE_O = 128 output channels) stages per input channel:
//     [o tile ot = o / 128][channel i < I_pad][piece][sub-tile s = (o % 128) / 32][lane l = o % 32 + 32 (k / 8)][j = k % 8]
// 4096 halves = 8 KB per (ot, i), read and written as 16-byte units.  I_pad rounds I up to the CSC_CH = 2 channels of a stage; the
// channels [I, I_pad) of the image are zeros.
#pragma once
#include "critic_host.h"      // (constexpr functions below: the kernels call them too)

namespace bsrnn {

constexpr int CSC_O = CRITIC_WIDTHS[0];               // 1024 output channels of the first layer
constexpr int CSC_TILE_O = 128, CSC_TILE_T = 128;     // a workgroup's tile: 4 waves as 2 (o) x 2 (t), 64 x 64 each
constexpr int CSC_CH = 2;                             // input channels per LDS stage
constexpr int CSC_BLOCK = 2 * CSC_TILE_O * CRITIC_TAPS;       // halves of the image per (o tile, channel): both pieces
constexpr int CSC_FILL = 512;                         // workgroups a launch aims at: two per CU
constexpr int CSC_MIN_SLAB = 8;                       // never under 8 channels (128 products) per slab
constexpr int CSC_ORDER_PLANAR = 0, CSC_ORDER_INTERLEAVED = 1;
constexpr float CSC_F16_MAX = 65504.f;

constexpr int csc_i_pad(int I) { return (I + CSC_CH - 1) / CSC_CH * CSC_CH; }
constexpr int64_t csc_image_halves(int I) { return (int64_t)(CSC_O / CSC_TILE_O) * csc_i_pad(I) * CSC_BLOCK; }

// Position (in halves) of piece `piece` of W[o][i][k] in the image; i < csc_i_pad(I)
constexpr int64_t csc_image_index(int I, int o, int i, int k, int piece)
{
    const int ot = o / CSC_TILE_O, s = (o % CSC_TILE_O) / 32, lane = o % 32 + 32 * (k / 8), j = k % 8;
    return ((int64_t)ot * csc_i_pad(I) + i) * CSC_BLOCK + (int64_t)piece * (CSC_BLOCK / 2) + s * 512 + lane * 8 + j;
}
// The inverse: (o, i, k, piece) of position p; returns false when p is padding (i >= I), whose value is zero
constexpr bool csc_image_source(int I, int64_t p, int* o, int* i, int* k, int* piece)
{
    const int64_t blk = p / CSC_BLOCK;
    const int r = (int)(p % CSC_BLOCK), w = r % (CSC_BLOCK / 2), s = w / 512, lane = (w % 512) / 8, j = w % 8;
    *piece = r / (CSC_BLOCK / 2);
    *i = (int)(blk % csc_i_pad(I));
    *o = (int)(blk / csc_i_pad(I)) * CSC_TILE_O + 32 * s + lane % 32;
    *k = 8 * (lane / 32) + j;
    return *i < I;
}

// Row of x that channel i of the critic reads.  Planar: x is [C][I][T] in the reference's order (all real parts, then all imaginary
// parts).  Interleaved: x is the separator's spectrum (re, im, re, im, ...), F = I / 2 bins: channel i < F is the real part of bin i.
constexpr int csc_channel_row(int I, int i, int x_order)
{
    if (x_order != CSC_ORDER_INTERLEAVED) return i;
    const int F = I / 2;
    return i < F ? 2 * i : 2 * (i - F) + 1;
}

struct CscPlan {
    int I, C, T;
    int len[CRITIC_LAYERS];          // frames behind the four layers
    int t_tiles, o_tiles;            // tiles of 128 frames per row, of 128 output channels
    // K = (i, k) is cut into `slabs` runs of `ch_per_slab` input channels (a multiple of CSC_CH; the last run may be shorter); slab s owns
    // channels [s * ch_per_slab, min(I, (s + 1) * ch_per_slab)).  A slab's partial sum is hi + 2^-11 lo of its channels in channel order;
    // the partial sums are added in slab order, then the bias, then the activation.
    int slabs, ch_per_slab;
    // Workspace in floats: [y1 | y2 | y3 | y4 | shared], `shared` the larger of the fp16x2 partial sums [slabs][C][1024][len[0]] and the
    // scratch of the exact layers (critic_forward_scratch_floats of all four: the re-run needs the first too).  The exact chain of an
    // interleaved input first copies x into the reference's order behind it: ws_exact_floats = ws_floats + C * I * T.
    int64_t off_y[CRITIC_LAYERS], off_shared, ws_floats, ws_exact_floats;
};

inline int64_t csc_round4(int64_t v) { return (v + 3) / 4 * 4; }

inline CscPlan csc_plan(int I, int C, int T)
{
    CscPlan p{};
    p.I = I; p.C = C; p.T = T;
    critic_chain(T, p.len);
    p.t_tiles = critic_ceil(p.len[0], CSC_TILE_T);
    p.o_tiles = CSC_O / CSC_TILE_O;
    const int64_t tiles = (int64_t)C * p.t_tiles * p.o_tiles;
    int64_t want = tiles >= CSC_FILL ? 1 : (CSC_FILL + tiles - 1) / tiles;
    const int most = I / CSC_MIN_SLAB;
    if (want > most) want = most;
    if (want < 1) want = 1;
    p.ch_per_slab = critic_ceil(critic_ceil(I, (int)want), CSC_CH) * CSC_CH;
    p.slabs = critic_ceil(I, p.ch_per_slab);
    int64_t at = 0, shared = (int64_t)p.slabs * C * CSC_O * p.len[0];
    int in = I, t = T;
    for (int l = 0; l < CRITIC_LAYERS; ++l) {
        p.off_y[l] = at;
        at += csc_round4((int64_t)C * CRITIC_WIDTHS[l] * p.len[l]);
        const int64_t s = critic_forward_scratch_floats(C, in, t, CRITIC_WIDTHS[l]);
        if (s > shared) shared = s;
        in = CRITIC_WIDTHS[l]; t = p.len[l];
    }
    p.off_shared = at;
    p.ws_floats = at + csc_round4(shared);
    p.ws_exact_floats = p.ws_floats + (int64_t)C * I * T;
    return p;
}

enum CscWhy {
    CSC_OK = 0,
    CSC_BAD_CHANNELS,        // in_channels < 1
    CSC_BAD_ROWS,            // C < 1
    CSC_TOO_SHORT,           // T < CRITIC_MIN_T: the input does not reach the last layer
    CSC_BAD_ORDER,           // x_order outside {planar, interleaved}
    CSC_ODD_INTERLEAVED,     // an interleaved input has an even number of channels
    CSC_TOO_LARGE,           // x, the image, a layer's output or the workspace would pass 2^31 - 1 elements
};
inline int csc_check_channels(int64_t I)
{
    if (I < 1) return CSC_BAD_CHANNELS;
    if (I > CRITIC_MAX_ELEMS || (I + 1) * CSC_O * CRITIC_TAPS > CRITIC_MAX_ELEMS) return CSC_TOO_LARGE;      // W and one piece of the image
    return CSC_OK;
}
inline int csc_check(int64_t I, int64_t C, int64_t T, int64_t x_order)
{
    if (int why = csc_check_channels(I)) return why;
    if (C < 1) return CSC_BAD_ROWS;
    if (T < CRITIC_MIN_T) return CSC_TOO_SHORT;
    if (x_order != CSC_ORDER_PLANAR && x_order != CSC_ORDER_INTERLEAVED) return CSC_BAD_ORDER;
    if (x_order == CSC_ORDER_INTERLEAVED && I % 2) return CSC_ODD_INTERLEAVED;
    if (C > CRITIC_MAX_ELEMS || T > CRITIC_MAX_ELEMS) return CSC_TOO_LARGE;
    if (critic_check(C, I, T, CSC_O) != CRITIC_OK) return CSC_TOO_LARGE;
    if (csc_plan((int)I, (int)C, (int)T).ws_exact_floats > CRITIC_MAX_ELEMS) return CSC_TOO_LARGE;
    return CSC_OK;
}

}  // namespace bsrnn
