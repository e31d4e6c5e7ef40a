// The committed critic's gradient (bsrnn_critic_enable_grad / _score_grad / _layer1_dx): the layout of the first layer's SECOND fp16x2 weight
// image, the tiling of the fp16x2 dx, the workspace of a score with its gradient and the argument verdicts, as integer arithmetic on the
// host.  HIP-free: api_critic.hip checks and plans a call with it, critic_grad.hip takes the plan by value, tests/cpp/critic_grad_check.cpp
// compiles it alone.  Everything is a function of (in_channels, C, T) only, so the order of every sum - and with it every bit of a
// gradient - is the same from run to run.
//
// THE PRODUCT.  dx of layer 1 (critic_host.h, "THE DEFINITION", O = 1024) for row c:
//     G[(i, k)][t] = sum_o W[o][i][k] * dp1[c][o][t]                      M = (i, k), N = t, K = o = 1024 on v_mfma_f32_32x32x16_f16
//     dx[c][i][s]  = sum over the taps k = s % 3, s % 3 + 3, ... < 16 (in that order) of G[(i, k)][(s - k) / 3]      frames outside [0, T1) are zeros
// Both operands are fp16x2 (gemm.hip, Piece<2>): hi += a1 b1, lo += a1 b2 + a2 b1, G = hi + 2^-11 lo.  dp1 is a gradient through two means,
// far below fp16's normal range: the kernel multiplies it by 2^e, e = 14 - floor(log2 max |dp1|) (the maximum recorded on the device by the
// pass that forms dp1), which puts the largest operand into [2^14, 2^15), and multiplies the folded result by 2^-e.  Both are exact.
//
// THE IMAGE.  An operand of the 32x32x16 MFMA holds 8 consecutive K values per lane, and K is o here (the forward's image,
// critic_score_host.h, holds 8 consecutive taps per lane: it cannot serve).  The same two pieces of W [1024][I][16], in the order this
// product's A fragments are read: lane (r = l & 31, h = l >> 5) holds A[r][8 h .. 8 h + 7].  One block is what a workgroup (a tile of
// CGD_CH = 8 input channels = 128 rows m = 16 (i % 8) + k) stages per 16 output channels:
//     [channel tile it = i / 8][o block ob = o / 16][piece][sub-tile s = m / 32][lane l = m % 32 + 32 ((o % 16) / 8)][j = o % 8]
// 4096 halves = 8 KB per (it, ob), read and written as 16-byte units.  The channels [I, cgd_i_pad(I)) of the image are zeros.
#pragma once
#include "critic_score_host.h"

namespace bsrnn {

constexpr int CGD_CH = 8;                                         // input channels of a tile: 8 x 16 taps = 128 rows of the product
constexpr int CGD_TILE_T = 128;                                   // frames of dp1 under a tile: four waves as 2 (m) x 2 (t), 64 x 64 each
constexpr int CGD_HALO = CRITIC_DX_HALO;                          // a tile of 128 frames completes 3 * 123 = 369 input positions ...
constexpr int CGD_TILE_S = CRITIC_STRIDE * (CGD_TILE_T - CGD_HALO);      // ... [369 n, 369 n + 369) from frames [123 n - 5, 123 n + 123)
constexpr int CGD_KB = 16;                                        // output channels per block of the image: one MFMA's K
constexpr int CGD_STAGE_O = 32;                                   // output channels per LDS stage: two blocks
constexpr int CGD_MAX_TARGET = 14;                                // the scaled maximum of dp1 lies in [2^14, 2^15)

constexpr int cgd_i_pad(int I) { return (I + CGD_CH - 1) / CGD_CH * CGD_CH; }
constexpr int64_t cgd_image_halves(int I) { return (int64_t)(cgd_i_pad(I) / CGD_CH) * (CSC_O / CGD_KB) * CSC_BLOCK; }

// Position (in halves) of piece `piece` of W[o][i][k] in the dx image; i < cgd_i_pad(I)
constexpr int64_t cgd_image_index(int I, int o, int i, int k, int piece)
{
    (void)I;
    const int it = i / CGD_CH, m = (i % CGD_CH) * CRITIC_TAPS + k, ob = o / CGD_KB, s = m / 32, lane = m % 32 + 32 * ((o % CGD_KB) / 8), j = o % 8;
    return ((int64_t)it * (CSC_O / CGD_KB) + ob) * CSC_BLOCK + (int64_t)piece * (CSC_BLOCK / 2) + s * 512 + lane * 8 + j;
}
// The inverse: (o, i, k, piece) of position p; returns false when p is padding (i >= I), whose value is zero
constexpr bool cgd_image_source(int I, int64_t p, int* o, int* i, int* k, int* piece)
{
    const int64_t blk = p / CSC_BLOCK;
    const int r = (int)(p % CSC_BLOCK), w = r % (CSC_BLOCK / 2), s = w / 512, lane = (w % 512) / 8, j = w % 8;
    const int m = 32 * s + lane % 32;
    *piece = r / (CSC_BLOCK / 2);
    *o = (int)(blk % (CSC_O / CGD_KB)) * CGD_KB + 8 * (lane / 32) + j;
    *i = (int)(blk / (CSC_O / CGD_KB)) * CGD_CH + m / CRITIC_TAPS;
    *k = m % CRITIC_TAPS;
    return *i < I;
}

// The tile that owns input position s of a row, the positions it owns and the first of its 128 frames (may be negative: zeros)
constexpr int cgd_tile_of(int s) { return s / CGD_TILE_S; }
constexpr int cgd_tile_first(int bs) { return bs * CGD_TILE_S; }
constexpr int cgd_tile_frame0(int bs) { return bs * (CGD_TILE_T - CGD_HALO) - CGD_HALO; }
// The column (frame - frame0) of a tile's product that position cgd_tile_first(bs) + d takes tap k from (k % 3 == d % 3); inside [0, 128)
constexpr int cgd_fold_column(int d, int k) { return CGD_HALO + (d - k) / CRITIC_STRIDE; }

// The power of two the dx kernel scales dp1 by, from the bit pattern of max |dp1| (0 for a zero, an infinite or a NaN maximum)
constexpr int cgd_scale_exponent(uint32_t max_bits)
{
    if (max_bits == 0 || max_bits >= 0x7f800000u) return 0;
    int e = (int)(max_bits >> 23) - 127;                          // floor(log2) of a normal number
    if (max_bits < 0x00800000u) {                                 // a subnormal maximum: the position of its top bit
        e = -127;
        for (uint32_t v = max_bits; v < 0x00800000u; v <<= 1) --e;
        e += 1;
    }
    return CGD_MAX_TARGET - e;
}

struct CgdPlan {
    CscPlan f;                       // the forward: y1 .. y4 and the shared block (which holds a layer's dy between its dx and its leaky pass)
    int i_tiles, s_tiles;            // tiles of 8 input channels, of 369 input positions per row: one workgroup each per row, over the whole K
    // Workspace in floats on top of the forward's: [f.ws_floats | dp1 | dp2 | dp3 | dp4 | pooled gradient (32) | max word (4)], and behind
    // them what only the exact chain of an INTERLEAVED input needs: the planar copy of x and the planar dx, C * I * T each.
    int64_t off_dp[CRITIC_LAYERS], off_pool, off_max, ws_floats, off_xp, off_dxp, ws_exact_floats;
};

inline CgdPlan cgd_plan(int I, int C, int T)
{
    CgdPlan g{};
    g.f = csc_plan(I, C, T);
    g.i_tiles = cgd_i_pad(I) / CGD_CH;
    g.s_tiles = critic_ceil(T, CGD_TILE_S);
    int64_t at = g.f.ws_floats;
    for (int l = 0; l < CRITIC_LAYERS; ++l) { g.off_dp[l] = at; at += csc_round4((int64_t)C * CRITIC_WIDTHS[l] * g.f.len[l]); }
    g.off_pool = at; at += CRITIC_WIDTHS[CRITIC_LAYERS - 1];
    g.off_max = at; at += 4;
    g.ws_floats = at;
    g.off_xp = at; at += csc_round4((int64_t)C * I * T);
    g.off_dxp = at; at += csc_round4((int64_t)C * I * T);
    g.ws_exact_floats = at;
    return g;
}

enum CgdWhy {
    CGD_OK = 0,
    CGD_BAD_CHANNELS,        // in_channels < 1
    CGD_BAD_ROWS,            // C < 1
    CGD_TOO_SHORT,           // T < CRITIC_MIN_T
    CGD_BAD_ORDER,           // x_order outside {planar, interleaved}
    CGD_ODD_INTERLEAVED,     // an interleaved input has an even number of channels
    CGD_TOO_LARGE,           // a tensor of the call, the dx image, the workspace or the grid would pass 2^31 - 1 elements
};
inline int cgd_check_channels(int64_t I)
{
    if (int why = csc_check_channels(I)) return why == CSC_BAD_CHANNELS ? CGD_BAD_CHANNELS : CGD_TOO_LARGE;
    if ((I + CGD_CH) * CSC_O * CRITIC_TAPS > CRITIC_MAX_ELEMS) return CGD_TOO_LARGE;          // one piece of the dx image
    return CGD_OK;
}
inline int cgd_check(int64_t I, int64_t C, int64_t T, int64_t x_order)
{
    switch (csc_check(I, C, T, x_order)) {
    case CSC_OK: break;
    case CSC_BAD_CHANNELS: return CGD_BAD_CHANNELS;
    case CSC_BAD_ROWS: return CGD_BAD_ROWS;
    case CSC_TOO_SHORT: return CGD_TOO_SHORT;
    case CSC_BAD_ORDER: return CGD_BAD_ORDER;
    case CSC_ODD_INTERLEAVED: return CGD_ODD_INTERLEAVED;
    default: return CGD_TOO_LARGE;
    }
    if (int why = cgd_check_channels(I)) return why;
    const CgdPlan g = cgd_plan((int)I, (int)C, (int)T);
    if (g.ws_exact_floats > CRITIC_MAX_ELEMS) return CGD_TOO_LARGE;
    if ((int64_t)g.i_tiles * g.s_tiles * C > CRITIC_MAX_ELEMS) return CGD_TOO_LARGE;
    return CGD_OK;
}

}  // namespace bsrnn
