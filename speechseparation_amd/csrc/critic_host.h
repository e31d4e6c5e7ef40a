// The critic's strided convolution (bsrnn_critic_conv_*; reference bsrnn.py:512-536: four Conv1d(kernel 16, stride 3) layers): the
// definition, the length chain of the four layers, the split of a layer's products into workgroups and the scratch that follows from it,
// as integer arithmetic on the host.  HIP-free: api_critic.hip checks and plans a call with it, critic.hip takes the layout by value,
// tests/cpp/critic_check.cpp compiles it alone.  Everything here is a function of the shape (C, I, T, O) only, so the order of every
// sum - and with it every bit of a result - is the same from run to run.
//
// THE DEFINITION.  x [C][I][T] (T contiguous), W [O][I][16], b [O] (torch's layouts), T_out = (T - 16) / 3 + 1:
//     y[c][o][t] = act(b[o] + sum_{i < I} sum_{k < 16} W[o][i][k] * x[c][i][3 t + k])          act = LeakyReLU(0.01) or the identity
// and with dp = dy * act'(y) (slope 0.01 where y <= 0, as leaky_bwd_kernel reads it off the output):
//     db[o] = sum_{c, t} dp[c][o][t]        dW[o][i][k] = sum_{c, t} dp[c][o][t] * x[c][i][3 t + k]
//     dx[c][i][s] = sum_o sum_{k < 16, (s - k) % 3 == 0, 0 <= (s - k) / 3 < T_out} W[o][i][k] * dp[c][o][(s - k) / 3]        for every s < T
#pragma once
#include <stdint.h>

namespace bsrnn {

constexpr int CRITIC_TAPS = 16;                       // kernel size of every layer
constexpr int CRITIC_STRIDE = 3;
constexpr int CRITIC_LAYERS = 4;
constexpr int CRITIC_WIDTHS[CRITIC_LAYERS] = {1024, 128, 64, 32};      // output channels of the four layers
constexpr int CRITIC_MIN_T = 601;                     // the shortest input that reaches the last layer: 601 -> 196 -> 61 -> 16 -> 1
constexpr int64_t CRITIC_MAX_ELEMS = ((int64_t)1 << 31) - 1;      // elements of any one tensor of a call (grid sizes and tile counts are 32-bit)

// Tiles of the three products (critic.hip).  Forward and dW stage CRITIC_CH input channels (64 values of K resp. N) per LDS slab.
constexpr int CRITIC_TILE = 64;                       // outputs t x output channels o of a forward tile; o x (channel, tap) of a dW tile
constexpr int CRITIC_CH = 4;                          // input channels per LDS stage: 4 x 16 taps = 64
constexpr int CRITIC_SPAN = CRITIC_STRIDE * (CRITIC_TILE - 1) + CRITIC_TAPS;      // 205 floats of x per channel under a tile of 64 outputs
constexpr int CRITIC_DW_FRAMES = 32;                  // frames t per LDS stage of the dW reduction
constexpr int CRITIC_DX_HALO = 5;                     // dx: a tile of 64 frames of dp completes 3 * 59 = 177 input positions ...
constexpr int CRITIC_DX_TILE = CRITIC_STRIDE * (CRITIC_TILE - CRITIC_DX_HALO);    // ... [177 n, 177 n + 177) from frames [59 n - 5, 59 n + 59)
constexpr int CRITIC_FILL = 1024;                     // workgroups a launch aims at when the shape allows: four per CU

inline int critic_t_out(int T) { return T < CRITIC_TAPS ? 0 : (T - CRITIC_TAPS) / CRITIC_STRIDE + 1; }

// The lengths behind the four layers; false when the input is too short to reach the last one (T < CRITIC_MIN_T)
inline bool critic_chain(int T, int out[CRITIC_LAYERS])
{
    for (int l = 0; l < CRITIC_LAYERS; ++l) {
        T = critic_t_out(T);
        out[l] = T;
        if (T < 1) { for (int m = l + 1; m < CRITIC_LAYERS; ++m) out[m] = 0; return false; }
    }
    return true;
}

struct CriticLayout {
    int T_out;
    // forward: K = (i, k) is cut into `slabs` runs of `ch_per_slab` input channels (a multiple of CRITIC_CH; the last run may be
    // shorter); slab s owns channels [s * ch_per_slab, min(I, (s + 1) * ch_per_slab)).  Inside a slab the products are added channel by
    // channel, tap by tap; the slabs' partial sums are added in slab order, then the bias.
    int slabs, ch_per_slab;
    int t_tiles, o_tiles;            // tiles of 64 frames per row c, tiles of 64 output channels
    // dW / db: the reduction over (c, t) runs in `dw_chunks` runs of `dw_frames` frames (a multiple of CRITIC_DW_FRAMES; the last may be
    // shorter); chunk z owns frames [z * dw_frames, min(T_out, (z + 1) * dw_frames)) of EVERY row c, added row by row, frame by frame; the
    // chunks' partial sums are added in chunk order.  One chunk: no partial records, the product is written in place.
    int dw_chunks, dw_frames;
    int i_tiles;                     // tiles of CRITIC_CH input channels (dW and dx)
    int s_tiles;                     // dx: tiles of CRITIC_DX_TILE input positions per row
};

inline int critic_ceil(int a, int b) { return (a + b - 1) / b; }

inline CriticLayout critic_layout(int C, int I, int T, int O)
{
    CriticLayout g{};
    g.T_out = critic_t_out(T);
    g.t_tiles = critic_ceil(g.T_out, CRITIC_TILE);
    g.o_tiles = critic_ceil(O, CRITIC_TILE);
    g.i_tiles = critic_ceil(I, CRITIC_CH);
    g.s_tiles = critic_ceil(T, CRITIC_DX_TILE);
    // forward: enough slabs to reach CRITIC_FILL workgroups, never under 8 channels (128 products) per slab
    const int64_t tiles = (int64_t)C * g.t_tiles * g.o_tiles;
    int64_t want = tiles >= CRITIC_FILL ? 1 : (CRITIC_FILL + tiles - 1) / tiles;
    const int most = critic_ceil(I, 2 * CRITIC_CH);
    if (want > most) want = most;
    if (want < 1) want = 1;
    g.ch_per_slab = critic_ceil(critic_ceil(I, (int)want), CRITIC_CH) * CRITIC_CH;
    g.slabs = critic_ceil(I, g.ch_per_slab);
    // dW: one chunk when the output alone fills the chip (the first layer: 16 x 1025 tiles), else about CRITIC_FILL workgroups, and
    // never more than 512 frames of a row per chunk
    const int64_t wt = (int64_t)g.o_tiles * g.i_tiles;
    int chunks = 1;
    if (wt < CRITIC_FILL) {
        chunks = (int)((CRITIC_FILL + wt - 1) / wt);
        const int by_len = critic_ceil(g.T_out, 512);
        if (chunks < by_len) chunks = by_len;
        const int cap = critic_ceil(g.T_out, CRITIC_DW_FRAMES);
        if (chunks > cap) chunks = cap;
        if (chunks > 256) chunks = 256;
    }
    g.dw_frames = critic_ceil(critic_ceil(g.T_out, chunks), CRITIC_DW_FRAMES) * CRITIC_DW_FRAMES;
    g.dw_chunks = critic_ceil(g.T_out, g.dw_frames);
    return g;
}

// Scratch of the two calls, in floats.  Forward: the slabs' partial sums [slabs][C][O][T_out].  Backward: dp [C][O][T_out] when leaky
// (the identity reads dy in place), then the chunks' records [dw_chunks][O * I * 16 | O] when there is more than one chunk.
inline int64_t critic_forward_scratch_floats(int C, int I, int T, int O)
{
    const CriticLayout g = critic_layout(C, I, T, O);
    return (int64_t)g.slabs * C * O * g.T_out;
}
inline int64_t critic_dw_record_floats(int I, int O) { return (int64_t)O * I * CRITIC_TAPS + O; }
inline int64_t critic_backward_scratch_floats(int C, int I, int T, int O, int leaky)
{
    const CriticLayout g = critic_layout(C, I, T, O);
    const int64_t dp = leaky ? ((int64_t)C * O * g.T_out + 3) / 4 * 4 : 0;
    return dp + (g.dw_chunks > 1 ? (int64_t)g.dw_chunks * critic_dw_record_floats(I, O) : 0);
}

enum CriticWhy {
    CRITIC_OK = 0,
    CRITIC_BAD_SIZE,         // C, I or O < 1
    CRITIC_TOO_SHORT,        // T < 16: no output frame
    CRITIC_TOO_LARGE,        // a tensor of the call (x, W, y) or the forward scratch has more than CRITIC_MAX_ELEMS elements
};
inline int critic_check(int64_t C, int64_t I, int64_t T, int64_t O)
{
    if (C < 1 || I < 1 || O < 1) return CRITIC_BAD_SIZE;
    if (T < CRITIC_TAPS) return CRITIC_TOO_SHORT;
    if (C > CRITIC_MAX_ELEMS || I > CRITIC_MAX_ELEMS || T > CRITIC_MAX_ELEMS || O > CRITIC_MAX_ELEMS) return CRITIC_TOO_LARGE;
    const int64_t To = critic_t_out((int)T);
    // (each factor is below 2^31, so a product of two fits int64; the third is applied after a division check)
    auto big = [](int64_t a, int64_t b, int64_t c) { return a * b > CRITIC_MAX_ELEMS || a * b * c > CRITIC_MAX_ELEMS; };
    if (big(C, I, T) || big(O, I, CRITIC_TAPS) || big(C, O, To)) return CRITIC_TOO_LARGE;
    if (critic_forward_scratch_floats((int)C, (int)I, (int)T, (int)O) > CRITIC_MAX_ELEMS) return CRITIC_TOO_LARGE;
    return CRITIC_OK;
}

}  // namespace bsrnn
