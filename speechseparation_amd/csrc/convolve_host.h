// Long FIR convolution of rows of different lengths (bsrnn_fir_bank_*, bsrnn_convolve_ragged): the definition and the plan, as integer
// arithmetic on the host.  HIP-free: api_resample.hip plans a call with it, fft.hip takes ConvRow by value, tests/cpp/convolve_plan_check.cpp
// compiles it alone.
//
// THE DEFINITION is torch.nn.functional.conv1d(x, h, padding='same') (m_dataset.py:92-114 applies a room impulse response with it): for a
// row x of n samples and a filter h of k taps, left = (k - 1) / 2,
//     y[m] = sum_{j < k} x[m + j - left] h[j],      x = 0 outside [0, n),      m in [0, n)
// - a cross-correlation, the extra sample of padding on the right for even k.  With g[i] = h[k - 1 - i] and shift = k / 2 this is
//     y[m] = (x * g)[m + shift].
// THE SCHEME is a uniformly partitioned overlap-save convolution on the library's 2048-point real FFT: B = 1024, g in P = ceil(k / B)
// partitions of B taps, each zero-padded to 2048 and transformed once (the filter image [P][1025] complex).  Input frame v holds
// x[(v - 1) B, (v + 1) B); block u of x * g - its samples [u B, (u + 1) B) - is the second half of
//     irfft(sum_{p <= min(P - 1, u)} X[u - p] H[p]),
// summed over p ascending.  A row needs blocks shift / B ... (n - 1 + shift) / B, stored shift samples to the left and clipped to [0, n).
// Frames past the row's end are zero and are neither transformed nor read: a block's sum skips their partitions, which changes no bit.
#pragma once
#include <stdint.h>

#include <vector>

namespace bsrnn {

constexpr int CONV_B = 1024;                          // block length = hop of both walks = taps per partition
constexpr int CONV_LD = 2050;                         // floats per spectrum of the workspace and of the filter images: 1025 (re, im), no padding
constexpr int CONV_MAX_TAPS = 262144;                 // 1 <= k <= this (5.9 s at 44.1 kHz, 256 partitions)
constexpr int64_t CONV_MAX_LEN = (int64_t)1 << 40;    // 1 <= n <= this: frame and block numbers fit an int
constexpr int64_t CONV_FRAME_BUDGET = 65536;          // spectra per workspace buffer before a call is split into row groups (0.5 GB each)
constexpr int CONV_GROUP_ROWS = 32768;                // ... and rows per group (a grid dimension)
#ifndef BSRNN_CONV_TILE
#define BSRNN_CONV_TILE 16                            // (-DBSRNN_CONV_TILE=8 builds the variant profiles/convolve_bench.txt compares: 8 - 11 % slower)
#endif
constexpr int CONV_TILE = BSRNN_CONV_TILE;            // consecutive blocks one multiply-accumulate thread owns

inline int conv_partitions(int k) { return (k + CONV_B - 1) / CONV_B; }
inline int64_t conv_left(int k) { return (k - 1) / 2; }
inline int64_t conv_shift(int k) { return k / 2; }
inline int64_t conv_image_floats(int k) { return (int64_t)conv_partitions(k) * CONV_LD; }

// What a row of n samples under a filter of k taps computes: blocks [u0, u1] (nb of them) from input frames [f0, f1] (nx of them).
struct ConvPlan { int P; int64_t shift, u0, u1, nb, f0, f1, nx; };
inline ConvPlan conv_plan(int64_t n, int k)
{
    ConvPlan q;
    q.P = conv_partitions(k);
    q.shift = conv_shift(k);
    q.u0 = q.shift / CONV_B;
    q.u1 = (n - 1 + q.shift) / CONV_B;
    q.nb = q.u1 - q.u0 + 1;
    // the last frame a block reads a sample of the row from: the kept half of a product never sees a frame's sample 0, so frame v counts
    // from x[(v - 1) B + 1] on
    const int64_t last = (n + CONV_B - 2) / CONV_B;
    q.f0 = q.u0 - (q.P - 1) > 0 ? q.u0 - (q.P - 1) : 0;
    q.f1 = q.u1 < last ? q.u1 : last;
    q.nx = q.f1 - q.f0 + 1;
    return q;
}
// block u stores y[m0, m1): its samples [u B, (u + 1) B) moved left by shift, clipped to the row
struct ConvStore { int64_t m0, m1; };
inline ConvStore conv_store(const ConvPlan& q, int64_t n, int64_t u)
{
    const int64_t a = u * CONV_B - q.shift, b = a + CONV_B;
    return {a > 0 ? a : 0, b < n ? b : n};
}
// the partitions block u sums, ascending: those whose frame u - p lies in [f0, f1]
struct ConvSpan { int64_t p_lo, p_hi; };
inline ConvSpan conv_span(const ConvPlan& q, int64_t u)
{
    const int64_t lo = u - q.f1, hi = u < q.P - 1 ? u : q.P - 1;
    return {lo > 0 ? lo : 0, hi};
}
// number of 1024-sample pieces of a row that is copied (filter -1)
inline int64_t conv_copy_blocks(int64_t n) { return (n + CONV_B - 1) / CONV_B; }

// Row groups: consecutive rows whose spectra fit the budget in both buffers (nx[r] input frames, nb[r] blocks; a copied row has none).
// and at most CONV_GROUP_ROWS rows.  A group holds at least one row, so a single row beyond the budget is a group of its own and the workspace grows for it.
struct ConvGroup { int first, rows; int64_t x_frames, y_frames; };
inline std::vector<ConvGroup> conv_groups(const int64_t* nx, const int64_t* nb, int R, int64_t budget = CONV_FRAME_BUDGET)
{
    std::vector<ConvGroup> out;
    ConvGroup g{0, 0, 0, 0};
    for (int r = 0; r < R; ++r) {
        if (g.rows > 0 && (g.rows == CONV_GROUP_ROWS || g.x_frames + nx[r] > budget || g.y_frames + nb[r] > budget)) {
            out.push_back(g);
            g = ConvGroup{r, 0, 0, 0};
        }
        ++g.rows; g.x_frames += nx[r]; g.y_frames += nb[r];
    }
    out.push_back(g);
    return out;
}

// What the three kernels know of a row, by index in a table on the device.  H = null: the row is copied (nb pieces of 1024 samples,
// u0 = shift = nx = 0).  xoff / yoff: the row's first spectrum in the group's two buffers.
struct ConvRow {
    const float* H;          // the filter's image [P][CONV_LD]
    int64_t n, shift, xoff, yoff;
    int P, u0, nb, f0, nx, pad_;
};

}  // namespace bsrnn
