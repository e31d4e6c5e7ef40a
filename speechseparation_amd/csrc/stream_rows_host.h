// Row sets of the streaming rows calls (bsrnn_stream_process_rows, bsrnn_stream_reset_rows): which of a stream's C rows a call means
// travels BY VALUE in the kernel arguments, as a fixed bitset - no allocation, no staging copy, and nothing that has to outlive the call
// under the deferred range policy.  256 bytes of kernel arguments; that caps those calls at STREAM_ROWS_MAX rows.
// Host-only arithmetic (no HIP types): api_stream.hip packs, fft.hip tests bits, tests/cpp/stream_rows_check.cpp checks both with g++.
// RowHops (bsrnn_stream_process_hops): how many hops each row advances, by value in the same way - 8 bits per row, 2 KB of kernel
// arguments, which is why that call takes at most STREAM_HOPS_MAX hops (tests/cpp/stream_hops_check.cpp).
#pragma once
#include <cstdint>

namespace bsrnn {

constexpr int STREAM_ROWS_MAX = 2048;      // BSRNN_STREAM_ROWS_MAX of include/bsrnn_hip.h

struct RowSet { uint32_t w[STREAM_ROWS_MAX / 32]; };      // bit r & 31 of word r >> 5 = row r

constexpr bool row_set_has(const RowSet& s, int r) { return (s.w[r >> 5] >> (r & 31)) & 1u; }

// active[C] (nonzero = in the set; null = every row) -> set; bits of rows >= C are zero.  Returns how many rows are in the set, or -1
// when C is outside [1, STREAM_ROWS_MAX] (the set is then empty).
inline int pack_row_set(const uint8_t* active, int C, RowSet& out)
{
    for (uint32_t& w : out.w) w = 0;
    if (C < 1 || C > STREAM_ROWS_MAX) return -1;
    int n = 0;
    for (int r = 0; r < C; ++r) {
        if (active && !active[r]) continue;
        out.w[r >> 5] |= 1u << (r & 31);
        ++n;
    }
    return n;
}

// rows[n] (each in [0, C); a row may be named twice) -> set.  Returns -1 when every entry is good, else the index of the first bad one
// (n itself when C is outside [1, STREAM_ROWS_MAX]); the set is then unspecified.
inline int pack_row_list(const int32_t* rows, int n, int C, RowSet& out)
{
    for (uint32_t& w : out.w) w = 0;
    if (C < 1 || C > STREAM_ROWS_MAX) return n;
    for (int i = 0; i < n; ++i) {
        const int32_t r = rows[i];
        if (r < 0 || r >= C) return i;
        out.w[r >> 5] |= 1u << (r & 31);
    }
    return -1;
}

constexpr int STREAM_HOPS_MAX = 255;       // BSRNN_STREAM_HOPS_MAX of include/bsrnn_hip.h: a count fits 8 bits

struct RowHops { uint32_t w[STREAM_ROWS_MAX / 4]; };      // bits 8 (r & 3) .. 8 (r & 3) + 7 of word r >> 2 = hops of row r

// the one accessor, of the host and of the kernels
constexpr int row_hops_of(const RowHops& t, int r) { return (int)((t.w[r >> 2] >> (8 * (r & 3))) & 0xffu); }

// What pack_row_hops found: how many rows have at least one hop, and whether every count is 0 or n_hops (then the call is a rows call:
// bsrnn_stream_process_rows with active = hops != 0).
struct RowHopsInfo { int rows_with_hops; bool all_or_none; };

// hops[C] (each in [0, n_hops]) -> table; counts of rows >= C are zero.  Returns -1 when every entry is good, else the index of the first
// bad one - C itself when C is outside [1, STREAM_ROWS_MAX] or n_hops outside [1, STREAM_HOPS_MAX]; the table is then unspecified.
inline int pack_row_hops(const int32_t* hops, int C, int n_hops, RowHops& out, RowHopsInfo& info)
{
    for (uint32_t& w : out.w) w = 0;
    info.rows_with_hops = 0;
    info.all_or_none = true;
    if (C < 1 || C > STREAM_ROWS_MAX || n_hops < 1 || n_hops > STREAM_HOPS_MAX) return C;
    for (int r = 0; r < C; ++r) {
        const int32_t h = hops[r];
        if (h < 0 || h > n_hops) return r;
        out.w[r >> 2] |= (uint32_t)h << (8 * (r & 3));
        info.rows_with_hops += h != 0;
        info.all_or_none = info.all_or_none && (h == 0 || h == n_hops);
    }
    return -1;
}

// Floats of one row's carry as bsrnn_stream_get_row / _set_row move it: buf[2048], prev[2048], state[4][2][K][64]
inline int64_t stream_row_floats(int K) { return 2 * 2048 + (int64_t)8 * K * 64; }

}  // namespace bsrnn
