// Row sets of the streaming rows calls (bsrnn_stream_process_rows, bsrnn_stream_reset_rows): which of a stream's C rows a call means
// travels BY VALUE in the kernel arguments, as a fixed bitset - no allocation, no staging copy, and nothing that has to outlive the call
// under the deferred range policy.  256 bytes of kernel arguments; that caps those calls at STREAM_ROWS_MAX rows.
// Host-only arithmetic (no HIP types): api.hip packs, fft.hip tests bits, tests/cpp/stream_rows_check.cpp checks both with g++.
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

// Floats of one row's carry as bsrnn_stream_get_row / _set_row move it: buf[2048], prev[2048], state[4][2][K][64]
inline int64_t stream_row_floats(int K) { return 2 * 2048 + (int64_t)8 * K * 64; }

}  // namespace bsrnn
