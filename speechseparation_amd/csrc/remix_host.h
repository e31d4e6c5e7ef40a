// The re-mix of an optimizer step (bsrnn_remix_ragged): the definition, the argument checks, the tile count and the traffic model, as
// integer arithmetic on the host.  HIP-free: api_resample.hip checks and plans a call with it, remix.hip takes the two descriptors by
// index in a table on the device, tests/cpp/remix_plan_check.cpp compiles it alone.
//
// THE DEFINITION is MixDataSet.__getitem__'s arithmetic (m_dataset.py:158-178) on sources that stay where they are.  A row of n samples
// owns a run of terms; the value of term t at output sample i is
//     v_t(i) = src[i - at] * gain   if 0 <= i - at < len,   else +0
// - at > 0 is random_resize's left padding, at < 0 its cut, the product one fp32 multiply.  The first term is the target (the dialog),
// the others the backgrounds, and for 0 <= i < n
//     target[i] = v_0(i),     mix[i] = v_0(i) + ((((+0 + v_1(i)) + v_2(i)) + ...)
// every + one fp32 addition in that order, no product fused into an addition: Python's `dialog + sum(backgrounds)`.  Both outputs are
// +0 for n <= i < width, and nothing is written behind width.
#pragma once
#include <stdint.h>

namespace bsrnn {

constexpr int REMIX_THREADS = 256;                    // lanes of a workgroup
constexpr int REMIX_PER_LANE = 8;                     // outputs a lane forms, REMIX_THREADS samples apart: every access a wave makes is 64 consecutive floats
constexpr int REMIX_TILE = REMIX_THREADS * REMIX_PER_LANE;      // consecutive outputs of one row a workgroup owns (BSRNN_REMIX_TILE)
constexpr int64_t REMIX_MAX_LEN = (int64_t)1 << 40;   // bound of width, of both strides, of a term's len and of |at|: no index sum leaves int64
constexpr int64_t REMIX_MAX_EXTENT = (int64_t)1 << 60;      // (R - 1) * stride stays below this (floats)

// The two tables of a call as the kernel reads them: the layout of bsrnn_remix_term / bsrnn_remix_row (api_resample.hip asserts it)
struct RemixTerm {
    const float* src;        // len floats on the device; null only with len == 0
    int64_t len, at;         // source sample j lands on output sample at + j
    float gain;
    int32_t pad_;
};
struct RemixRow {
    int64_t n;               // samples of the row that are formed; [n, width) is zeros
    int32_t first_term, n_terms;     // terms [first_term, first_term + n_terms) of the call's table, the target first
};

enum RemixWhy {
    REMIX_OK = 0,
    REMIX_NULL_TABLE,        // rows or terms is null
    REMIX_BAD_COUNT,         // R < 1 or n_terms < 1
    REMIX_BAD_WIDTH,         // width outside [0, REMIX_MAX_LEN]
    REMIX_MIX_STRIDE,        // mix_stride < width, or beyond the bounds
    REMIX_TARGET_STRIDE,     // target_stride likewise
    REMIX_ROW_LENGTH,        // rows[index].n outside [0, width]
    REMIX_ROW_TERMS,         // rows[index] owns no term, or its range leaves [0, n_terms)
    REMIX_TERM_LENGTH,       // terms[index].len outside [0, REMIX_MAX_LEN]
    REMIX_TERM_OFFSET,       // |terms[index].at| > REMIX_MAX_LEN
    REMIX_TERM_SOURCE,       // terms[index].src is null with len > 0
};
struct RemixVerdict { int why; int64_t index; };      // index: the row or term at fault, -1 where none is

inline bool remix_stride_ok(int64_t stride, int64_t width, int32_t R)
{
    return stride >= width && stride <= REMIX_MAX_LEN && (R <= 1 || stride <= REMIX_MAX_EXTENT / (R - 1));
}

// Everything bsrnn_remix_ragged refuses about its tables and sizes (the output pointers are the entry point's), in the order it says so
inline RemixVerdict remix_check(const RemixRow* rows, int32_t R, const RemixTerm* terms, int32_t n_terms, int64_t mix_stride,
                                int64_t target_stride, int64_t width)
{
    if (!rows || !terms) return {REMIX_NULL_TABLE, -1};
    if (R < 1 || n_terms < 1) return {REMIX_BAD_COUNT, -1};
    if (width < 0 || width > REMIX_MAX_LEN) return {REMIX_BAD_WIDTH, -1};
    if (!remix_stride_ok(mix_stride, width, R)) return {REMIX_MIX_STRIDE, -1};
    if (!remix_stride_ok(target_stride, width, R)) return {REMIX_TARGET_STRIDE, -1};
    for (int32_t r = 0; r < R; ++r) {
        if (rows[r].n < 0 || rows[r].n > width) return {REMIX_ROW_LENGTH, r};
        if (rows[r].n_terms < 1 || rows[r].first_term < 0 || rows[r].first_term > n_terms - rows[r].n_terms) return {REMIX_ROW_TERMS, r};
    }
    for (int32_t t = 0; t < n_terms; ++t) {
        if (terms[t].len < 0 || terms[t].len > REMIX_MAX_LEN) return {REMIX_TERM_LENGTH, t};
        if (terms[t].at < -REMIX_MAX_LEN || terms[t].at > REMIX_MAX_LEN) return {REMIX_TERM_OFFSET, t};
        if (!terms[t].src && terms[t].len > 0) return {REMIX_TERM_SOURCE, t};
    }
    return {REMIX_OK, -1};
}

// Workgroups per row (grid.x): the tiles of [0, width), the same for every row; at most 2^29
inline int64_t remix_tiles(int64_t width) { return (width + REMIX_TILE - 1) / REMIX_TILE; }

// Source samples of a term a row of n samples reads: |[0, n) intersected with [at, at + len)|
inline int64_t remix_term_reads(int64_t n, int64_t at, int64_t len)
{
    const int64_t lo = at > 0 ? at : 0, hi = at + len < n ? at + len : n;
    return hi > lo ? hi - lo : 0;
}

// The traffic model of a valid call: 4 bytes per source sample read, 8 * width bytes written per row (both outputs, zeros included)
struct RemixTraffic { int64_t read, written; };
inline RemixTraffic remix_traffic(const RemixRow* rows, int32_t R, const RemixTerm* terms, int64_t width)
{
    RemixTraffic q{0, 0};
    for (int32_t r = 0; r < R; ++r) {
        for (int32_t t = rows[r].first_term; t < rows[r].first_term + rows[r].n_terms; ++t)
            q.read += 4 * remix_term_reads(rows[r].n, terms[t].at, terms[t].len);
        q.written += 8 * width;
    }
    return q;
}

}  // namespace bsrnn
