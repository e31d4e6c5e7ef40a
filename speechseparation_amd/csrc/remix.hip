// The re-mix of an optimizer step on the device (bsrnn_remix_ragged; remix_host.h holds the definition and the checks): mixtures and
// targets of all rows in ONE launch, written straight into the padded [rows][width] buffers the ragged training step takes.
//
// A workgroup owns REMIX_TILE consecutive outputs of one row, a lane REMIX_PER_LANE of them REMIX_THREADS samples apart: every load
// and store of a wave is 64 consecutive floats (256 bytes).  A term's source offset i - at is arbitrary - the reference draws it with
// randint - so three terms in four start off a 16-byte boundary relative to the stores; with dword accesses side by side across the
// lanes there is ONE path for every (pointer, at, stride), and nothing to keep identical between two.  Pure streaming: each source
// sample is read once, each output written once.
// The eight loads of a term are issued together and waited for once: they are UNCONDITIONAL, from the source index clamped into
// [0, len) - a lane outside the term re-reads the source's first or last sample and discards it - because a load under a lane mask is
// compiled into a branch of its own with its own wait (eight round trips per term instead of one).  A term that meets the tile's
// samples of [0, n) nowhere is skipped by the whole workgroup, which is also what keeps a null source of no samples unread; skipping
// changes no bit: a skipped term's values are all +0, and the running sum is never -0 (it starts at +0, and a rounded sum is -0 only
// when both addends are), so sum + +0 == sum.
// The arithmetic is spelled out per sample - one multiply, then the additions in term order, contraction off - so the bits are those
// of torch's `x * gain` and `dialog + sum(backgrounds)`.  The row and term tables are read at wave-uniform addresses.
#include "kernels.h"

namespace bsrnn {

namespace {

// v_t(i) for the lane's REMIX_PER_LANE outputs i0 + k * REMIX_THREADS of the tile starting at t0; false: the term is +0 on the whole tile
__device__ __forceinline__ bool remix_values(const RemixTerm& q, int64_t t0, int64_t i0, int64_t n, float (&v)[REMIX_PER_LANE])
{
#pragma clang fp contract(off)
    const int64_t lo = q.at > 0 ? q.at : 0, hi = q.at + q.len < n ? q.at + q.len : n;       // the term's samples of the row: [lo, hi)
    if (hi <= lo || hi <= t0 || lo >= t0 + REMIX_TILE) return false;                         // workgroup-uniform
    float x[REMIX_PER_LANE];
#pragma unroll
    for (int k = 0; k < REMIX_PER_LANE; ++k) {
        const int64_t j = i0 + k * REMIX_THREADS - q.at;
        x[k] = q.src[j < 0 ? 0 : (j < q.len ? j : q.len - 1)];
    }
#pragma unroll
    for (int k = 0; k < REMIX_PER_LANE; ++k) {
        const int64_t i = i0 + k * REMIX_THREADS;
        const float p = x[k] * q.gain;
        v[k] = (i >= lo && i < hi) ? p : 0.0f;
    }
    return true;
}

}  // namespace

// grid (tiles of a row, rows); rows [R] and terms on the device; mix / target rows mix_stride / target_stride floats apart
__global__ __launch_bounds__(REMIX_THREADS) void remix_ragged_kernel(const RemixRow* __restrict__ rows, const RemixTerm* __restrict__ terms, int R,
                                                                     float* __restrict__ mix, int64_t mix_stride, float* __restrict__ target,
                                                                     int64_t target_stride, int64_t width)
{
#pragma clang fp contract(off)
    const int64_t t0 = (int64_t)blockIdx.x * REMIX_TILE, i0 = t0 + threadIdx.x;
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        const RemixRow row = rows[r];
        const RemixTerm* own = terms + row.first_term;
        float v0[REMIX_PER_LANE], acc[REMIX_PER_LANE], v[REMIX_PER_LANE];
#pragma unroll
        for (int k = 0; k < REMIX_PER_LANE; ++k) v0[k] = acc[k] = 0.0f;
        remix_values(own[0], t0, i0, row.n, v0);               // the target
        for (int b = 1; b < row.n_terms; ++b) {                // the backgrounds, in order: sum() starts from 0
            if (!remix_values(own[b], t0, i0, row.n, v)) continue;
#pragma unroll
            for (int k = 0; k < REMIX_PER_LANE; ++k) acc[k] = acc[k] + v[k];
        }
        float* m = mix + (int64_t)r * mix_stride;
        float* t = target + (int64_t)r * target_stride;
#pragma unroll
        for (int k = 0; k < REMIX_PER_LANE; ++k) {
            const int64_t i = i0 + k * REMIX_THREADS;
            if (i < width) { m[i] = v0[k] + acc[k]; t[i] = v0[k]; }      // [n, width): +0 + +0
        }
    }
}

void launch_remix_ragged(const RemixRow* rows, const RemixTerm* terms, int R, float* mix, int64_t mix_stride, float* target, int64_t target_stride,
                         int64_t width, hipStream_t s)
{
    const int64_t tiles = remix_tiles(width);
    if (tiles < 1) return;
    hipLaunchKernelGGL(remix_ragged_kernel, dim3((unsigned)tiles, R < 65535 ? R : 65535), dim3(REMIX_THREADS), 0, s, rows, terms, R, mix, mix_stride,
                       target, target_stride, width);
}

}  // namespace bsrnn
