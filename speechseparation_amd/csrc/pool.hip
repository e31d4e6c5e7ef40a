// The two copy kernels of the native session pool (bsrnn_pool_feed; the plan and the table: pool_host.h).  Around ONE
// bsrnn_stream_process_hops per round, the gather launch packs every named session's audio - what waits in its FIFO, then its input -
// into the [C, L*1024] rectangle the hops call reads and stores what stays waiting; the scatter launch hands every session its hops of the
// [C, L*1024] result at the session's own pointer and stride (for a session with a sample rate of its own both are its rows of the pool's
// staging rectangles, and the hop of the stream's delay is not handed on: out_skip).  Under 1 MB per tick: both launches are
// launch-bound, so they are plain coalesced copies.  A workgroup owns one 1024-sample segment of one table entry (one row of one session), so every length test below
// is workgroup-uniform.  Session pointers and strides are the caller's: only 4-byte alignment is assumed, and a segment moves in
// 16-byte pieces only when its foreign side happens to be 16-byte aligned (the rectangles are: their rows are whole hops of an aligned
// allocation).
#include "kernels.h"
#include "pool_host.h"

namespace bsrnn {

namespace {

constexpr int POOL_THREADS = 256;
static_assert(POOL_HOP == 4 * POOL_THREADS, "a thread moves four floats of a segment");

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// 1024 floats src -> dst, one of them an aligned rectangle row (uniform choice per workgroup)
__device__ __forceinline__ void copy_segment(float* __restrict__ dst, const float* __restrict__ src, int tid)
{
    if (aligned16(dst) && aligned16(src)) {
        reinterpret_cast<float4*>(dst)[tid] = reinterpret_cast<const float4*>(src)[tid];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[tid + k * POOL_THREADS] = src[tid + k * POOL_THREADS];
    }
}

// grid (max(L, 1), entries).  chunk [C][L*1024], fifo [C][1024].
__global__ __launch_bounds__(POOL_THREADS) void pool_gather_kernel(const PoolEntry* __restrict__ tab, float* __restrict__ chunk,
                                                                   float* fifo, const int L)
{
    const PoolEntry e = tab[blockIdx.y];
    const int seg = blockIdx.x, tid = threadIdx.x;
    float* q = fifo + (size_t)e.row * POOL_HOP;
    if (seg < L) {
        float* d = chunk + ((size_t)e.row * L + seg) * POOL_HOP;
        const int j0 = seg * POOL_HOP, n_data = e.n_fifo + e.n_in;          // n_data = hops * 1024: a segment is all audio or all zeros
        if (j0 >= n_data) {
            reinterpret_cast<float4*>(d)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (seg == 0 && e.n_fifo > 0) {
            // the row's first segment of the session's first round: what waited, then the input (n_fifo < 1024 <= n_data)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = tid + k * POOL_THREADS;
                d[i] = i < e.n_fifo ? q[i] : e.src[i - e.n_fifo];
            }
        } else {
            copy_segment(d, e.src + (j0 - e.n_fifo), tid);
        }
    }
    // What stays waiting.  Its source is the input, never the FIFO (pool_host.h); the reads of the FIFO above belong to this same
    // workgroup and have been stored to the rectangle by the time the barrier lets anyone write.
    if (seg == 0 && e.n_pend > 0) {
        __syncthreads();
        for (int i = tid; i < e.n_pend; i += POOL_THREADS) q[e.pend_off + i] = e.pend_src[i];
    }
}

// grid (L, entries).  out [C][L*1024]; nothing behind an entry's n_out - out_skip samples is written.
__global__ __launch_bounds__(POOL_THREADS) void pool_scatter_kernel(const PoolEntry* __restrict__ tab, const float* __restrict__ out, const int L)
{
    const PoolEntry e = tab[blockIdx.y];
    const int seg = blockIdx.x, j0 = seg * POOL_HOP;
    if (j0 >= e.n_out || j0 < e.out_skip) return;            // (out_skip: the dropped first hop of a session with a rate; whole segments)
    copy_segment(e.dst + (j0 - e.out_skip), out + ((size_t)e.row * L + seg) * POOL_HOP, threadIdx.x);
}

}  // namespace

void launch_pool_gather(const PoolEntry* tab, int n_entries, float* chunk, float* fifo, int L, hipStream_t s)
{
    if (n_entries < 1) return;
    hipLaunchKernelGGL(pool_gather_kernel, dim3(L > 0 ? L : 1, n_entries), dim3(POOL_THREADS), 0, s, tab, chunk, fifo, L);
}

void launch_pool_scatter(const PoolEntry* tab, int n_entries, const float* out, int L, hipStream_t s)
{
    if (n_entries < 1 || L < 1) return;
    hipLaunchKernelGGL(pool_scatter_kernel, dim3(L, n_entries), dim3(POOL_THREADS), 0, s, tab, out, L);
}

}  // namespace bsrnn
