// Sample-rate conversion on the device: scipy.signal.resample_poly's polyphase FIR (resample_host.h holds the definition and every
// index rule).  One kernel for bsrnn_resample and for the streaming resampler: they differ only in where an input sample lives (the
// caller's buffer, or the resampler's carry in front of it), never in how an output sample is formed - resample_mac below, the same
// taps in the same order - which is what makes the concatenated streaming output equal the one-shot call bit for bit.
//
// A workgroup owns `tile` consecutive outputs of one row.  Their inputs are one contiguous span (tile * down / up + L samples), staged
// in LDS once and read L times.  The taps come through L1 / L2 from the table laid out BY OUTPUT, [ld][up] with column j mod up
// (resample_table_by_output): for each t the lanes of a wave read consecutive floats.  With the table as [up][ld] - a row per phase,
// 16-byte loads - every lane of a load read another row, 64 cache lines per instruction, and the kernel ran at the vector memory
// pipeline's one line per clock, 7 to 15 times a copy of the same bytes; the whole table is 13 KB at 48 k -> 44.1 k, 52 KB at the largest audio pair,
// and every workgroup of the launch reads the same one (measurements: DESIGN.md section 4n).  fp32 accumulation in four partial sums
// (t mod 4), added pairwise at the end.
#include "kernels.h"
#include "resample_host.h"
#include "resample_bank_host.h"

namespace bsrnn {

namespace {

struct RsAcc { float a, b, c, d; };

// One output sample's share of n taps (n % 4 == 0): x[0 .. n) from LDS against taps[0], taps[up], .. (its column of the table)
__device__ __forceinline__ void resample_mac(const float* __restrict__ x, const float* __restrict__ taps, unsigned up, int n, RsAcc& s)
{
    for (int t = 0; t < n; t += 4) {
        const float h0 = taps[0], h1 = taps[up], h2 = taps[2 * up], h3 = taps[3 * up];
        taps += 4 * up;
        s.a = __builtin_fmaf(x[t], h0, s.a);
        s.b = __builtin_fmaf(x[t + 1], h1, s.b);
        s.c = __builtin_fmaf(x[t + 2], h2, s.c);
        s.d = __builtin_fmaf(x[t + 3], h3, s.d);
    }
}

// Input sample i of the row whose segments start at ra / rb: zero outside [a0, n_total)
__device__ __forceinline__ float resample_input(const ResampleArgs& g, const float* ra, const float* rb, int64_t i)
{
    if (i < g.a0 || i >= g.n_total) return 0.0f;
    return i < g.a1 ? ra[i - g.a0] : rb[i - g.a1];
}

// The extra workgroup of a bank call's row: inputs [c0, n_total) of the row, what the next call still needs, to dst
__device__ __forceinline__ void resample_carry(const ResampleArgs& g, const float* ra, const float* rb, float* dst, int tid)
{
    const int n = (int)(g.n_total - g.c0);
    for (int k = tid; k < n; k += 256) dst[k] = resample_input(g, ra, rb, g.c0 + k);
}

// One tile: nj <= g.tile consecutive outputs of the row to dst[0 .. nj).  Where the tile's first output jt sits comes decomposed -
// jt * down = q0 * up + r0, jm0 = jt mod up - so that q0 may count from any origin the input axis of g (a0, a1, n_total) counts from:
// here the row's carry.  From there on 32 bits do (tile, down, up <= 1024).  This is resample_kernel's tile below as a function, for
// resample_bank_kernel alone: with resample_kernel calling it too that kernel came out of the compiler with another register
// allocation and schedule (1796 instructions for 1782), and it has to stay the kernel that was measured.
__device__ __forceinline__ void resample_tile(const ResampleArgs& g, const int vec, const float* ra, const float* rb, float* dst, float* xs,
                                              const int64_t q0, const unsigned r0, const unsigned jm0, const int nj, const int tid)
{
    const unsigned up = (unsigned)g.up, down = (unsigned)g.down;
    unsigned off[4], col[4];            // per output: where its inputs start in the span, its column of the table (j mod up)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        off[k] = (r0 + (unsigned)(tid + 256 * k) * down) / up;
        col[k] = (jm0 + (unsigned)(tid + 256 * k)) % up;
    }
    const int reach = (int)((r0 + (unsigned)(nj - 1) * down) / up);      // off of the tile's last output
    RsAcc acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = RsAcc{0.0f, 0.0f, 0.0f, 0.0f};

    for (int t0 = 0; t0 < g.ld; t0 += g.chunk) {
        const int nt = g.ld - t0 < g.chunk ? g.ld - t0 : g.chunk;
        const int len = reach + nt;                                      // <= RESAMPLE_SPAN (resample_tiling)
        const int64_t s0 = q0 - g.Kh + t0;                               // the input index of xs[0]
        if (vec) {
            // 16-byte loads of the aligned groups of four of segment b that lie wholly inside it and inside the span; the groups at
            // the edges, the carry and the zeros sample by sample.  (vec: every row of b starts 16-byte aligned.)
            const int64_t eb = s0 - g.a1, nb = g.n_total - g.a1;         // xs[0] is b[eb]
            const int64_t e_first = eb - (((eb % 4) + 4) % 4);
            const int groups = (int)((eb + len - e_first + 3) / 4);
            for (int u = tid; u < groups; u += 256) {
                const int64_t e4 = e_first + 4 * (int64_t)u;
                const int k = (int)(e4 - eb);
                if (e4 >= 0 && e4 + 3 < nb && k >= 0 && k + 3 < len) {
                    const float4 v = *reinterpret_cast<const float4*>(rb + e4);
                    xs[k] = v.x; xs[k + 1] = v.y; xs[k + 2] = v.z; xs[k + 3] = v.w;
                } else {
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (k + m >= 0 && k + m < len) xs[k + m] = resample_input(g, ra, rb, s0 + k + m);
                }
            }
        } else {
            for (int k = tid; k < len; k += 256) xs[k] = resample_input(g, ra, rb, s0 + k);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + 256 * k < nj) resample_mac(xs + off[k], g.tab + (size_t)t0 * up + col[k], up, nt, acc[k]);
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (tid + 256 * k < nj) dst[tid + 256 * k] = (acc[k].a + acc[k].b) + (acc[k].c + acc[k].d);
}

}  // namespace

// grid (n_tiles [+ 1 when a carry is written], R)
__global__ __launch_bounds__(256) void resample_kernel(const ResampleArgs g, const int vec)
{
    __shared__ float xs[RESAMPLE_SPAN];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.y;
    const float* ra = g.a + r * g.a_stride;
    const float* rb = g.b + r * g.b_stride;
    if ((int)blockIdx.x == g.n_tiles) {            // the extra workgroup of a streaming call: what the next call still needs
        float* dst = g.carry + r * g.carry_stride;
        const int n = (int)(g.n_total - g.c0);
        for (int k = tid; k < n; k += 256) dst[k] = resample_input(g, ra, rb, g.c0 + k);
        return;
    }
    const int64_t jt = g.j0 + (int64_t)blockIdx.x * g.tile;
    const int64_t left = g.j0 + g.n_j - jt;
    const int nj = left < g.tile ? (int)left : g.tile;
    // j * down = q0 * up + r0 for the tile's first output; from there on 32 bits do (tile, down, up <= 1024)
    const int64_t c = jt * g.down;
    const int64_t q0 = c / g.up;
    const unsigned r0 = (unsigned)(c - q0 * g.up), up = (unsigned)g.up, down = (unsigned)g.down;
    const unsigned jm0 = (unsigned)(jt % g.up);
    unsigned off[4], col[4];            // per output: where its inputs start in the span, its column of the table (j mod up)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        off[k] = (r0 + (unsigned)(tid + 256 * k) * down) / up;
        col[k] = (jm0 + (unsigned)(tid + 256 * k)) % up;
    }
    const int reach = (int)((r0 + (unsigned)(nj - 1) * down) / up);      // off of the tile's last output
    RsAcc acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = RsAcc{0.0f, 0.0f, 0.0f, 0.0f};

    for (int t0 = 0; t0 < g.ld; t0 += g.chunk) {
        const int nt = g.ld - t0 < g.chunk ? g.ld - t0 : g.chunk;
        const int len = reach + nt;                                      // <= RESAMPLE_SPAN (resample_tiling)
        const int64_t s0 = q0 - g.Kh + t0;                               // the input index of xs[0]
        if (vec) {
            // 16-byte loads of the aligned groups of four of segment b that lie wholly inside it and inside the span; the groups at
            // the edges, the carry and the zeros sample by sample.  (vec: every row of b starts 16-byte aligned.)
            const int64_t eb = s0 - g.a1, nb = g.n_total - g.a1;         // xs[0] is b[eb]
            const int64_t e_first = eb - (((eb % 4) + 4) % 4);
            const int groups = (int)((eb + len - e_first + 3) / 4);
            for (int u = tid; u < groups; u += 256) {
                const int64_t e4 = e_first + 4 * (int64_t)u;
                const int k = (int)(e4 - eb);
                if (e4 >= 0 && e4 + 3 < nb && k >= 0 && k + 3 < len) {
                    const float4 v = *reinterpret_cast<const float4*>(rb + e4);
                    xs[k] = v.x; xs[k + 1] = v.y; xs[k + 2] = v.z; xs[k + 3] = v.w;
                } else {
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (k + m >= 0 && k + m < len) xs[k + m] = resample_input(g, ra, rb, s0 + k + m);
                }
            }
        } else {
            for (int k = tid; k < len; k += 256) xs[k] = resample_input(g, ra, rb, s0 + k);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + 256 * k < nj) resample_mac(xs + off[k], g.tab + (size_t)t0 * up + col[k], up, nt, acc[k]);
        __syncthreads();
    }
    float* dst = g.out + r * g.out_stride + (jt - g.j0);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (tid + 256 * k < nj) dst[tid + 256 * k] = (acc[k].a + acc[k].b) + (acc[k].c + acc[k].d);
}

// A bank call: rows that differ in pair, block length and stream position, one workgroup per tile of one row.  grid (the most tiles
// a row of the group has + 1, rows of the group).  The row's descriptor is read with blockIdx.y alone - scalar loads from the
// kernel-argument segment - and so is its pair's entry of the table in device memory.  The row's input axis counts from its carry
// origin (resample_bank_host.h), which is all that differs from resample_kernel: resample_tile is that kernel's tile, statement for
// statement, and forms every output from the same taps in the same order (resample_mac).
// The pointer form (L.in_rows / L.out_rows, kernels.h): a row's block, or its output, is where its entry of a table in device memory says.
// The entry is read behind the BANK_ROW_RUNS test, so a held row never reads a stale pointer; 16-byte loads are then the row's own
// choice (its base aligned to 16 bytes), uniform for the workgroup and made before any barrier.
__global__ __launch_bounds__(256) void resample_bank_kernel(const BankLaunch L, const BankRows rows)
{
    __shared__ float xs[RESAMPLE_SPAN];
    const BankRow d = rows.r[blockIdx.y];
    if (!(d.w4 & BANK_ROW_RUNS)) return;                                  // held: the row keeps its carry set, nothing is copied
    const BankPair p = L.pairs[bank_row_pair(d)];
    const int n_tiles = (int)((d.n_j + (unsigned)p.tile - 1) / (unsigned)p.tile);
    const int bx = (int)blockIdx.x;
    if (bx > n_tiles || (bx == n_tiles && !(d.w4 & BANK_ROW_CARRIES))) return;      // past the row's work, before any barrier
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.y;
    const int cur = bank_row_cur(d), n_carry = bank_row_n_carry(d);
    ResampleArgs g;
    g.a = L.carry + cur * L.carry_set + r * L.cap; g.a0 = 0; g.a1 = n_carry;
    // the pointer form: the row's block is wherever its entry of the table says (read by rows that run alone, with blockIdx.y: uniform)
    g.b = L.in_rows ? L.in_rows[r] : L.in + r * L.in_stride; g.n_total = (int64_t)n_carry + d.n_in;
    const int vec = L.in_rows ? (g.b != nullptr && (reinterpret_cast<uintptr_t>(g.b) & 15u) == 0) : L.vec;
    g.tab = p.tab; g.up = p.up; g.down = p.down; g.Kh = p.Kh; g.ld = p.ld; g.chunk = p.chunk; g.tile = p.tile;
    g.c0 = d.keep;
    if (bx == n_tiles) {
        resample_carry(g, g.a, g.b, L.carry + (cur ^ 1) * L.carry_set + r * L.cap, tid);
        return;
    }
    const int64_t jd = (int64_t)bx * p.tile;                              // outputs in front of the tile, of this call
    const int64_t left = (int64_t)d.n_j - jd;
    const int nj = left < p.tile ? (int)left : p.tile;
    const int64_t c = (int64_t)bank_row_phase(d) + jd * p.down;           // (J + jd) * down = (origin + lead) * up + c
    const int64_t qd = c / p.up;
    float* out = L.out_rows ? L.out_rows[r] : L.out + r * L.out_stride;
    resample_tile(g, vec, g.a, g.b, out + jd, xs, bank_row_lead(d) + qd, (unsigned)(c - qd * p.up),
                  (unsigned)((bank_row_column(d) + jd) % p.up), nj, tid);
}

void launch_resample(ResampleArgs g, int R, hipStream_t s)
{
    const int blocks = g.n_tiles + (g.carry ? 1 : 0);
    if (blocks < 1 || R < 1) return;
    // 16-byte loads where every row of the caller's block starts aligned, as launch_metric_time_ragged decides: the base and the stride
    const int vec = g.b && ((uintptr_t)g.b & 15) == 0 && g.b_stride % 4 == 0;
    for (int r = 0; r < R; r += 65535) {             // (rows are the grid's y: 65535 per launch)
        const int rows = R - r < 65535 ? R - r : 65535;
        hipLaunchKernelGGL(resample_kernel, dim3(blocks, rows), dim3(256), 0, s, g, vec);
        if (g.a) g.a += rows * g.a_stride;
        if (g.b) g.b += rows * g.b_stride;
        if (g.carry) g.carry += rows * g.carry_stride;
        if (g.out) g.out += rows * g.out_stride;
    }
}

void launch_resample_bank(BankLaunch L, const int* tiles, const BankRow* rows, int C, hipStream_t s)
{
    L.vec = L.in && ((uintptr_t)L.in & 15) == 0 && L.in_stride % 4 == 0;      // as launch_resample decides: the base and the stride
    for (int r0 = 0; r0 < C; r0 += BANK_GROUP_ROWS) {                          // one launch per group of descriptors
        const int n = C - r0 < BANK_GROUP_ROWS ? C - r0 : BANK_GROUP_ROWS;
        BankRows group;
        unsigned blocks = 0;
        for (int i = 0; i < n; ++i) {
            const BankRow& d = group.r[i] = rows[r0 + i];
            if (!(d.w4 & BANK_ROW_RUNS)) continue;
            const unsigned tile = (unsigned)tiles[bank_row_pair(d)];
            const unsigned b = (d.n_j + tile - 1) / tile + 1;
            blocks = b > blocks ? b : blocks;
        }
        for (int i = n; i < BANK_GROUP_ROWS; ++i) group.r[i] = BankRow{0, 0, 0, 0, 0};
        if (blocks) {
            BankLaunch G = L;
            if (G.in) G.in += (int64_t)r0 * L.in_stride;
            if (G.out) G.out += (int64_t)r0 * L.out_stride;
            if (G.in_rows) G.in_rows += r0;
            if (G.out_rows) G.out_rows += r0;
            G.carry += (int64_t)r0 * L.cap;
            hipLaunchKernelGGL(resample_bank_kernel, dim3(blocks, n), dim3(256), 0, s, G, group);
        }
    }
}

}  // namespace bsrnn
