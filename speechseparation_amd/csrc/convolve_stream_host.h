// The streaming (hop-by-hop) form of the long FIR convolution (bsrnn_fir_stream_*): what a row has been handed, which blocks a call forms,
// what a flush still owes, as integer arithmetic on the host.  HIP-free: api_resample.hip plans a call with it, fft.hip reads FirStreamRow
// from a table on the device, tests/cpp/convolve_stream_check.cpp compiles it alone.
//
// THE SCHEME is the one-shot's (convolve_host.h), walked in stream order.  A row that has taken N samples has the frames v < N / B complete
// (frame v = x[(v - 1) B, (v + 1) B), zeros in front of the stream); the spectrum of frame v lies in slot v mod P of the row's ring, and
// block u of x * g = sum_{p <= min(P - 1, u)} H[p] X[u - p], p ascending, is formed as soon as frame u is there and stored at u B - shift.
// Blocks are walked in order, so slot v mod P is written again (by frame v + P) only after its last reader (block v + P - 1): a ring of
// exactly P slots.  shift = k / 2 (FIR_ALIGN_SAME: the concatenated output is bsrnn_convolve_ragged's, bit for bit) or 0
// (FIR_ALIGN_CAUSAL: y[m] = (x * g)[m], no output sample depends on a later input sample).  Blocks below shift / B store nothing and are
// not formed; their frames are still analysed.
// A FLUSH knows the final length n = N: blocks up to u1 = (n - 1 + shift) / B are owed, frames up to f1 = min(u1, (n + B - 2) / B) are
// analysed with zeros behind the row's end, frames behind f1 are neither analysed nor read (the one-shot's rule, conv_plan).  A block formed
// before the flush reads frames <= u < N / B <= f1 only, so nothing formed earlier would have to be revised.
// BULK FEEDING (many blocks of few rows per call) is correct and slow: one workgroup walks a row's blocks one after the other.  The
// one-shot remains the fast path for whole rows; the stream's hot case is a tick - many rows, one block each.
#pragma once
#include "convolve_host.h"

namespace bsrnn {

constexpr int FIR_ALIGN_SAME = 0;                         // BSRNN_FIR_SAME
constexpr int FIR_ALIGN_CAUSAL = 1;                       // BSRNN_FIR_CAUSAL
constexpr int64_t FIR_STREAM_COUNT_MAX = (int64_t)1 << 30;      // samples into or out of one row in one call
constexpr int64_t FIR_STREAM_NO_CAP = INT64_MAX / 4;      // a process call's frame cap and store end: none
constexpr int FIR_STREAM_ROW_FLOATS = 2 * CONV_B;         // per row beside the ring: the previous 1024 inputs and a FIFO of < 1024

inline int64_t fir_stream_shift(int k, int align) { return align == FIR_ALIGN_CAUSAL ? 0 : conv_shift(k); }
// samples a row that took N has been handed
inline int64_t fir_stream_emitted(int64_t N, int64_t shift)
{
    const int64_t e = N / CONV_B * CONV_B - shift;
    return e > 0 ? e : 0;
}
// what the next process call hands a row at N that gives it n_in samples
inline int64_t fir_stream_ready(int64_t N, int64_t n_in, int64_t shift) { return fir_stream_emitted(N + n_in, shift) - fir_stream_emitted(N, shift); }
// the frames that call completes = the blocks it walks: [first, first + count)
struct FirStreamBlocks { int64_t first, count; };
inline FirStreamBlocks fir_stream_blocks(int64_t N, int64_t n_in) { return {N / CONV_B, (N + n_in) / CONV_B - N / CONV_B}; }
inline int fir_stream_slot(int64_t frame, int P) { return (int)(frame % P); }
// floats of the ring of C rows under filters of up to max_taps taps
inline int64_t fir_stream_ring_floats(int C, int max_taps) { return (int64_t)C * conv_partitions(max_taps) * CONV_LD; }

// The flush of a row at N under k taps: it walks [first, first + count) = [N / B, u1] (count 0: nothing is owed), analyses those of
// them that are <= f1, forms those that are >= u0, and hands out n_out = N - emitted(N) samples; the last block stores [m0, m1).
struct FirFlushPlan { int64_t shift, u0, u1, f1, first, count, n_out, m0, m1; };
inline FirFlushPlan fir_stream_flush_plan(int64_t N, int k, int align)
{
    FirFlushPlan f{};
    f.shift = fir_stream_shift(k, align);
    f.u0 = f.shift / CONV_B;
    f.first = N / CONV_B;
    if (N < 1) { f.u1 = f.f1 = -1; return f; }
    f.u1 = (N - 1 + f.shift) / CONV_B;
    const int64_t last = (N + CONV_B - 2) / CONV_B;
    f.f1 = f.u1 < last ? f.u1 : last;
    f.count = f.u1 >= f.first ? f.u1 - f.first + 1 : 0;
    f.n_out = N - fir_stream_emitted(N, f.shift);
    const int64_t a = f.u1 * CONV_B - f.shift, b = a + CONV_B;
    f.m0 = a > 0 ? a : 0;
    f.m1 = b < N ? b : N;
    return f;
}

// What the kernel knows of a row in one call, by index in a table on the device.  ub == ue and n_in == 0: the row is held.  H = null: a
// bypass row, n_in samples are copied.  Output sample m of the stream goes to the row's out[m - E0], m in [max(0, .), n_end).
struct FirStreamRow {
    const float* H;          // the filter's image [P][CONV_LD]
    int64_t N0;              // samples taken before the call
    int64_t E0;              // samples handed out before the call
    int64_t shift;
    int64_t n_end;           // flush: the final length; process: FIR_STREAM_NO_CAP
    int64_t ub, ue;          // frames / blocks [ub, ue) are walked
    int64_t u0;              // blocks below are not formed
    int64_t f1;              // frames behind are neither analysed nor read (flush; process: FIR_STREAM_NO_CAP)
    int32_t n_in;            // samples the row reads from the call's input
    int32_t P;
    int32_t keep;            // 1: the previous-1024 tail and the FIFO are brought up to N0 + n_in (process); 0: flush
    int32_t pad_;
};
inline FirStreamRow fir_stream_row_held() { return FirStreamRow{}; }
inline FirStreamRow fir_stream_row_process(const float* H, int k, int align, int64_t N, int64_t n_in)
{
    FirStreamRow q{};
    q.H = H; q.N0 = N; q.shift = fir_stream_shift(k, align); q.E0 = fir_stream_emitted(N, q.shift);
    q.n_end = q.f1 = FIR_STREAM_NO_CAP;
    const FirStreamBlocks b = fir_stream_blocks(N, n_in);
    q.ub = b.first; q.ue = b.first + b.count; q.u0 = q.shift / CONV_B;
    q.n_in = (int32_t)n_in; q.P = conv_partitions(k); q.keep = 1;
    return q;
}
inline FirStreamRow fir_stream_row_flush(const float* H, int k, int align, int64_t N)
{
    const FirFlushPlan f = fir_stream_flush_plan(N, k, align);
    FirStreamRow q{};
    if (f.count == 0) return q;
    q.H = H; q.N0 = N; q.shift = f.shift; q.E0 = fir_stream_emitted(N, f.shift);
    q.n_end = N; q.f1 = f.f1;
    q.ub = f.first; q.ue = f.first + f.count; q.u0 = f.u0;
    q.n_in = 0; q.P = conv_partitions(k); q.keep = 0;
    return q;
}

}  // namespace bsrnn
