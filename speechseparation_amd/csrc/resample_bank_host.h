// A bank of streaming resamplers (bsrnn_resampler_bank_*): C rows, each on one of up to BANK_PAIRS_MAX declared rate pairs and at its own
// place in its own stream, converted by ONE launch.  A row of the bank follows exactly the arithmetic of a single-pair bsrnn_resampler
// of its pair (resample_host.h: resample_ready, resample_n_out, resample_base, the keep-from rule, resample_carry_floats); this header
// only turns "row r takes n_in samples now" or "row r is flushed" into what the kernel has to know about that row, and into the row's next
// position.  Host-only arithmetic, no HIP types: api_resample.hip builds the descriptors, resample.hip reads them,
// tests/cpp/resample_bank_check.cpp checks both with g++.
//
// The descriptors travel BY VALUE in the kernel arguments, as RowSet and RowHops do (stream_rows_host.h): no allocation, no staging
// copy, nothing that has to outlive the call.  That makes their size the number of rows one launch takes, so a descriptor holds nothing
// the kernel can do without.
// WHAT IS 64-BIT AND WHAT IS NOT.  A row's position - N inputs taken, J outputs given - is 64-bit and stays on the host (BankPos).  The
// kernel never needs it: every input index it forms is a DIFFERENCE from the row's carry origin o = max(0, floor(J * down / up) - Kh), the
// stream index of the first sample the carry holds, and those differences are bounded by the carry's size plus the call's block; what
// it needs of J itself are two residues below up <= 1024.  With o as the origin of the kernel's input axis the rules of ResampleArgs
// hold unchanged: the carry is [0, n_carry), the block [n_carry, n_carry + n_in), zeros elsewhere - the zeros in front of the stream
// included, because o = 0 exactly while the stream's beginning is still inside the filter's reach.  So NO field of the descriptor is
// 64-bit: five 32-bit words.  The price is a limit on one call's block, BANK_BLOCK_MAX samples in and out per row, so that
// n_carry + n_in and the count fit 31 bits (the kernel still forms tile * down products of a call in 64 bits); a position near 2^40 is
// no different from one near 0.
#pragma once
#include "resample_host.h"

namespace bsrnn {

constexpr int BANK_PAIRS_MAX = 16;                       // BSRNN_BANK_PAIRS_MAX of include/bsrnn_hip.h: a pair index fits 4 bits
constexpr int64_t BANK_BLOCK_MAX = (int64_t)1 << 30;     // samples one call takes from a row, and gives to it

// Where a row stands: N inputs taken, J outputs given, its pair, and which of the two carry sets holds inputs [keep_from(J), N).
struct BankPos { int64_t N = 0, J = 0; int32_t pair = 0, cur = 0; };

// What the kernel knows of one row in one call.  Input indices count from the carry origin (above).
//   n_in   samples of the caller's block (0 in a flush)
//   n_j    outputs written, out[r][0 .. n_j)
//   keep   the next carry starts at input index keep: the launch copies [keep, n_carry + n_in) to the other set
//   w3     bits 0-15 n_carry, the samples the current carry holds (<= resample_carry_floats <= 21506);
//          bits 16-31 lead = floor(J * down / up) - origin, at most Kh <= 10240: where output J's phase-0 tap sits
//   w4     bits 0-9 (J * down) mod up, bits 10-19 J mod up (both < up <= 1024), bits 20-23 the pair, bit 24 the current carry set,
//          bit 25 the row runs in this call (clear: held, nothing is read or written for it), bit 26 the row writes a carry (a process
//          call; clear in a flush, which leaves the row reset)
struct BankRow { uint32_t n_in, n_j, keep, w3, w4; };

constexpr uint32_t BANK_ROW_RUNS = 1u << 25, BANK_ROW_CARRIES = 1u << 26;
BSRNN_RS_HD constexpr int bank_row_n_carry(const BankRow& d) { return (int)(d.w3 & 0xffffu); }
BSRNN_RS_HD constexpr int bank_row_lead(const BankRow& d) { return (int)(d.w3 >> 16); }
BSRNN_RS_HD constexpr unsigned bank_row_phase(const BankRow& d) { return d.w4 & 0x3ffu; }
BSRNN_RS_HD constexpr unsigned bank_row_column(const BankRow& d) { return (d.w4 >> 10) & 0x3ffu; }
BSRNN_RS_HD constexpr int bank_row_pair(const BankRow& d) { return (int)((d.w4 >> 20) & 0xfu); }
BSRNN_RS_HD constexpr int bank_row_cur(const BankRow& d) { return (int)((d.w4 >> 24) & 1u); }

// Rows per launch.  A dispatch has 4096 bytes of kernel-argument space; 256 of them are the arguments the compiler appends (grid
// sizes and the like), and 256 more are kept for the kernel's other arguments (BankLaunch, kernels.h: 88 bytes today).  The rest
// holds BankRow descriptors: 3584 / 20 = 179 rows, so a 64-row pool is one launch and the widest stream (2048 rows) twelve.
constexpr int BANK_ARG_SPACE = 4096, BANK_ARG_IMPLICIT = 256, BANK_ARG_OTHER = 256;
constexpr int BANK_GROUP_ROWS = (BANK_ARG_SPACE - BANK_ARG_IMPLICIT - BANK_ARG_OTHER) / (int)sizeof(BankRow);
struct BankRows { BankRow r[BANK_GROUP_ROWS]; };
static_assert(sizeof(BankRow) == 20, "five 32-bit words");
static_assert(sizeof(BankRows) + BANK_ARG_IMPLICIT + BANK_ARG_OTHER <= BANK_ARG_SPACE, "a group of descriptors fits the kernel-argument space");

// The keep-from rule: the first input that output J, the next one owed, still reads - the carry's origin.
inline int64_t bank_keep_from(const ResampleRatio& q, int64_t J)
{
    const int64_t b = resample_base(J, q.up, q.down, q.Kh);
    return b > 0 ? b : 0;
}

// The count a process of n_in more samples would give the row (bsrnn_resampler_ready's rule); n_in >= 0.
inline int64_t bank_row_ready(const ResampleRatio& q, const BankPos& p, int64_t n_in)
{
    return resample_ready(p.N + n_in, q.up, q.down, q.half) - p.J;
}
// What a flush owes the row: up to the final length of the N samples taken
inline int64_t bank_row_owed(const ResampleRatio& q, const BankPos& p) { return resample_n_out(p.N, q.up, q.down) - p.J; }

// A row starts a new stream, on the pair it has or on another one.  Host-only, as bsrnn_resampler_reset: with no input taken the
// carry holds no sample a call would read, whichever set is current.
inline void bank_row_reset(BankPos& p) { p.N = p.J = 0; }
inline void bank_row_assign(BankPos& p, int pair) { p.N = p.J = 0; p.pair = pair; }

enum BankWhy { BANK_OK = 0, BANK_BAD_COUNT, BANK_BLOCK_TOO_LONG, BANK_CARRY_OVERFLOW };

// A row that is not part of the call: nothing of it is read or written, its position and carry set stay.
inline BankRow bank_row_hold(const BankPos& p)
{
    return BankRow{0, 0, 0, 0, ((uint32_t)p.pair << 20) | ((uint32_t)p.cur << 24)};
}

namespace bank_detail {
inline BankRow describe(const ResampleRatio& q, const BankPos& p, int64_t n_in, int64_t J1, uint32_t flags)
{
    const int64_t c = p.J * q.down, origin = bank_keep_from(q, p.J);
    BankRow d;
    d.n_in = (uint32_t)n_in;
    d.n_j = (uint32_t)(J1 - p.J);
    d.keep = (uint32_t)(bank_keep_from(q, J1) - origin);
    d.w3 = (uint32_t)(p.N - origin) | ((uint32_t)(c / q.up - origin) << 16);
    d.w4 = (uint32_t)(c % q.up) | ((uint32_t)(p.J % q.up) << 10) | ((uint32_t)p.pair << 20) | ((uint32_t)p.cur << 24) | flags;
    return d;
}
}  // namespace bank_detail

// Row at p (on pair q) takes n_in samples now -> its descriptor and its next position.  n_in == 0 holds the row (BANK_OK, next == p).
// BANK_BAD_COUNT: n_in < 0 or beyond what a 64-bit position can still take; BANK_BLOCK_TOO_LONG: n_in or the count beyond
// BANK_BLOCK_MAX; BANK_CARRY_OVERFLOW: the next carry would not fit resample_carry_floats (cannot happen: resample_check.cpp).
inline int bank_row_process(const ResampleRatio& q, const BankPos& p, int64_t n_in, BankRow& d, BankPos& next)
{
    d = bank_row_hold(p);
    next = p;
    if (n_in < 0 || n_in > (INT64_MAX >> 12) - p.N) return BANK_BAD_COUNT;
    if (n_in == 0) return BANK_OK;
    if (n_in > BANK_BLOCK_MAX) return BANK_BLOCK_TOO_LONG;
    const int64_t N1 = p.N + n_in, J1 = resample_ready(N1, q.up, q.down, q.half);
    if (J1 - p.J > BANK_BLOCK_MAX) return BANK_BLOCK_TOO_LONG;
    if (N1 - bank_keep_from(q, J1) > resample_carry_floats(q)) return BANK_CARRY_OVERFLOW;
    d = bank_detail::describe(q, p, n_in, J1, BANK_ROW_RUNS | BANK_ROW_CARRIES);
    next.N = N1; next.J = J1; next.cur = p.cur ^ 1;
    return BANK_OK;
}

// Row at p is flushed: it gets what it is still owed, the future counting as zeros, and is left at the stream's beginning (its pair
// stays).  A row that is owed nothing is held by the kernel; its position is reset all the same.
inline int bank_row_flush(const ResampleRatio& q, const BankPos& p, BankRow& d, BankPos& next)
{
    d = bank_row_hold(p);
    next = p;
    next.N = next.J = 0;
    const int64_t owed = bank_row_owed(q, p);
    if (owed > BANK_BLOCK_MAX) return BANK_BLOCK_TOO_LONG;
    if (owed > 0) d = bank_detail::describe(q, p, 0, p.J + owed, BANK_ROW_RUNS);
    return BANK_OK;
}

}  // namespace bsrnn
