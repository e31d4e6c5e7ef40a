// The native session pool (bsrnn_pool_*): slots, the per-session count of samples that do not yet fill a hop, and the ROUND PLAN of one
// feed - what every row of every named session contributes to each bsrnn_stream_process_hops call of the feed, and what it leaves
// waiting.  Host-only arithmetic, no HIP types: api_pool.hip plans and fills the table, pool.hip reads it,
// tests/cpp/pool_plan_check.cpp checks both with g++.
//
// One feed.  Session i has p_i samples per row waiting in its FIFO (p_i < 1024) and brings n_i more: H_i = (p_i + n_i) / 1024 hops in
// hand.  The feed runs in rounds of at most max_hops hops; round j is one gather launch, ONE hops call of L_j = min(max_hops, the most
// hops any session still has) hops, one scatter launch.  Session i takes h_ij = min(hops it has left, L_j) of them, and because
// L_j < max_hops only when nobody has more left, h_ij = min(H_i - j * max_hops, max_hops) (0 once that is negative): a session's share of
// a round does not depend on who else is fed.
// Where the samples of a row's hops come from: the stream of the row is FIFO[0, p) ++ input[0, n).  Round j takes stream positions
// [1024 * done, 1024 * (done + h)), done = min(H, j * max_hops): the FIFO's samples lead the session's FIRST round and no other, all
// else is input.  What is left after the last hop, stream positions [1024 * H, p + n), becomes the FIFO's new content, stored by the
// gather launch of the session's last round with a hop.  A session without a whole hop only appends its input at FIFO offset p (in
// round 0: the feed's only launch when nobody has a hop).
// THE INVARIANT.  When at least one hop is consumed (H >= 1), 1024 * H > p, so the new remainder lies entirely in the INPUT and goes to
// FIFO offset 0; when none is, nothing of the FIFO is read at all.  So the source of a FIFO store is never the FIFO: no entry copies the
// FIFO onto itself.  One launch may still read a row's old FIFO content (into the rectangle) and store its new one - when the session's
// first round is also its last - and both lie in the FIFO's first 1024 floats; pool.hip therefore gives both to the SAME workgroup, the
// one that owns the row's first segment, which stores behind a barrier that follows its reads.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bsrnn {

constexpr int POOL_HOP = 1024;

// ---- slots: open hands out the lowest free one, close frees it; the pending count lives with the slot
struct PoolSlots {
    std::vector<uint8_t> open;
    std::vector<int32_t> pending;          // samples per row waiting, < POOL_HOP; 0 for a free slot
};
inline void pool_slots_init(PoolSlots& s, int slots)
{
    s.open.assign((size_t)(slots > 0 ? slots : 0), 0);
    s.pending.assign(s.open.size(), 0);
}
inline bool pool_slot_is_open(const PoolSlots& s, int slot) { return slot >= 0 && slot < (int)s.open.size() && s.open[(size_t)slot]; }
// -> the slot, or -1 when every slot is taken
inline int pool_slot_open(PoolSlots& s)
{
    for (size_t i = 0; i < s.open.size(); ++i)
        if (!s.open[i]) { s.open[i] = 1; s.pending[i] = 0; return (int)i; }
    return -1;
}
// -> false for a slot that is not open
inline bool pool_slot_close(PoolSlots& s, int slot)
{
    if (!pool_slot_is_open(s, slot)) return false;
    s.open[(size_t)slot] = 0;
    s.pending[(size_t)slot] = 0;
    return true;
}

// ---- the round plan
inline int64_t pool_hops_in_hand(int32_t p, int64_t n) { return (p + n) / POOL_HOP; }
inline int32_t pool_pending_after(int32_t p, int64_t n) { return (int32_t)((p + n) % POOL_HOP); }
// Rounds of a feed whose busiest session has h_max hops in hand; a feed without a hop still has its one gather launch (round 0)
inline int64_t pool_rounds(int64_t h_max, int max_hops) { return h_max <= 0 ? 1 : (h_max + max_hops - 1) / max_hops; }
// Hops of the hops call of round j (0: no call, only possible in round 0)
inline int32_t pool_round_hops(int64_t h_max, int max_hops, int64_t j)
{
    const int64_t left = h_max - j * max_hops;
    return (int32_t)(left <= 0 ? 0 : (left < max_hops ? left : max_hops));
}

// What round j means to one row of a session at (p, n).  Offsets count samples from the start of the row's input / output of this feed.
struct PoolPart {
    int32_t hops;         // h_ij
    int32_t n_fifo;       // samples the FIFO gives to the front of the rectangle's row (the session's first round only)
    int32_t n_in;         // samples the input gives behind them: n_fifo + n_in = hops * 1024
    int64_t in_off;       // ... from this offset of the input
    int64_t out_off;      // where the round's hops * 1024 output samples go in the session's output
    int32_t n_pend;       // samples this round stores into the FIFO (0: none)
    int32_t pend_off;     // ... at this FIFO offset: p when nothing was consumed, else 0
    int64_t pend_src;     // ... from this offset of the INPUT (never from the FIFO: the invariant above)
};
inline PoolPart pool_part(int32_t p, int64_t n, int max_hops, int64_t j)
{
    PoolPart q{};
    const int64_t H = pool_hops_in_hand(p, n);
    const int64_t done = H < j * max_hops ? H : j * max_hops;
    const int64_t h = H - done < max_hops ? H - done : max_hops;
    q.hops = (int32_t)h;
    q.out_off = done * POOL_HOP;
    if (h > 0) {
        q.n_fifo = done == 0 ? p : 0;
        q.n_in = (int32_t)(h * POOL_HOP - q.n_fifo);
        q.in_off = done == 0 ? 0 : done * POOL_HOP - p;
    }
    if (H == 0) {                      // no hop: append what came, in round 0
        if (j == 0) { q.n_pend = (int32_t)n; q.pend_off = p; q.pend_src = 0; }
    } else if (h > 0 && done + h == H) {      // the round of the last hop: the remainder, all of it input
        q.n_pend = pool_pending_after(p, n);
        q.pend_off = 0;
        q.pend_src = H * POOL_HOP - p;
    }
    return q;
}

// ---- the table both kernels read: one entry per row of every named session, per round.  Plain pointers, so a source may be the caller's
// device buffer, the pool's staging mirror (the host form) or any other device-resident buffer; only 4-byte alignment is assumed.
struct PoolEntry {
    const float* src;         // gather: n_in samples for the rectangle, behind the FIFO's
    const float* pend_src;    // gather: n_pend samples for the FIFO
    float* dst;               // scatter: n_out samples of the output rectangle's row go here
    int32_t row;              // row of the rectangles and of the FIFO
    int32_t n_fifo, n_in;
    int32_t n_pend, pend_off;
    int32_t n_out;            // hops * 1024
    int32_t out_skip;         // scatter: the row's first out_skip samples (0 or 1024) are not handed on; dst is where sample out_skip goes.
                              // A session with a sample rate of its own, in the round of its first hop (pool_rates_host.h); else 0.
    int32_t reserved;         // (keeps the pointers of the next entry 8-byte aligned; 0)
};
static_assert(sizeof(PoolEntry) == 56, "three pointers and eight 32-bit words");

// Entry of row `row`, whose input and output of this feed start at in_row / out_row (either may be null when nothing is taken / given)
inline PoolEntry pool_entry(const PoolPart& q, int32_t row, const float* in_row, float* out_row)
{
    PoolEntry e;
    e.src = q.n_in ? in_row + q.in_off : nullptr;
    e.pend_src = q.n_pend ? in_row + q.pend_src : nullptr;
    e.dst = q.hops ? out_row + q.out_off : nullptr;
    e.row = row;
    e.n_fifo = q.n_fifo; e.n_in = q.n_in;
    e.n_pend = q.n_pend; e.pend_off = q.pend_off;
    e.n_out = q.hops * POOL_HOP;
    e.out_skip = 0; e.reserved = 0;
    return e;
}

}  // namespace bsrnn
