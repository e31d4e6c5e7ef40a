// Sessions at their own sample rates in the native session pool (bsrnn_pool_create_rates, bsrnn_pool_open_rate, bsrnn_pool_drain): what
// one feed and one drain mean to a session in COUNTS - how many samples each stage takes and gives - and how large the pool's two
// staging rectangles have to be.  Host-only arithmetic, no HIP types, on top of resample_host.h (the conversions' definition),
// resample_bank_host.h (a row's position in its stream) and pool_host.h (hops and what waits): api_pool.hip plans with it,
// tests/cpp/pool_rates_check.cpp checks it with g++.
//
// A session at rate r sits on pair k of the pool's inbound bank (r -> 44100) and on pair k of its outbound bank (44100 -> r), with a
// BankPos in each, the same for all its rows.  Between them lie the FIFO and the stream, which count at the model's rate.  `skip` is
// what is left of the stream's one-hop delay to be dropped from the session's audio: POOL_HOP from open (or drain) until the session's
// first hop has run, 0 afterwards - always a whole hop, because the stream's output comes in whole hops.
//
// One feed of n samples at rate r, p samples waiting in the FIFO:
//   a     = bank_row_ready(in, n)         samples at 44.1 kHz, into the session's rows of conv_in
//   H     = (p + a) / 1024                hops, run in the rounds of pool_host.h with conv_in as the input
//   d     = min(skip, 1024 * H)           dropped: the first hop of the first round is not handed on
//   b     = 1024 * H - d                  samples in the session's rows of conv_out
//   n_out = bank_row_ready(out, b)        samples at rate r, to the session's own pointer
// A session at the model's rate has a = n, d = 0 and n_out = b: pool_host.h's numbers.
#pragma once
#include "pool_host.h"
#include "resample_bank_host.h"

namespace bsrnn {

constexpr int POOL_MODEL_RATE = 44100;

// Where a session with a rate stands between two calls
struct PoolRateSess {
    BankPos in, out;                 // its rows of the two banks (every row of a session stands at the same place)
    int32_t skip = POOL_HOP;         // samples of the stream's delay still to be dropped: POOL_HOP or 0
};

// What one feed means to the session, and where it leaves it
struct PoolRateFeed {
    int64_t a, hops, b, n_out;
    int32_t drop;                    // d
    int32_t pending, skip;           // afterwards
};

// qin: r -> 44100, qout: 44100 -> r.  p samples wait, n >= 0 arrive.
inline PoolRateFeed pool_rate_feed(const ResampleRatio& qin, const ResampleRatio& qout, const PoolRateSess& s, int32_t p, int64_t n)
{
    PoolRateFeed f{};
    f.a = bank_row_ready(qin, s.in, n);
    f.hops = pool_hops_in_hand(p, f.a);
    const int64_t whole = f.hops * POOL_HOP;
    f.drop = (int32_t)(s.skip < whole ? s.skip : whole);
    f.b = whole - f.drop;
    f.n_out = bank_row_ready(qout, s.out, f.b);
    f.pending = pool_pending_after(p, f.a);
    f.skip = s.skip - f.drop;
    return f;
}
// The same for a session at the model's rate: pool_host.h's numbers
inline PoolRateFeed pool_plain_feed(int32_t p, int64_t n)
{
    PoolRateFeed f{};
    f.a = n;
    f.hops = pool_hops_in_hand(p, n);
    f.b = f.n_out = f.hops * POOL_HOP;
    f.pending = pool_pending_after(p, n);
    return f;
}

// The positions after a feed of n samples that gave f (the banks' own rule: a row that takes nothing stays where it is)
inline void pool_rate_advance(PoolRateSess& s, int64_t n, const PoolRateFeed& f)
{
    if (n > 0) { s.in.N += n; s.in.J += f.a; s.in.cur ^= 1; }
    if (f.b > 0) { s.out.N += f.b; s.out.J += f.n_out; s.out.cur ^= 1; }
    s.skip = f.skip;
}

// A drain: the inbound rows are flushed (owed samples), what waits is padded with zeros to a whole hop, one more hop of zeros follows
// for the stream's delay, those hops run, the outbound rows take them (n1 samples) and are flushed (n2 more).  Afterwards the session
// stands at the beginning: both positions 0, skip = POOL_HOP, nothing pending.
struct PoolRateDrain {
    int64_t owed_in, pad, n_feed;    // n_feed = owed_in + pad + POOL_HOP samples in conv_in: the flush's, then zeros
    int64_t hops, b;
    int32_t drop;
    int64_t n1, n2, n_out;           // n_out = n1 + n2
};
inline PoolRateDrain pool_rate_drain(const ResampleRatio& qin, const ResampleRatio& qout, const PoolRateSess& s, int32_t p)
{
    PoolRateDrain g{};
    g.owed_in = bank_row_owed(qin, s.in);
    g.pad = (POOL_HOP - (p + g.owed_in) % POOL_HOP) % POOL_HOP;
    g.n_feed = g.owed_in + g.pad + POOL_HOP;
    g.hops = pool_hops_in_hand(p, g.n_feed);
    const int64_t whole = g.hops * POOL_HOP;
    g.drop = (int32_t)(s.skip < whole ? s.skip : whole);
    g.b = whole - g.drop;
    g.n1 = bank_row_ready(qout, s.out, g.b);
    BankPos after = s.out;
    after.N += g.b; after.J += g.n1;
    g.n2 = bank_row_owed(qout, after);
    g.n_out = g.n1 + g.n2;
    return g;
}
// A session at the model's rate: the padded hops and the extra one, as the stream gives them
inline PoolRateDrain pool_plain_drain(int32_t p)
{
    PoolRateDrain g{};
    g.pad = (POOL_HOP - p % POOL_HOP) % POOL_HOP;
    g.n_feed = g.pad + POOL_HOP;
    g.hops = pool_hops_in_hand(p, g.n_feed);
    g.b = g.n1 = g.n_out = g.hops * POOL_HOP;
    return g;
}

// ---- the staging rectangles conv_in [C][cap_in] and conv_out [C][cap_out]
// The most one feed of n samples can give a row of pair q: the count of a fresh row's final length, plus one for a row whose earlier
// samples left an output just short of determined.
inline int64_t pool_rate_most_ready(const ResampleRatio& q, int64_t n) { return resample_n_out(n, q.up, q.down) + 1; }
// The most a flush can owe a row of pair q: the outputs whose last input lies within half / up of the stream's end
inline int64_t pool_rate_most_owed(const ResampleRatio& q) { return q.half / q.down + 2; }

// cap_in for the inbound pairs qin [n] and feeds of at most max_block samples: the largest a, and a drain's flush plus its padding
// (fewer than a hop) plus the extra hop; whole hops, so that every row starts 16-byte aligned.
inline int64_t pool_rates_cap_in(const ResampleRatio* qin, int n, int64_t max_block)
{
    int64_t cap = 2 * POOL_HOP;
    for (int k = 0; k < n; ++k) {
        const int64_t a = pool_rate_most_ready(qin[k], max_block), f = pool_rate_most_owed(qin[k]) + 2 * POOL_HOP - 1;
        cap = a > cap ? a : cap;
        cap = f > cap ? f : cap;
    }
    return (cap + POOL_HOP - 1) / POOL_HOP * POOL_HOP;
}
// cap_out: the hops that what waited (fewer than a hop) and cap_in samples can make
inline int64_t pool_rates_cap_out(int64_t cap_in) { return (POOL_HOP - 1 + cap_in) / POOL_HOP * POOL_HOP; }

}  // namespace bsrnn
