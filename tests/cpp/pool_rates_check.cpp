// Host check of csrc/pool_rates_host.h: the counts of a feed and of a drain of a session with a sample rate of its own in the native
// session pool, against the step-by-step composition they stand for - a streaming resampler's counts (resample_host.h) in front of the
// pool's hops and pending arithmetic (pool_host.h) and another behind it - the staging capacities, and the LENGTH rule of drain.
// Build: g++ -O2 -std=c++17 -Wall -Werror -I speechseparation_amd/csrc tests/cpp/pool_rates_check.cpp -o pool_rates_check ; prints "ok".
#include "pool_rates_host.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace bsrnn;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// A single-pair streaming resampler's counts, as bsrnn_resampler_process / _flush keep them
struct Rs {
    ResampleRatio q;
    int64_t N = 0, J = 0;
    int64_t process(int64_t n)
    {
        N += n;
        const int64_t J1 = resample_ready(N, q.up, q.down, q.half), c = J1 - J;
        J = J1;
        return c;
    }
    int64_t flush()
    {
        const int64_t c = resample_n_out(N, q.up, q.down) - J;
        N = J = 0;
        return c;
    }
};

// The composition: resampler, the pool's FIFO and hops, the dropped first hop, resampler
struct Composition {
    Rs in, out;
    int32_t pending = 0, skip = POOL_HOP;
    int64_t fed = 0, received = 0;
    int64_t feed_model_rate(int64_t a, int64_t* hops)
    {
        *hops = pool_hops_in_hand(pending, a);
        pending = pool_pending_after(pending, a);
        int64_t whole = *hops * POOL_HOP;
        const int64_t k = skip < whole ? skip : whole;
        skip -= (int32_t)k;
        return whole - k;
    }
};

static void script(int rate, int64_t max_block, unsigned seed, bool never_a_hop)
{
    const ResampleRatio qin = resample_ratio(rate, POOL_MODEL_RATE), qout = resample_ratio(POOL_MODEL_RATE, rate);
    CHECK(qin.why == RESAMPLE_OK && qout.why == RESAMPLE_OK);
    const int64_t cap_in = pool_rates_cap_in(&qin, 1, max_block), cap_out = pool_rates_cap_out(cap_in);
    CHECK(cap_in % POOL_HOP == 0 && cap_out % POOL_HOP == 0);
    std::mt19937 rng(seed);
    Composition c;
    c.in.q = qin; c.out.q = qout;
    PoolRateSess s;
    int32_t p = 0;
    const int ticks = never_a_hop ? 3 : 40;
    for (int t = 0; t < ticks; ++t) {
        int64_t n;
        const unsigned kind = rng() % 8;
        if (never_a_hop) n = 1 + rng() % 20;                       // far below what a hop at 44.1 kHz needs, filters included
        else if (t == 0) n = 0;
        else if (t == 1) n = 1;
        else if (t == 2 || kind == 0) n = max_block;
        else if (kind == 1) n = 0;
        else if (kind == 2) n = 1;
        else n = rng() % (max_block + 1);
        const PoolRateFeed f = pool_rate_feed(qin, qout, s, p, n);
        // step by step
        const int64_t a = c.in.process(n);
        int64_t hops = 0;
        const int64_t b = c.feed_model_rate(a, &hops);
        const int64_t n_out = c.out.process(b);
        c.fed += n; c.received += n_out;
        CHECK(f.a == a && f.hops == hops && f.b == b && f.n_out == n_out);
        CHECK(f.pending == c.pending && f.skip == c.skip && (f.skip == 0 || f.skip == POOL_HOP));
        CHECK(f.drop == 0 || f.drop == POOL_HOP);
        CHECK(f.a <= cap_in && f.hops * POOL_HOP <= cap_out && f.b <= cap_out);
        // the descriptors' own arithmetic agrees (resample_bank_host.h)
        BankRow d; BankPos nx;
        CHECK(bank_row_process(qin, s.in, n, d, nx) == BANK_OK && (int64_t)d.n_j == a);
        CHECK(bank_row_process(qout, s.out, b, d, nx) == BANK_OK && (int64_t)d.n_j == n_out);
        pool_rate_advance(s, n, f);
        p = f.pending;
        CHECK(s.in.N == c.in.N && s.in.J == c.in.J && s.out.N == c.out.N && s.out.J == c.out.J);
        // a drain now and then, and at the end
        if (t == ticks - 1 || rng() % 16 == 0) {
            const PoolRateDrain g = pool_rate_drain(qin, qout, s, p);
            const int64_t owed = c.in.flush();
            const int64_t pad = (POOL_HOP - (c.pending + owed) % POOL_HOP) % POOL_HOP;
            int64_t h2 = 0;
            const int64_t b2 = c.feed_model_rate(owed + pad + POOL_HOP, &h2);
            const int64_t n1 = c.out.process(b2), n2 = c.out.flush();
            CHECK(c.pending == 0);
            CHECK(g.owed_in == owed && g.pad == pad && g.n_feed == owed + pad + POOL_HOP && g.hops == h2 && g.b == b2);
            CHECK(g.n1 == n1 && g.n2 == n2 && g.n_out == n1 + n2);
            CHECK(g.n_feed <= cap_in && g.hops * POOL_HOP <= cap_out);
            CHECK(owed <= pool_rate_most_owed(qin));
            if (never_a_hop) CHECK(c.received == 0);
            c.received += n1 + n2;
            // LENGTH: n samples fed at r give resample_len(m, 44100, r), m = resample_len(n, r, 44100) in whole hops
            const int64_t m0 = resample_n_out(c.fed, qin.up, qin.down), m = (m0 + POOL_HOP - 1) / POOL_HOP * POOL_HOP;
            CHECK(c.received == resample_n_out(m, qout.up, qout.down));
            c.fed = c.received = 0;
            c.skip = POOL_HOP;
            s = PoolRateSess();
            p = 0;
        }
    }
}

static void plain(unsigned seed)
{
    std::mt19937 rng(seed);
    int32_t p = 0;
    for (int t = 0; t < 200; ++t) {
        const int64_t n = t < 2 ? t : rng() % 9000;
        const PoolRateFeed f = pool_plain_feed(p, n);
        CHECK(f.a == n && f.hops == pool_hops_in_hand(p, n) && f.drop == 0 && f.b == f.hops * POOL_HOP && f.n_out == f.b);
        CHECK(f.pending == pool_pending_after(p, n));
        int64_t given = 0;
        for (int64_t j = 0; j < pool_rounds(f.hops, 3); ++j) given += (int64_t)pool_part(p, n, 3, j).hops * POOL_HOP;
        CHECK(given == f.n_out);
        p = f.pending;
        const PoolRateDrain g = pool_plain_drain(p);
        CHECK((p + g.n_feed) % POOL_HOP == 0 && g.n_out == (p + POOL_HOP - 1) / POOL_HOP * POOL_HOP + POOL_HOP && g.n_feed < 2 * POOL_HOP + 1);
    }
}

int main()
{
    const int rates[] = {8000, 16000, 22050, 32000, 48000, 96000};
    unsigned seed = 1;
    for (int r : rates) {
        for (int64_t max_block : {(int64_t)1, (int64_t)700, (int64_t)4800, (int64_t)48000})
            for (int k = 0; k < 6; ++k) script(r, max_block, seed++, false);
        script(r, 48000, seed++, true);
        // what a flush can owe, at every place of a short stream
        const ResampleRatio q = resample_ratio(r, POOL_MODEL_RATE), qo = resample_ratio(POOL_MODEL_RATE, r);
        for (const ResampleRatio& x : {q, qo})
            for (int64_t N = 0; N < 5000; ++N) {
                BankPos p; p.N = N; p.J = resample_ready(N, x.up, x.down, x.half);
                CHECK(bank_row_owed(x, p) <= pool_rate_most_owed(x));
                CHECK(bank_row_ready(x, p, 777) <= pool_rate_most_ready(x, 777));
            }
    }
    // several rates: the capacity is the largest any of them needs
    ResampleRatio q[3] = {resample_ratio(8000, POOL_MODEL_RATE), resample_ratio(48000, POOL_MODEL_RATE), resample_ratio(96000, POOL_MODEL_RATE)};
    for (int k = 0; k < 3; ++k) CHECK(pool_rates_cap_in(q, 3, 4800) >= pool_rates_cap_in(q + k, 1, 4800));
    plain(99);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
