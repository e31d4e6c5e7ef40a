// Host check of csrc/pool_host.h: the slots, the pending arithmetic and the round plan of the native session pool (bsrnn_pool_feed).
// A CPU walk of the table entries - what pool.hip's two kernels do with them - against the naive model: the row's stream is
// concat(pending, input), cut into hops and a remainder.
// Build: g++ -O2 -std=c++17 -Wall -I speechseparation_amd/csrc tests/cpp/pool_plan_check.cpp -o pool_plan_check ; prints "ok".
#include "pool_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bsrnn;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// ---- the kernels' semantics on the host
// gather: rectangle row = FIFO[0, n_fifo) ++ src[0, n_in), zeros to L*1024; then FIFO[pend_off ...) = pend_src[0, n_pend).
// The FIFO is read BEFORE it is stored (pool.hip: one workgroup, a barrier between), and the store's source must not be the FIFO.
static void walk_gather(const PoolEntry& e, std::vector<float>& chunk, int L, float* fifo_base, int C)
{
    float* q = fifo_base + (size_t)e.row * POOL_HOP;
    if (L > 0) {
        float* d = chunk.data() + (size_t)e.row * L * POOL_HOP;
        CHECK(e.n_fifo + e.n_in <= L * POOL_HOP);
        CHECK(e.n_fifo >= 0 && e.n_fifo < POOL_HOP);
        CHECK((e.n_fifo + e.n_in) % POOL_HOP == 0);
        CHECK(e.n_fifo == 0 || e.n_in >= POOL_HOP - e.n_fifo);        // the FIFO's samples stay inside the row's first segment
        for (int i = 0; i < e.n_fifo; ++i) d[i] = q[i];
        for (int i = 0; i < e.n_in; ++i) d[e.n_fifo + i] = e.src[i];
        for (int i = e.n_fifo + e.n_in; i < L * POOL_HOP; ++i) d[i] = 0.f;
    } else {
        CHECK(e.n_fifo == 0 && e.n_in == 0);
    }
    if (e.n_pend) {
        CHECK(e.pend_off >= 0 && e.n_pend > 0 && e.pend_off + e.n_pend < POOL_HOP);
        // THE INVARIANT: the source of a FIFO store lies outside the FIFOs, and a store behind a consumed hop starts at offset 0
        const float* lo = fifo_base; const float* hi = fifo_base + (size_t)C * POOL_HOP;
        CHECK(e.pend_src + e.n_pend <= lo || e.pend_src >= hi);
        CHECK(e.n_fifo == 0 || e.pend_off == 0);
        CHECK(e.n_out == 0 ? e.n_fifo == 0 : e.pend_off == 0);          // no hop: nothing of the FIFO is read; a hop: the remainder restarts it
        for (int i = 0; i < e.n_pend; ++i) q[e.pend_off + i] = e.pend_src[i];
    }
}
// the hops call, as far as the samples' bookkeeping goes: out = chunk for a row's first count * 1024 samples, zeros behind them
static void walk_hops(const std::vector<float>& chunk, std::vector<float>& out, int L, const std::vector<int>& counts)
{
    for (size_t r = 0; r < counts.size(); ++r)
        for (int i = 0; i < L * POOL_HOP; ++i)
            out[r * L * POOL_HOP + i] = i < counts[r] * POOL_HOP ? chunk[r * L * POOL_HOP + i] : 0.f;
}
static void walk_scatter(const PoolEntry& e, const std::vector<float>& out, int L)
{
    CHECK(e.n_out <= L * POOL_HOP && e.n_out % POOL_HOP == 0);
    for (int i = 0; i < e.n_out; ++i) e.dst[i] = out[(size_t)e.row * L * POOL_HOP + i];
}

// A pool of `slots` one-row sessions on the host: feeds of arbitrary lengths per session, every sample a unique number, so that "used
// exactly once, in order" is an equality of sequences.
struct Model {
    int slots, max_hops;
    PoolSlots sl;
    std::vector<float> fifo;                       // [slots][1024]
    std::vector<std::vector<float>> fed, got;      // per slot: everything fed so far / everything that came out
    std::vector<float> next_value;
    Model(int s, int mh) : slots(s), max_hops(mh), fifo((size_t)s * POOL_HOP, -1.f), fed(s), got(s), next_value(s)
    {
        pool_slots_init(sl, s);
        for (int i = 0; i < s; ++i) next_value[i] = (float)(i * 1000000 + 1);
    }
    // -> number of hops calls the feed made
    int feed(const std::vector<int>& who, const std::vector<int64_t>& n_in)
    {
        const int n = (int)who.size();
        std::vector<std::vector<float>> in(n), outb(n);
        int64_t h_max = 0;
        for (int i = 0; i < n; ++i) {
            in[i].resize((size_t)n_in[i]);
            for (float& v : in[i]) { v = next_value[who[i]]; next_value[who[i]] += 1.f; }
            fed[who[i]].insert(fed[who[i]].end(), in[i].begin(), in[i].end());
            const int64_t H = pool_hops_in_hand(sl.pending[who[i]], n_in[i]);
            outb[i].assign((size_t)H * POOL_HOP, -7.f);
            h_max = std::max(h_max, H);
        }
        const int64_t rounds = pool_rounds(h_max, max_hops);
        int calls = 0;
        std::vector<int64_t> taken(n, 0);
        for (int64_t j = 0; j < rounds; ++j) {
            const int L = pool_round_hops(h_max, max_hops, j);
            CHECK(L <= max_hops && (L > 0 || (j == 0 && h_max == 0)));
            std::vector<float> chunk((size_t)slots * L * POOL_HOP, -3.f), out((size_t)slots * L * POOL_HOP, -5.f);
            std::vector<int> counts(slots, 0);
            std::vector<PoolEntry> tab;
            int longest = 0;
            for (int i = 0; i < n; ++i) {
                const PoolPart q = pool_part(sl.pending[who[i]], n_in[i], max_hops, j);
                // the issue's rule: a session takes min(hops left, L_j)
                const int64_t left = pool_hops_in_hand(sl.pending[who[i]], n_in[i]) - taken[i];
                CHECK(q.hops == std::min<int64_t>(left, L));
                CHECK(q.n_fifo == (taken[i] == 0 && q.hops ? sl.pending[who[i]] : 0));         // the FIFO leads the first round only
                taken[i] += q.hops;
                counts[who[i]] = q.hops;
                longest = std::max(longest, q.hops);
                if (j > 0 && q.hops == 0) { CHECK(q.n_pend == 0); continue; }
                tab.push_back(pool_entry(q, who[i], in[i].data(), outb[i].data()));
            }
            CHECK(longest == L);
            for (const PoolEntry& e : tab) walk_gather(e, chunk, L, fifo.data(), slots);
            if (L == 0) continue;
            ++calls;
            walk_hops(chunk, out, L, counts);
            for (const PoolEntry& e : tab) walk_scatter(e, out, L);
        }
        for (int i = 0; i < n; ++i) {
            CHECK(taken[i] == pool_hops_in_hand(sl.pending[who[i]], n_in[i]));
            sl.pending[who[i]] = pool_pending_after(sl.pending[who[i]], n_in[i]);
            got[who[i]].insert(got[who[i]].end(), outb[i].begin(), outb[i].end());
        }
        return calls;
    }
    // everything that came out, then what waits, is everything that went in: every sample exactly once, in order
    void check(int slot)
    {
        std::vector<float> all = got[slot];
        CHECK(all.size() % POOL_HOP == 0);
        CHECK(sl.pending[slot] >= 0 && sl.pending[slot] < POOL_HOP);
        all.insert(all.end(), fifo.begin() + (size_t)slot * POOL_HOP, fifo.begin() + (size_t)slot * POOL_HOP + sl.pending[slot]);
        CHECK(all == fed[slot]);
    }
};

int main()
{
    // ---- slots: the lowest free one, always
    {
        PoolSlots s;
        pool_slots_init(s, 4);
        CHECK(pool_slot_open(s) == 0 && pool_slot_open(s) == 1 && pool_slot_open(s) == 2);
        CHECK(pool_slot_close(s, 1) && !pool_slot_close(s, 1) && !pool_slot_close(s, 3) && !pool_slot_close(s, -1) && !pool_slot_close(s, 4));
        CHECK(pool_slot_open(s) == 1 && pool_slot_open(s) == 3 && pool_slot_open(s) == -1);
        CHECK(pool_slot_close(s, 0) && pool_slot_close(s, 2));
        s.pending[3] = 77;
        CHECK(pool_slot_open(s) == 0 && pool_slot_open(s) == 2 && pool_slot_open(s) == -1);
        CHECK(pool_slot_close(s, 3) && pool_slot_open(s) == 3 && s.pending[3] == 0);          // a slot's next session starts with nothing
        CHECK(pool_slot_is_open(s, 3) && !pool_slot_is_open(s, 4) && !pool_slot_is_open(s, -1));
    }
    // ---- pending arithmetic over feeds of 0, 700, 1024, 2500 and 3072 samples
    {
        const int64_t feeds[] = {0, 700, 1024, 2500, 3072, 700, 0, 1024, 3072, 2500};
        int32_t p = 0;
        int64_t total = 0, hops = 0;
        for (int64_t n : feeds) {
            hops += pool_hops_in_hand(p, n);
            p = pool_pending_after(p, n);
            total += n;
            CHECK(p == total % POOL_HOP && hops == total / POOL_HOP);
        }
        CHECK(pool_hops_in_hand(1023, 0) == 0 && pool_hops_in_hand(1023, 1) == 1 && pool_pending_after(1023, 1) == 0);
    }
    // ---- rounds
    CHECK(pool_rounds(0, 2) == 1 && pool_rounds(1, 2) == 1 && pool_rounds(2, 2) == 1 && pool_rounds(3, 2) == 2 && pool_rounds(5, 2) == 3);
    CHECK(pool_rounds(255, 255) == 1 && pool_rounds(256, 255) == 2);
    CHECK(pool_round_hops(5, 2, 0) == 2 && pool_round_hops(5, 2, 1) == 2 && pool_round_hops(5, 2, 2) == 1 && pool_round_hops(0, 2, 0) == 0);
    {   // the example of the GPU test: 5 hops + 300 samples beside 1 hop at max_hops = 2 -> counts 2 / 2 / 1 and 1 / 0 / 0
        const int want_a[3] = {2, 2, 1}, want_b[3] = {1, 0, 0};
        for (int j = 0; j < 3; ++j) {
            CHECK(pool_part(0, 5 * 1024 + 300, 2, j).hops == want_a[j]);
            CHECK(pool_part(0, 1024, 2, j).hops == want_b[j]);
        }
        CHECK(pool_part(0, 5 * 1024 + 300, 2, 2).n_pend == 300 && pool_part(0, 5 * 1024 + 300, 2, 1).n_pend == 0);
        CHECK(pool_part(0, 1024, 2, 0).n_pend == 0);
    }
    // ---- the walk: three sessions, the feeds of the GPU test's script and more, at max_hops 2, 3 and 255
    for (int max_hops : {2, 3, 255}) {
        Model m(4, max_hops);
        for (int i = 0; i < 3; ++i) CHECK(pool_slot_open(m.sl) == i);
        const int64_t script[8][3] = {{0, 700, 1024}, {700, 1024, 2500}, {1024, 2500, 3072}, {2500, 3072, 0},
                                      {3072, 0, 700}, {324, 324, 1023}, {1, 5 * 1024 + 300, 0}, {1024, 1024, 1024}};
        for (const auto& t : script) {
            int64_t h_max = 0;
            for (int i = 0; i < 3; ++i) h_max = std::max(h_max, pool_hops_in_hand(m.sl.pending[i], t[i]));
            const int calls = m.feed({0, 1, 2}, {t[0], t[1], t[2]});
            CHECK(calls == (int)((h_max + max_hops - 1) / max_hops));       // nobody has a hop: no call at all
            for (int i = 0; i < 3; ++i) m.check(i);
        }
        // a session not named keeps what waits; one fed alone, one fed nothing
        const int32_t p1 = m.sl.pending[1];
        m.feed({2, 0}, {999, 0});
        CHECK(m.sl.pending[1] == p1);
        m.feed({1}, {3 * 1024 - p1});
        CHECK(m.sl.pending[1] == 0);
        for (int i = 0; i < 3; ++i) m.check(i);
        // many hops in one feed: 600 hops is three rounds at 255, 300 at 2
        const int64_t h0 = pool_hops_in_hand(m.sl.pending[0], 600 * 1024 + 5);
        CHECK(h0 >= 600 && m.feed({0, 2}, {600 * 1024 + 5, 1}) == (int)((h0 + max_hops - 1) / max_hops));
        for (int i = 0; i < 3; ++i) m.check(i);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
