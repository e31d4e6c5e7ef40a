// Checks of csrc/resample_bank_host.h with a plain C++ compiler (tests/test_resample_bank_host.py builds and runs this):
//   self                     random per-row schedules of blocks, holds, flushes, resets and re-assignments over several pairs: every row
//                            of the bank against a single-pair stream of its pair computed from resample_host.h alone, the descriptor's
//                            fields against that stream's absolute positions, and the kernel's tile arithmetic against the absolute form
//   desc ri ro N J cur pair n_in flush
//                            one descriptor: "why n_in n_j keep n_carry lead phase column pair cur runs carries  N1 J1 cur1"
//   group                    "sizeof(BankRow) BANK_GROUP_ROWS sizeof(BankRows) BANK_ARG_SPACE BANK_ARG_IMPLICIT BANK_ARG_OTHER"
#include "resample_bank_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace bsrnn;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); }          \
    } while (0)

// A single-pair streaming resampler as api.hip's resampler_run keeps it: two counters, rules from resample_host.h
struct Twin {
    ResampleRatio q;
    int64_t N = 0, J = 0;
    int64_t keep_from(int64_t j) const { const int64_t b = resample_base(j, q.up, q.down, q.Kh); return b > 0 ? b : 0; }
    int64_t process(int64_t n) { N += n; const int64_t J1 = resample_ready(N, q.up, q.down, q.half), c = J1 - J; J = J1; return c; }
    int64_t flush() { const int64_t c = resample_n_out(N, q.up, q.down) - J; N = J = 0; return c; }
};

static void check_descriptor(const ResampleRatio& q, const ResampleTiling& g, const BankPos& p, const Twin& before, const BankRow& d,
                             int64_t n_in, int64_t count, bool flush, std::mt19937_64& rnd)
{
    const int64_t origin = before.keep_from(before.J);
    CHECK(d.w4 & BANK_ROW_RUNS);
    CHECK(((d.w4 & BANK_ROW_CARRIES) != 0) == !flush);
    CHECK(d.n_in == (uint32_t)n_in && d.n_j == (uint32_t)count);
    CHECK(bank_row_pair(d) == p.pair && bank_row_cur(d) == p.cur);
    CHECK(bank_row_n_carry(d) == before.N - origin);
    CHECK(bank_row_n_carry(d) <= resample_carry_floats(q));
    CHECK(bank_row_lead(d) == before.J * q.down / q.up - origin && bank_row_lead(d) <= q.Kh);
    CHECK(bank_row_phase(d) == (uint64_t)(before.J * q.down % q.up) && bank_row_column(d) == (uint64_t)(before.J % q.up));
    const int64_t J1 = before.J + count, N1 = before.N + n_in;
    CHECK(d.keep == before.keep_from(J1) - origin);
    if (!flush) CHECK(N1 - before.keep_from(J1) <= resample_carry_floats(q));            // the next carry fits
    // the kernel's tile arithmetic (resample_bank_kernel), tile bx of this call, against the absolute form of resample_kernel
    const int64_t n_tiles = (count + g.tile - 1) / g.tile;
    for (int k = 0; k < 4 && n_tiles > 0; ++k) {
        const int64_t bx = k == 0 ? 0 : k == 1 ? n_tiles - 1 : (int64_t)(rnd() % (uint64_t)n_tiles);
        const int64_t jd = bx * g.tile, c = (int64_t)bank_row_phase(d) + jd * q.down, qd = c / q.up;
        const int64_t jt = before.J + jd, ca = jt * q.down;
        CHECK(bank_row_lead(d) + qd == ca / q.up - origin);
        CHECK(c - qd * q.up == ca % q.up);
        CHECK((int64_t)((bank_row_column(d) + jd) % q.up) == jt % q.up);
        CHECK(ca / q.up - origin >= 0);
    }
}

static int self_check()
{
    const int rates[][2] = {{48000, 44100}, {16000, 44100}, {1000, 1}, {44100, 8000}, {44100, 44100}, {44100, 96000}};
    const int n_pairs = (int)(sizeof(rates) / sizeof(rates[0]));
    std::vector<ResampleRatio> q;
    std::vector<ResampleTiling> g;
    for (const auto& r : rates) { q.push_back(resample_ratio(r[0], r[1])); CHECK(q.back().why == RESAMPLE_OK); g.push_back(resample_tiling(q.back())); }
    CHECK(g[2].chunk < g[2].ld && g[2].tile == 5);                                        // the pair whose rows are walked in chunks
    CHECK(g[0].chunk == g[0].ld && g[0].tile == 1024);
    std::mt19937_64 rnd(20240917);
    const int C = 9;
    for (int round = 0; round < 40; ++round) {
        std::vector<BankPos> pos(C);
        std::vector<Twin> twin(C);
        for (int r = 0; r < C; ++r) { pos[r].pair = 0; twin[r].q = q[0]; }
        // some rounds start far into a stream: the twin's counters are set to the same place
        const bool far = round % 4 == 3;
        for (int r = 0; r < C && far; ++r) {
            const int k = (int)(rnd() % n_pairs);
            bank_row_assign(pos[r], k); twin[r].q = q[k];
            const int64_t N = ((int64_t)1 << 40) + (int64_t)(rnd() % 100000);
            twin[r].N = pos[r].N = N;
            twin[r].J = pos[r].J = resample_ready(N, q[k].up, q[k].down, q[k].half);
        }
        for (int tick = 0; tick < 60; ++tick) {
            for (int r = 0; r < C; ++r) {
                const uint64_t what = rnd() % 16;
                BankPos& p = pos[r];
                Twin& t = twin[r];
                BankRow d;
                BankPos next;
                if (what == 0) {                         // reset
                    bank_row_reset(p); t.N = t.J = 0;
                } else if (what == 1) {                  // re-assignment
                    const int k = (int)(rnd() % n_pairs);
                    bank_row_assign(p, k); t.q = q[k]; t.N = t.J = 0;
                    CHECK(p.pair == k);
                } else if (what == 2) {                  // flush
                    const Twin before = t;
                    const int64_t owed = t.flush();
                    CHECK(bank_row_owed(q[p.pair], p) == owed);
                    CHECK(bank_row_flush(q[p.pair], p, d, next) == BANK_OK);
                    CHECK(next.N == 0 && next.J == 0 && next.pair == p.pair && next.cur == p.cur);
                    if (owed > 0) check_descriptor(q[p.pair], g[p.pair], p, before, d, 0, owed, true, rnd);
                    else CHECK(!(d.w4 & BANK_ROW_RUNS) && d.n_j == 0);
                    p = next;
                } else if (what < 6) {                   // hold
                    CHECK(bank_row_ready(q[p.pair], p, 0) == 0);
                    CHECK(bank_row_process(q[p.pair], p, 0, d, next) == BANK_OK);
                    CHECK(!(d.w4 & BANK_ROW_RUNS) && d.n_in == 0 && d.n_j == 0 && bank_row_cur(d) == p.cur && bank_row_pair(d) == p.pair);
                    CHECK(next.N == p.N && next.J == p.J && next.cur == p.cur && next.pair == p.pair);
                } else {                                 // a block: short, about a hop, or many tiles
                    const int64_t n = what < 9 ? 1 + (int64_t)(rnd() % 8) : what < 14 ? 1 + (int64_t)(rnd() % 3000) : 1 + (int64_t)(rnd() % 200000);
                    const Twin before = t;
                    CHECK(bank_row_ready(q[p.pair], p, n) == resample_ready(t.N + n, t.q.up, t.q.down, t.q.half) - t.J);
                    const int64_t count = t.process(n);
                    CHECK(bank_row_process(q[p.pair], p, n, d, next) == BANK_OK);
                    check_descriptor(q[p.pair], g[p.pair], p, before, d, n, count, false, rnd);
                    CHECK(next.N == t.N && next.J == t.J && next.cur == (p.cur ^ 1) && next.pair == p.pair);
                    p = next;
                }
                CHECK(p.N == t.N && p.J == t.J);
            }
        }
    }
    // refusals of the arithmetic itself
    BankRow d;
    BankPos p, next;
    CHECK(bank_row_process(q[0], p, -1, d, next) == BANK_BAD_COUNT);
    CHECK(bank_row_process(q[0], p, BANK_BLOCK_MAX + 1, d, next) == BANK_BLOCK_TOO_LONG);
    CHECK(bank_row_process(q[5], p, BANK_BLOCK_MAX, d, next) == BANK_BLOCK_TOO_LONG);     // 44.1 -> 96 k: more comes out than a call may give
    CHECK(bank_row_process(q[0], p, BANK_BLOCK_MAX, d, next) == BANK_OK && d.n_in == (uint32_t)BANK_BLOCK_MAX);
    p.N = (INT64_MAX >> 12) - 5;
    CHECK(bank_row_process(q[0], p, 6, d, next) == BANK_BAD_COUNT);
    // the group of descriptors beside the other arguments
    CHECK(sizeof(BankRow) == 20 && sizeof(BankRows) == 20u * BANK_GROUP_ROWS);
    CHECK((int)sizeof(BankRows) + BANK_ARG_IMPLICIT + BANK_ARG_OTHER <= BANK_ARG_SPACE);
    CHECK((int)sizeof(BankRows) + (int)sizeof(BankRow) + BANK_ARG_IMPLICIT + BANK_ARG_OTHER > BANK_ARG_SPACE);      // and no row more would
    CHECK(BANK_GROUP_ROWS >= 64);
    std::printf("ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "self")) return self_check();
    if (argc == 2 && !std::strcmp(argv[1], "group")) {
        std::printf("%zu %d %zu %d %d %d\n", sizeof(BankRow), BANK_GROUP_ROWS, sizeof(BankRows), BANK_ARG_SPACE, BANK_ARG_IMPLICIT, BANK_ARG_OTHER);
        return 0;
    }
    if (argc == 10 && !std::strcmp(argv[1], "desc")) {
        const ResampleRatio q = resample_ratio(std::atoll(argv[2]), std::atoll(argv[3]));
        if (q.why != RESAMPLE_OK) return 2;
        BankPos p, next;
        p.N = std::atoll(argv[4]); p.J = std::atoll(argv[5]); p.cur = std::atoi(argv[6]); p.pair = std::atoi(argv[7]);
        const int64_t n_in = std::atoll(argv[8]);
        BankRow d;
        const int why = std::atoi(argv[9]) ? bank_row_flush(q, p, d, next) : bank_row_process(q, p, n_in, d, next);
        std::printf("%d %u %u %u %d %d %u %u %d %d %d %d  %lld %lld %d\n", why, d.n_in, d.n_j, d.keep, bank_row_n_carry(d), bank_row_lead(d),
                    bank_row_phase(d), bank_row_column(d), bank_row_pair(d), bank_row_cur(d), (d.w4 & BANK_ROW_RUNS) != 0,
                    (d.w4 & BANK_ROW_CARRIES) != 0, (long long)next.N, (long long)next.J, next.cur);
        return 0;
    }
    std::fprintf(stderr, "usage: resample_bank_check self | group | desc rate_in rate_out N J cur pair n_in flush\n");
    return 2;
}
