// Drives csrc/sections_host.h for tests/test_sections_host.py (host only; built with -Wall -Werror, and with the sanitizers).
//   defaults                                   the default rule, one line
//   refusals                                   sections_check's answers for the bad argument sets, one line
//   scan FILE R0..R6 CAP FLUSH [SPLIT...|each] FILE: float64 [n][2]; R0..R6 the rule's seven fields; the hops are fed in the pieces the
//                                              split positions cut ("each": hop by hop), the last piece with FLUSH; per feed a line
//                                              "feed <n_out>" and the sections written (at most CAP), at the end the state
//   splits FILE R0..R6                         every split into two feeds, and hop by hop, against one feed; prints "ok <n>"
#include "sections_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace bsrnn;

static std::vector<double> read_doubles(const char* path)
{
    std::vector<double> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    double buf[256];
    size_t n;
    while ((n = fread(buf, sizeof(double), 256, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    if (v.size() % 2) { fprintf(stderr, "%s: odd number of doubles\n", path); exit(2); }
    return v;
}

static SectionRule rule_from(char** a)
{
    SectionRule q;
    q.dialog_db = atof(a[0]); q.bridge_db = atof(a[1]); q.background_db = atof(a[2]); q.silence_db = atof(a[3]);
    q.level_floor = atof(a[4]); q.floor_db = atof(a[5]); q.min_run = atoi(a[6]);
    return q;
}

static bool same(const std::vector<Section>& a, const std::vector<Section>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].kind != b[i].kind || a[i].first_hop != b[i].first_hop || a[i].end_hop != b[i].end_hop) return false;
    return true;
}

// the hops [a, b) into st, appended to out
static void feed(const SectionRule& q, SectionState& st, const std::vector<double>& act, int64_t a, int64_t b, bool flush, std::vector<Section>& out)
{
    std::vector<Section> got((size_t)(b - a) + 1);
    const int64_t n = sections_scan(q, st, act.data() + 2 * a, b - a, flush, got.data(), (int64_t)got.size());
    if (n > (int64_t)got.size()) { fprintf(stderr, "more sections than hops + 1\n"); exit(3); }
    out.insert(out.end(), got.begin(), got.begin() + n);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "defaults") {
        const SectionRule q;
        const SectionState st;
        printf("%.17g %.17g %.17g %.17g %.17g %.17g %d | %lld %lld %d %lld %lld\n", q.dialog_db, q.bridge_db, q.background_db, q.silence_db,
               q.level_floor, q.floor_db, q.min_run, (long long)st.n_dialog, (long long)st.n_background, st.open_kind, (long long)st.open_hop,
               (long long)st.hop);
        return 0;
    }
    if (mode == "refusals") {
        SectionRule q, bad;
        bad.min_run = 0;
        SectionState st;
        const double act[2] = {1.0, 1.0};
        int64_t n = 0;
        printf("%d %d %d %d %d %d %d %d\n", sections_check(q, nullptr, act, 1, 1, &n), sections_check(q, &st, act, 1, 1, nullptr),
               sections_check(q, &st, act, -1, 1, &n), sections_check(q, &st, act, 1, -1, &n), sections_check(bad, &st, act, 1, 1, &n),
               sections_check(q, &st, nullptr, 1, 1, &n), sections_check(q, &st, nullptr, 0, 0, &n), sections_check(q, &st, act, 1, 0, &n));
        return 0;
    }
    if (mode == "scan" && argc >= 12) {
        const std::vector<double> act = read_doubles(argv[2]);
        const SectionRule q = rule_from(argv + 3);
        const int64_t cap = atoll(argv[10]), n = (int64_t)act.size() / 2;
        const bool flush = atoi(argv[11]) != 0;
        std::vector<int64_t> cuts;
        if (argc == 13 && !strcmp(argv[12], "each")) { for (int64_t i = 1; i < n; ++i) cuts.push_back(i); }
        else for (int i = 12; i < argc; ++i) cuts.push_back(atoll(argv[i]));
        cuts.push_back(n);
        SectionState st;
        std::vector<Section> out((size_t)cap);          // exactly cap: the sanitizers see a write behind it
        int64_t at = 0;
        for (size_t k = 0; k < cuts.size(); ++k) {
            const int64_t b = cuts[k];
            if (b < at || b > n) { fprintf(stderr, "bad split\n"); return 2; }
            const int64_t got = sections_scan(q, st, act.data() + 2 * at, b - at, flush && k + 1 == cuts.size(), out.data(), cap);
            printf("feed %lld\n", (long long)got);
            for (int64_t i = 0; i < got && i < cap; ++i) printf("%d %lld %lld\n", out[i].kind, (long long)out[i].first_hop, (long long)out[i].end_hop);
            at = b;
        }
        printf("state %lld %lld %d %lld %lld\n", (long long)st.n_dialog, (long long)st.n_background, st.open_kind,
               st.open_kind ? (long long)st.open_hop : 0LL, (long long)st.hop);
        return 0;
    }
    if (mode == "splits" && argc >= 10) {
        const std::vector<double> act = read_doubles(argv[2]);
        const SectionRule q = rule_from(argv + 3);
        const int64_t n = (int64_t)act.size() / 2;
        SectionState one;
        std::vector<Section> want;
        feed(q, one, act, 0, n, true, want);
        for (int64_t cut = 0; cut <= n; ++cut) {
            SectionState st;
            std::vector<Section> got;
            feed(q, st, act, 0, cut, false, got);
            feed(q, st, act, cut, n, true, got);
            if (!same(got, want) || st.hop != n) { printf("split at %lld differs\n", (long long)cut); return 1; }
        }
        SectionState st;
        std::vector<Section> got;
        for (int64_t i = 0; i < n; ++i) feed(q, st, act, i, i + 1, false, got);
        feed(q, st, act, n, n, true, got);
        if (!same(got, want)) { printf("hop by hop differs\n"); return 1; }
        printf("ok %lld\n", (long long)want.size());
        return 0;
    }
    return 2;
}
