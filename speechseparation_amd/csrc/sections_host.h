// Dialog / background section mining, the host end (bsrnn_sections_scan): the run-length state machine of the reference's
// gendataset-separate.py:103-149 over the per-hop figures that bsrnn_hop_activity leaves - for every hop of 1024 samples the mean of
// est^2 / (mix - est)^2 and the mean of mix^2.  Host arithmetic only, no HIP, no allocation, so tests run it without a GPU
// (tests/cpp/sections_check.cpp) and a C host or the LADSPA side can use it through the C ABI.
//
// Per hop:  db    = 10 ln(ratio)                                  natural logs, as the reference writes them (:104, :109)
//           level = floor_db if level_mean < level_floor, else 10 ln(level_mean)
// A ratio of exactly 0 (an all-zero estimate) gives db = -inf.  The reference's math.log(0) raises there; this is the one deliberate
// deviation.  +inf and NaN pass through; a NaN db fails every comparison below, so such a hop can only bridge (through its level) or reset.
// Then, in this order:
//   1. db > dialog_db:       if n_background > 0, it goes to 0 and the open section closes; ++n_dialog; if n_dialog >= min_run and no
//                            section is open, a dialog section opens AT THIS HOP (the first min_run - 1 hops of a run are not part of it)
//   2. else (db > bridge_db or level < silence_db) and n_dialog >= min_run: the hop belongs to the open section, no counter moves
//   3. else db < background_db: the mirror image of 1 for background
//   4. else: both counters go to 0 and the open section closes
// A closed section is {kind, first_hop, end_hop}, end_hop exclusive; a flush closes an open section behind the last hop consumed.
// The state carries everything from call to call: feeding the hops of a stream in any split gives the sections of one call.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace bsrnn {

constexpr int ACT_RATIO = 0, ACT_LEVEL = 1, ACT_Q = 2;          // the order of BSRNN_ACT_* (api.hip asserts that the two agree)
constexpr int SECTION_NONE = 0, SECTION_DIALOG = 1, SECTION_BACKGROUND = 2;

// The fields of bsrnn_section_rule / _state of include/bsrnn_hip.h, in their order (api.hip copies them field by field)
struct SectionRule {
    double dialog_db = 10.0, bridge_db = 3.0, background_db = -30.0, silence_db = -100.0;      // gendataset-separate.py:111, :126, :129
    double level_floor = 1e-10, floor_db = -200.0;                                            // :106-107
    int32_t min_run = 10;                                                                     // :120, :138
};
struct SectionState {
    int64_t n_dialog = 0, n_background = 0;
    int32_t open_kind = SECTION_NONE;
    int64_t open_hop = 0;            // first hop of the open section (meaningless while none is open)
    int64_t hop = 0;                 // hops consumed so far
};
struct Section { int32_t kind; int64_t first_hop, end_hop; };

inline double section_db(double ratio)
{
    return ratio == 0.0 ? -std::numeric_limits<double>::infinity() : 10.0 * std::log(ratio);
}
inline double section_level(const SectionRule& q, double level_mean)
{
    return level_mean < q.level_floor ? q.floor_db : 10.0 * std::log(level_mean);
}

enum SectionsWhy { SECTIONS_OK, SECTIONS_NULL_STATE, SECTIONS_NULL_COUNT, SECTIONS_NEGATIVE, SECTIONS_MIN_RUN, SECTIONS_NULL_ACT };

// (st: the caller's state object, whatever its type - only its presence is looked at)
inline SectionsWhy sections_check(const SectionRule& q, const void* st, const double* act, int64_t n_hops, int64_t cap, const int64_t* n_out)
{
    if (!st) return SECTIONS_NULL_STATE;
    if (!n_out) return SECTIONS_NULL_COUNT;
    if (n_hops < 0 || cap < 0) return SECTIONS_NEGATIVE;
    if (q.min_run < 1) return SECTIONS_MIN_RUN;
    if (!act && n_hops > 0) return SECTIONS_NULL_ACT;
    return SECTIONS_OK;
}

// act [n_hops][ACT_Q] -> the sections these hops (and the flush) close, the first `cap` of them into out (any type with the three
// fields of Section; out may be null when cap is 0); returns how many were closed.  The state advances over all n_hops whatever cap is,
// so a caller sizes with cap = 0 on a copy of its state and repeats.  Arguments as sections_check has passed them.
template <class S>
inline int64_t sections_scan(const SectionRule& q, SectionState& st, const double* act, int64_t n_hops, bool flush, S* out, int64_t cap)
{
    int64_t n = 0;
    auto close = [&]() {
        if (st.open_kind == SECTION_NONE) return;
        if (n < cap) { out[n].kind = st.open_kind; out[n].first_hop = st.open_hop; out[n].end_hop = st.hop; }
        ++n;
        st.open_kind = SECTION_NONE;
    };
    for (int64_t i = 0; i < n_hops; ++i) {
        const double db = section_db(act[i * ACT_Q + ACT_RATIO]);
        const double level = section_level(q, act[i * ACT_Q + ACT_LEVEL]);
        if (db > q.dialog_db) {
            if (st.n_background > 0) { st.n_background = 0; close(); }
            ++st.n_dialog;
            if (st.n_dialog >= q.min_run && st.open_kind == SECTION_NONE) { st.open_kind = SECTION_DIALOG; st.open_hop = st.hop; }
        } else if ((db > q.bridge_db || level < q.silence_db) && st.n_dialog >= q.min_run) {
            // the hop belongs to the open section
        } else if (db < q.background_db) {
            if (st.n_dialog > 0) { st.n_dialog = 0; close(); }
            ++st.n_background;
            if (st.n_background >= q.min_run && st.open_kind == SECTION_NONE) { st.open_kind = SECTION_BACKGROUND; st.open_hop = st.hop; }
        } else {
            st.n_dialog = st.n_background = 0;
            close();
        }
        ++st.hop;
    }
    if (flush) close();
    return n;
}

}  // namespace bsrnn
