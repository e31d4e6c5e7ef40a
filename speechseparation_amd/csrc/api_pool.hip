// C ABI of libbsrnn_hip.so, the native session pool (bsrnn_pool_*): one wide bsrnn_stream, a FIFO row per stream row and, for sessions
// at their own sample rates, two resampler banks.  Context and shared helpers: api_internal.h / api.hip.
#include "api_internal.h"
#include "pool_rates_host.h"

extern "C" {

// --------------------------------------------------------------------------- the native session pool
// Slots, pending counts and the round plan: pool_host.h; the two copy kernels: pool.hip.  A pool owns ONE wide bsrnn_stream and, on the
// device, the two rectangles of its hops calls, a FIFO row per stream row and the table block; per round of a feed it uploads the
// table, launches the gather, makes one bsrnn_stream_process_hops and launches the scatter, all on the caller's stream.
struct bsrnn_pool {
    bsrnn_ctx* ctx = nullptr;
    bsrnn_stream* st = nullptr;
    int slots = 0, rows = 0, C = 0, max_hops = 0;
    PoolSlots sl;
    // One device allocation: [chunk C x max_hops*1024 | out, the same | fifo C x 1024 | staging in C x (max_hops+1)*1024 | staging out
    // C x max_hops*1024].  One pinned allocation: [staging in | staging out].  The table block [C entries, then C wet/dry values] travels
    // through a ring reserved at create: no feed allocates.
    float *base = nullptr, *chunk = nullptr, *out = nullptr, *fifo = nullptr, *d_hin = nullptr, *d_hout = nullptr;
    float *h_in = nullptr, *h_out = nullptr;
    UploadRing tab;
    hipStream_t last = nullptr;        // the stream of the last feed: bsrnn_pool_open resets its rows in that stream's order
    bool reset_queued = false;         // ... and a feed on another stream waits for that stream first
    // a call's scratch, sized at create (no feed allocates)
    std::vector<uint8_t> seen;                                 // [slots]
    std::vector<int32_t> counts;                               // [C]
    struct Span { uintptr_t a, e; int32_t i; };
    std::vector<Span> spans;                                   // [slots]: the input ranges of a call, by start, with a running largest end
    // What the rounds of a call read and write per session of the call ([slots]; filled by its checks): a session at the model's rate
    // brings the caller's pointers and count, a session with a rate its rows of conv_in / conv_out and the count the inbound bank gives
    struct View { const float* in; float* out; int64_t in_stride, out_stride, n; int32_t drop; };
    std::vector<View> view;
    // Sessions at their own sample rates (bsrnn_pool_create_rates; pool_rates_host.h).  bin == null: a pool without.  A second device
    // allocation: [conv_in C x cap_in | conv_out C x cap_out | two tables of C pointers, the bank launches' pointer form].  The pointer
    // tables travel through the tail of a table mirror (ptr_off), once per call that names such a session.
    int n_rates = 0;
    int32_t rate[BANK_PAIRS_MAX] = {};
    int64_t max_block = 0, cap_in = 0, cap_out = 0;
    bsrnn_resampler_bank *bin = nullptr, *bout = nullptr;      // rate -> 44100 and 44100 -> rate, C rows each
    float *conv_base = nullptr, *conv_in = nullptr, *conv_out = nullptr;
    char* d_ptrs = nullptr;
    size_t ptr_off = 0;
    std::vector<int32_t> pair;                                 // [slots]: the session's pair, -1 at the model's rate
    std::vector<int32_t> skip;                                 // [slots]: samples of the stream's delay still to be dropped, 1024 or 0
};

static int64_t pool_row_span_bytes(int rows, int64_t stride, int64_t n) { return n > 0 ? ((int64_t)(rows - 1) * stride + n) * (int64_t)sizeof(float) : 0; }

// ---- sessions with a rate: the two banks' descriptors of a call (host arithmetic, scratch of the banks: nothing of it counts until
// pool_rates_launch)
static void pool_rates_hold_all(bsrnn_pool* pl)
{
    for (bsrnn_resampler_bank* bk : {pl->bin, pl->bout})
        for (int r = 0; r < pl->C; ++r) { bk->desc[r] = bank_row_hold(bk->pos[r]); bk->next[r] = bk->pos[r]; }
}
// The slot's rows take n samples inbound and b outbound
static int pool_rates_describe(bsrnn_pool* pl, const char* who, int i, int32_t slot, int64_t n, int64_t b)
{
    const int k = pl->pair[slot];
    for (int rr = 0; rr < pl->rows; ++rr) {
        const int r = slot * pl->rows + rr;
        if (bank_row_process(pl->bin->q[k], pl->bin->pos[r], n, pl->bin->desc[r], pl->bin->next[r]) != BANK_OK ||
            bank_row_process(pl->bout->q[k], pl->bout->pos[r], b, pl->bout->desc[r], pl->bout->next[r]) != BANK_OK)
            return fail(BSRNN_EARG, "%s: session %d (slot %d): %lld samples at %d Hz are more than its resamplers can still take", who, i, slot,
                        (long long)n, pl->rate[k]);
    }
    return 0;
}
// The pointer tables of a call, through the tail of a table mirror: first [C] then second [C] (entries of rows that do not run are never read)
static int pool_rates_pointers(bsrnn_pool* pl, const float*** first, float*** second, int* k)
{
    char* h = nullptr;
    if (int rc = pl->tab.next(&h, k)) return rc;
    *first = reinterpret_cast<const float**>(h + pl->ptr_off);
    *second = reinterpret_cast<float**>(h + pl->ptr_off) + pl->C;
    std::fill(*first, *first + 2 * (size_t)pl->C, nullptr);
    return 0;
}
static int pool_rates_upload(bsrnn_pool* pl, int k, hipStream_t s)
{
    HIP_TRY(hipMemcpyAsync(pl->d_ptrs, pl->tab.h + (size_t)k * pl->tab.cap + pl->ptr_off, 2 * (size_t)pl->C * sizeof(void*), hipMemcpyHostToDevice, s));
    return pl->tab.record(k, s);
}
// One launch of a bank with the descriptors in its scratch; afterwards its rows stand where the descriptors leave them
static int pool_rates_launch(bsrnn_pool* pl, bsrnn_resampler_bank* bk, const float* in, int64_t in_stride, const float* const* in_rows, float* out,
                             int64_t out_stride, float* const* out_rows, hipStream_t s)
{
    BankLaunch L{bk->pairs, in, in_stride, out, out_stride, bk->carry, bk->cap, (int64_t)pl->C * bk->cap, 0, in_rows, out_rows};
    launch_resample_bank(L, bk->tile, bk->desc.data(), pl->C, s);
    HIP_TRY(hipGetLastError());
    bk->pos.swap(bk->next);
    return 0;
}

// Everything a feed refuses, before any device work; fills n_out[i], *h_max and the sessions' views.  who: the entry point's name.
static int pool_check_feed(bsrnn_pool* pl, const char* who, int32_t n, const int32_t* slots, const float* const* in, const int64_t* in_stride,
                           const int64_t* n_in, float* const* out, const int64_t* out_stride, int64_t* n_out, int64_t* h_max, bool host_form,
                           bool* any_rated)
{
    if (!slots || !in || !in_stride || !n_in || !out || !out_stride || !n_out)
        return fail(BSRNN_EARG, "%s: null argument (the slots, the pointers, strides and counts of both sides and n_out_host are needed)", who);
    if (n > pl->slots) return fail(BSRNN_EARG, "%s: n_sessions = %d, the pool has %d slots", who, n, pl->slots);
    std::fill(pl->seen.begin(), pl->seen.end(), (uint8_t)0);
    *h_max = 0;
    *any_rated = false;
    if (pl->bin) pool_rates_hold_all(pl);
    for (int i = 0; i < n; ++i) {
        const int32_t slot = slots[i];
        if (!pool_slot_is_open(pl->sl, slot)) return fail(BSRNN_EARG, "%s: session %d names slot %d, which is not open", who, i, slot);
        if (pl->seen[slot]) return fail(BSRNN_EARG, "%s: session %d names slot %d, which an earlier session of the call names too", who, i, slot);
        pl->seen[slot] = 1;
        if (n_in[i] < 0 || n_in[i] > (INT64_MAX >> 12))
            return fail(BSRNN_EARG, "%s: session %d (slot %d) brings n_in = %lld samples, need 0 or more", who, i, slot, (long long)n_in[i]);
        if (in_stride[i] < n_in[i])
            return fail(BSRNN_EARG, "%s: session %d (slot %d): in_stride = %lld is below its %lld samples", who, i, slot, (long long)in_stride[i],
                        (long long)n_in[i]);
        if (n_in[i] > 0 && !in[i]) return fail(BSRNN_EARG, "%s: session %d (slot %d) brings %lld samples from a null pointer", who, i, slot, (long long)n_in[i]);
        const int k = pl->pair[slot];
        PoolRateFeed f;
        if (k < 0) {
            f = pool_plain_feed(pl->sl.pending[slot], n_in[i]);
            pl->view[i] = {in[i], out[i], in_stride[i], out_stride[i], n_in[i], 0};
        } else {
            // a session with a rate: its samples count at that rate, the rounds see its rows of the staging rectangles
            if (host_form)
                return fail(BSRNN_EARG, "%s: session %d (slot %d) has a sample rate of its own (%d Hz); the host form serves sessions at the "
                                        "model's rate, feed it with bsrnn_pool_feed", who, i, slot, pl->rate[k]);
            if (n_in[i] > pl->max_block)
                return fail(BSRNN_EARG, "%s: session %d (slot %d) brings n_in = %lld samples at %d Hz, the pool was created for max_block = %lld",
                            who, i, slot, (long long)n_in[i], pl->rate[k], (long long)pl->max_block);
            const int row0 = slot * pl->rows;
            f = pool_rate_feed(pl->bin->q[k], pl->bout->q[k], PoolRateSess{pl->bin->pos[row0], pl->bout->pos[row0], pl->skip[slot]},
                               pl->sl.pending[slot], n_in[i]);
            pl->view[i] = {pl->conv_in + (size_t)row0 * pl->cap_in, pl->conv_out + (size_t)row0 * pl->cap_out, pl->cap_in, pl->cap_out, f.a,
                           f.drop};
            if (int rc = pool_rates_describe(pl, who, i, slot, n_in[i], f.b)) return rc;
            *any_rated = true;
        }
        n_out[i] = f.n_out;
        if (out_stride[i] < n_out[i])
            return fail(BSRNN_EARG, "%s: session %d (slot %d): out_stride = %lld is below the %lld samples it gets", who, i, slot,
                        (long long)out_stride[i], (long long)n_out[i]);
        if (n_out[i] > 0 && !out[i]) return fail(BSRNN_EARG, "%s: session %d (slot %d) gets %lld samples at a null pointer", who, i, slot, (long long)n_out[i]);
        *h_max = std::max(*h_max, f.hops);
    }
    // no output range of the call may share a byte with any input range of the call: inputs by start with a running largest end, then one
    // binary search per output
    pl->spans.clear();
    for (int i = 0; i < n; ++i) {
        const int64_t nb = pool_row_span_bytes(pl->rows, in_stride[i], n_in[i]);
        if (nb) pl->spans.push_back({(uintptr_t)in[i], (uintptr_t)in[i] + (uintptr_t)nb, i});
    }
    std::sort(pl->spans.begin(), pl->spans.end(), [](const bsrnn_pool::Span& x, const bsrnn_pool::Span& y) { return x.a < y.a; });
    for (size_t k = 1; k < pl->spans.size(); ++k)
        if (pl->spans[k].e < pl->spans[k - 1].e) { pl->spans[k].e = pl->spans[k - 1].e; pl->spans[k].i = pl->spans[k - 1].i; }
    for (int i = 0; i < n && !pl->spans.empty(); ++i) {
        const int64_t nb = pool_row_span_bytes(pl->rows, out_stride[i], n_out[i]);
        if (!nb) continue;
        const uintptr_t a = (uintptr_t)out[i], e = a + (uintptr_t)nb;
        // the last input that starts below the output's end; the running end says whether it, or one before it, reaches the output
        size_t lo = 0, hi = pl->spans.size();
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (pl->spans[mid].a < e) lo = mid + 1; else hi = mid; }
        if (lo > 0 && pl->spans[lo - 1].e > a)
            return fail(BSRNN_EARG, "%s: the output of session %d (slot %d) overlaps the input of session %d (slot %d); a later round reads input "
                                    "behind what an earlier one has written, so in place is not offered", who, i, slots[i], pl->spans[lo - 1].i,
                        slots[pl->spans[lo - 1].i]);
    }
    return 0;
}

// The slot's session is on `pair` (-1: at the model's rate) from now on and at the beginning of its audio: host-only, as
// bsrnn_resampler_bank_assign - with no input taken the carries hold no sample a call would read.
static void pool_rates_assign(bsrnn_pool* pl, int slot, int pair)
{
    pl->pair[slot] = pair;
    pl->skip[slot] = pair < 0 ? 0 : POOL_HOP;
    if (!pl->bin) return;
    for (int rr = 0; rr < pl->rows; ++rr) {
        const int r = slot * pl->rows + rr;
        bank_row_assign(pl->bin->pos[r], pair < 0 ? 0 : pair);
        bank_row_assign(pl->bout->pos[r], pair < 0 ? 0 : pair);
    }
}

// One feed behind its argument checks.  host_form: in / out are host pointers; each round's samples go through the pinned staging.
// What the sessions bring and where their hops go: pl->view (a session with a rate: its rows of conv_in and conv_out, and in the round of
// its first hop since open or drain that hop is not handed on).
static int pool_feed_rounds(bsrnn_pool* pl, int32_t n, const int32_t* slots, int64_t h_max, const float* mix_host, float mix, hipStream_t s,
                            bool host_form)
{
    const int C = pl->C, R = pl->rows, mh = pl->max_hops;
    const size_t SI = (size_t)(mh + 1) * POOL_HOP, SO = (size_t)mh * POOL_HOP;      // row strides of the staging blocks
    const int64_t rounds = pool_rounds(h_max, mh);
    char* const d_tab = pl->tab.d;
    float* d_mix = reinterpret_cast<float*>(d_tab + (size_t)C * sizeof(PoolEntry));
    for (int64_t j = 0; j < rounds; ++j) {
        const int L = pool_round_hops(h_max, mh, j);
        char* h = nullptr;
        int k = 0;
        if (int rc = pl->tab.next(&h, &k)) return rc;
        PoolEntry* tab = reinterpret_cast<PoolEntry*>(h);
        float* h_mix = reinterpret_cast<float*>(h + (size_t)C * sizeof(PoolEntry));
        std::fill(pl->counts.begin(), pl->counts.end(), 0);
        if (mix_host) std::fill(h_mix, h_mix + C, 1.0f);
        int n_ent = 0, r_lo = C, r_hi = -1;
        for (int i = 0; i < n; ++i) {
            const int32_t slot = slots[i];
            const bsrnn_pool::View& v = pl->view[i];
            const PoolPart q = pool_part(pl->sl.pending[slot], v.n, mh, j);
            for (int rr = 0; rr < R; ++rr) {
                const int row = slot * R + rr;
                pl->counts[row] = q.hops;
                if (mix_host) h_mix[row] = mix_host[i];
                if (j > 0 && q.hops == 0) continue;         // (done in an earlier round: its rows are held and their rectangle rows never read)
                const float* in_row = v.in ? v.in + (size_t)rr * v.in_stride : nullptr;
                if (!host_form) {
                    PoolEntry e = pool_entry(q, row, in_row, v.out ? v.out + (size_t)rr * v.out_stride : nullptr);
                    if (v.drop && q.hops) {                 // the dropped hop is the first of round 0; what follows moves up by it
                        if (q.out_off == 0) e.out_skip = v.drop;
                        else e.dst -= v.drop;
                    }
                    tab[n_ent++] = e;
                    continue;
                }
                // host form: this round's samples of the row, [for the rectangle | for the FIFO], into the staging row; the entry names its mirror
                float* stage = pl->h_in + (size_t)row * SI;
                if (q.n_in) memcpy(stage, in_row + q.in_off, (size_t)q.n_in * sizeof(float));
                if (q.n_pend) memcpy(stage + q.n_in, in_row + q.pend_src, (size_t)q.n_pend * sizeof(float));
                PoolEntry e = pool_entry(q, row, nullptr, nullptr);
                e.src = pl->d_hin + (size_t)row * SI;
                e.pend_src = e.src + q.n_in;
                e.dst = pl->d_hout + (size_t)row * SO;
                tab[n_ent++] = e;
                if (q.n_in || q.n_pend) { r_lo = std::min(r_lo, row); r_hi = std::max(r_hi, row); }
            }
        }
        if (host_form && r_hi >= r_lo)
            HIP_TRY(hipMemcpyAsync(pl->d_hin + (size_t)r_lo * SI, pl->h_in + (size_t)r_lo * SI, (size_t)(r_hi - r_lo + 1) * SI * sizeof(float),
                                   hipMemcpyHostToDevice, s));
        const size_t bytes = mix_host ? (size_t)C * (sizeof(PoolEntry) + sizeof(float)) : (size_t)std::max(n_ent, 1) * sizeof(PoolEntry);
        HIP_TRY(hipMemcpyAsync(d_tab, h, bytes, hipMemcpyHostToDevice, s));
        if (int rc = pl->tab.record(k, s)) return rc;
        launch_pool_gather(reinterpret_cast<const PoolEntry*>(d_tab), n_ent, pl->chunk, pl->fifo, L, s);
        HIP_TRY(hipGetLastError());
        if (L == 0) continue;                               // nobody has a hop: the feed was this one launch
        // the FIFO has been written; the hops call reads the pool's own rectangle, so a re-run of the range policy consumes nothing twice
        if (int rc = bsrnn_stream_process_hops(pl->st, pl->chunk, pl->out, L, pl->counts.data(), mix_host ? d_mix : nullptr, mix_host ? 1.0f : mix, s))
            return rc;
        launch_pool_scatter(reinterpret_cast<const PoolEntry*>(d_tab), n_ent, pl->out, L, s);
        HIP_TRY(hipGetLastError());
        if (!host_form) continue;
        r_lo = C; r_hi = -1;
        for (int e = 0; e < n_ent; ++e)
            if (tab[e].n_out) { r_lo = std::min(r_lo, (int)tab[e].row); r_hi = std::max(r_hi, (int)tab[e].row); }
        HIP_TRY(hipMemcpyAsync(pl->h_out + (size_t)r_lo * SO, pl->d_hout + (size_t)r_lo * SO, (size_t)(r_hi - r_lo + 1) * SO * sizeof(float),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) {
            const bsrnn_pool::View& v = pl->view[i];
            const PoolPart q = pool_part(pl->sl.pending[slots[i]], v.n, mh, j);
            for (int rr = 0; rr < R && q.hops; ++rr)
                memcpy(v.out + (size_t)rr * v.out_stride + q.out_off, pl->h_out + (size_t)(slots[i] * R + rr) * SO, (size_t)q.hops * POOL_HOP * sizeof(float));
        }
    }
    for (int i = 0; i < n; ++i) {
        pl->sl.pending[slots[i]] = pool_pending_after(pl->sl.pending[slots[i]], pl->view[i].n);
        pl->skip[slots[i]] -= pl->view[i].drop;
    }
    return 0;
}

static int pool_feed(bsrnn_pool* pl, const char* who, int32_t n, const int32_t* slots, const float* const* in, const int64_t* in_stride,
                     const int64_t* n_in, float* const* out, const int64_t* out_stride, int64_t* n_out, const float* mix_host, float mix,
                     hipStream_t s, bool host_form)
{
    if (!pl) return fail(BSRNN_EARG, "%s: null pool", who);
    if (n < 0) return fail(BSRNN_EARG, "%s: n_sessions = %d", who, n);
    if (n == 0) return 0;
    int64_t h_max = 0;
    bool any_rated = false;
    if (int rc = pool_check_feed(pl, who, n, slots, in, in_stride, n_in, out, out_stride, n_out, &h_max, host_form, &any_rated)) return rc;
    bsrnn_ctx* c = pl->ctx;
    if (int rc = check_ready(c)) return rc;
    ENTER_CALL(c, s);
    if (pl->reset_queued && pl->last != s) HIP_TRY(hipStreamSynchronize(pl->last));      // (rows that bsrnn_pool_open reset in another stream's order)
    pl->reset_queued = false;
    pl->last = s;
    if (!host_form && !any_rated) return pool_feed_rounds(pl, n, slots, h_max, mix_host, mix, s, false);
    if (!host_form) {
        // Sessions with a rate are named.  ONE inbound launch: every such session's samples, at its own pointer, to its rows of conv_in
        // at 44.1 kHz; the rounds, which read conv_in and write conv_out for them; ONE outbound launch: conv_out to the sessions' pointers.
        const float** p_in = nullptr;
        float** p_out = nullptr;
        int k = 0;
        if (int rc = pool_rates_pointers(pl, &p_in, &p_out, &k)) return rc;
        for (int i = 0; i < n; ++i) {
            if (pl->pair[slots[i]] < 0) continue;
            for (int rr = 0; rr < pl->rows; ++rr) {
                const int row = slots[i] * pl->rows + rr;
                if (n_in[i] > 0) p_in[row] = in[i] + (size_t)rr * in_stride[i];
                if (n_out[i] > 0) p_out[row] = out[i] + (size_t)rr * out_stride[i];
            }
        }
        if (int rc = pool_rates_upload(pl, k, s)) return rc;
        const float* const* d_in = reinterpret_cast<const float* const*>(pl->d_ptrs);
        float* const* d_out = reinterpret_cast<float* const*>(pl->d_ptrs) + pl->C;
        if (int rc = pool_rates_launch(pl, pl->bin, nullptr, 0, d_in, pl->conv_in, pl->cap_in, nullptr, s)) return rc;
        if (int rc = pool_feed_rounds(pl, n, slots, h_max, mix_host, mix, s, false)) return rc;
        return pool_rates_launch(pl, pl->bout, pl->conv_out, pl->cap_out, nullptr, nullptr, 0, d_out, s);
    }
    // the host form waits for its own kernels anyway, so it repairs a range violation whatever the policy says (as bsrnn_stream_step_host)
    const int keep = c->range_policy;
    c->range_policy = BSRNN_RANGE_EXACT;
    int rc = pool_feed_rounds(pl, n, slots, h_max, mix_host, mix, s, true);
    c->range_policy = keep;
    if (!rc) HIP_TRY(hipStreamSynchronize(s));
    return rc;
}

// rated: the table block's mirrors also carry the two pointer tables of a call that names sessions with a rate
static int pool_create(bsrnn_ctx* c, int32_t slots, int32_t rows_per_session, int32_t max_hops, bool rated, bsrnn_pool** out)
{
    if (!c) return fail(BSRNN_EARG, "bsrnn_pool_create: null context");
    if (!out || slots < 1 || rows_per_session < 1)
        return fail(BSRNN_EARG, "bsrnn_pool_create: need slots >= 1, rows_per_session >= 1 and a place for the object, got %d x %d", slots, rows_per_session);
    if ((int64_t)slots * rows_per_session > STREAM_ROWS_MAX)
        return fail(BSRNN_EARG, "bsrnn_pool_create: %d slots x %d rows is more than BSRNN_STREAM_ROWS_MAX = %d rows", slots, rows_per_session, STREAM_ROWS_MAX);
    if (max_hops < 1 || max_hops > STREAM_HOPS_MAX)
        return fail(BSRNN_EARG, "bsrnn_pool_create: max_hops = %d is outside [1, BSRNN_STREAM_HOPS_MAX = %d]", max_hops, STREAM_HOPS_MAX);
    if (int rc = check_ready(c)) return rc;
    std::unique_ptr<bsrnn_pool> pl(new bsrnn_pool());
    pl->ctx = c; pl->slots = slots; pl->rows = rows_per_session; pl->max_hops = max_hops;
    const int C = pl->C = slots * rows_per_session;
    pool_slots_init(pl->sl, slots);
    pl->seen.assign(slots, 0);
    pl->counts.assign(C, 0);
    pl->spans.reserve(slots);
    pl->view.assign(slots, bsrnn_pool::View{});
    pl->pair.assign(slots, -1);
    pl->skip.assign(slots, 0);
    int rc = bsrnn_stream_create(c, C, &pl->st);
    if (!rc) rc = bsrnn_stream_reserve(pl->st, max_hops);
    if (rc) { if (pl->st) bsrnn_stream_destroy(pl->st); return rc; }
    const size_t rect = (size_t)C * max_hops * POOL_HOP, fifo = (size_t)C * POOL_HOP, stage_in = (size_t)C * (max_hops + 1) * POOL_HOP;
    pl->ptr_off = ((size_t)C * (sizeof(PoolEntry) + sizeof(float)) + 7) & ~size_t(7);
    const size_t tab_bytes = (pl->ptr_off + (rated ? 2 * (size_t)C * sizeof(void*) : 0) + 255) & ~size_t(255);
    const size_t d_bytes = (3 * rect + fifo + stage_in) * sizeof(float), h_bytes = (stage_in + rect) * sizeof(float);
    g_dbg[DBG_ALLOC] += 2;
    hipError_t e = hipMalloc((void**)&pl->base, d_bytes);
    if (e == hipSuccess) e = hipMemset(pl->base, 0, d_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&pl->h_in, h_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = pl->tab.reserve(tab_bytes);
    if (e == hipSuccess) {
        memset(pl->h_in, 0, h_bytes);
        memset(pl->tab.h, 0, UploadRing::MIRRORS * tab_bytes);
        float* p = pl->base;
        pl->chunk = p; p += rect;
        pl->out = p; p += rect;
        pl->fifo = p; p += fifo;
        pl->d_hin = p; p += stage_in;
        pl->d_hout = p; p += rect;
        pl->h_out = pl->h_in + stage_in;
        // the two kernels' first launches happen here: every row as an empty entry, which zero-fills the rectangle and moves nothing
        PoolEntry* tab = reinterpret_cast<PoolEntry*>(pl->tab.h);
        for (int r = 0; r < C; ++r) tab[r] = pool_entry(PoolPart{}, r, nullptr, nullptr);
        e = hipMemcpy(pl->tab.d, pl->tab.h, tab_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            launch_pool_gather(reinterpret_cast<const PoolEntry*>(pl->tab.d), C, pl->chunk, pl->fifo, max_hops, nullptr);
            launch_pool_scatter(reinterpret_cast<const PoolEntry*>(pl->tab.d), C, pl->out, max_hops, nullptr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        bsrnn_pool_destroy(pl.release());
        return fail(BSRNN_EHIP, "bsrnn_pool_create: %s", hipGetErrorString(e));
    }
    *out = pl.release();
    return 0;
}

int bsrnn_pool_create(bsrnn_ctx* c, int32_t slots, int32_t rows_per_session, int32_t max_hops, bsrnn_pool** out)
{
    return pool_create(c, slots, rows_per_session, max_hops, false, out);
}

void bsrnn_pool_destroy(bsrnn_pool* pl)
{
    if (!pl) return;
    (void)hipSetDevice(pl->ctx->device);
    (void)hipDeviceSynchronize();
    if (pl->conv_base) (void)hipFree(pl->conv_base);
    if (pl->bin) bsrnn_resampler_bank_destroy(pl->bin);
    if (pl->bout) bsrnn_resampler_bank_destroy(pl->bout);
    pl->tab.release();
    if (pl->h_in) (void)hipHostFree(pl->h_in);
    if (pl->base) (void)hipFree(pl->base);
    bsrnn_stream* st = pl->st;
    delete pl;
    bsrnn_stream_destroy(st);          // (last: a context that bsrnn_destroy retired goes with its last stream)
}

// pair: the session's rate pair, -1 at the model's rate
static int pool_open(bsrnn_pool* pl, int pair, int32_t* slot_out)
{
    for (int i = 0; i < pl->slots; ++i) {
        if (pl->sl.open[i]) continue;
        // the slot's rows start from silence, in the order of the stream the pool was last fed on; the FIFO needs nothing (pending 0: unread)
        for (int r = 0; r < pl->rows; ++r) pl->counts[r] = i * pl->rows + r;
        if (int rc = bsrnn_stream_reset_rows(pl->st, pl->counts.data(), pl->rows, pl->last)) return rc;
        pl->reset_queued = true;
        *slot_out = pool_slot_open(pl->sl);
        pool_rates_assign(pl, i, pair);
        return 0;
    }
    return fail(BSRNN_EARG, "bsrnn_pool_open: all %d slots are in use", pl->slots);
}

int bsrnn_pool_open(bsrnn_pool* pl, int32_t* slot_out)
{
    if (!pl || !slot_out) return fail(BSRNN_EARG, "bsrnn_pool_open: null %s", !pl ? "pool" : "slot_out");
    return pool_open(pl, -1, slot_out);
}

int bsrnn_pool_close(bsrnn_pool* pl, int32_t slot)
{
    if (!pl) return fail(BSRNN_EARG, "bsrnn_pool_close: null pool");
    if (!pool_slot_close(pl->sl, slot)) return fail(BSRNN_EARG, "bsrnn_pool_close: slot %d is not open", slot);
    pool_rates_assign(pl, slot, -1);
    return 0;
}

int64_t bsrnn_pool_pending(const bsrnn_pool* pl, int32_t slot) { return pl && pool_slot_is_open(pl->sl, slot) ? pl->sl.pending[slot] : -1; }

bsrnn_stream* bsrnn_pool_stream(bsrnn_pool* pl) { return pl ? pl->st : nullptr; }

int bsrnn_pool_get_pending(bsrnn_pool* pl, int32_t slot, float* host, int32_t* n)
{
    if (!pl || !host || !n) return fail(BSRNN_EARG, "bsrnn_pool_get_pending: null %s", !pl ? "pool" : "argument");
    if (!pool_slot_is_open(pl->sl, slot)) return fail(BSRNN_EARG, "bsrnn_pool_get_pending: slot %d is not open", slot);
    HIP_TRY(hipSetDevice(pl->ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, pl->fifo + (size_t)slot * pl->rows * POOL_HOP, (size_t)pl->rows * POOL_HOP * sizeof(float), hipMemcpyDeviceToHost));
    *n = pl->sl.pending[slot];
    return 0;
}

int bsrnn_pool_set_pending(bsrnn_pool* pl, int32_t slot, const float* host, int32_t n)
{
    if (!pl || !host) return fail(BSRNN_EARG, "bsrnn_pool_set_pending: null %s", !pl ? "pool" : "argument");
    if (!pool_slot_is_open(pl->sl, slot)) return fail(BSRNN_EARG, "bsrnn_pool_set_pending: slot %d is not open", slot);
    if (n < 0 || n >= POOL_HOP) return fail(BSRNN_EARG, "bsrnn_pool_set_pending: n = %d samples, a session has fewer than %d waiting", n, POOL_HOP);
    HIP_TRY(hipSetDevice(pl->ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(pl->fifo + (size_t)slot * pl->rows * POOL_HOP, host, (size_t)pl->rows * POOL_HOP * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    pl->sl.pending[slot] = n;
    return 0;
}

int bsrnn_pool_feed(bsrnn_pool* pl, int32_t n_sessions, const int32_t* slots_host, const float* const* in_dev, const int64_t* in_stride,
                    const int64_t* n_in, float* const* out_dev, const int64_t* out_stride, int64_t* n_out_host, const float* mix_host, float mix,
                    void* stream)
{
    return pool_feed(pl, "bsrnn_pool_feed", n_sessions, slots_host, in_dev, in_stride, n_in, out_dev, out_stride, n_out_host, mix_host, mix,
                     (hipStream_t)stream, false);
}

int bsrnn_pool_feed_host(bsrnn_pool* pl, int32_t n_sessions, const int32_t* slots_host, const float* const* in_host, const int64_t* in_stride,
                         const int64_t* n_in, float* const* out_host, const int64_t* out_stride, int64_t* n_out_host, const float* mix_host,
                         float mix)
{
    return pool_feed(pl, "bsrnn_pool_feed_host", n_sessions, slots_host, in_host, in_stride, n_in, out_host, out_stride, n_out_host, mix_host, mix,
                     nullptr, true);
}

// ---- sessions at their own sample rates (pool_rates_host.h)
int bsrnn_pool_create_rates(bsrnn_ctx* c, int32_t slots, int32_t rows_per_session, int32_t max_hops, const int32_t* rates, int32_t n_rates,
                            int64_t max_block, bsrnn_pool** out)
{
    if (!c) return fail(BSRNN_EARG, "bsrnn_pool_create_rates: null context");
    if (!out) return fail(BSRNN_EARG, "bsrnn_pool_create_rates: null place for the object");
    if (n_rates < 1 || n_rates > BANK_PAIRS_MAX)
        return fail(BSRNN_EARG, "bsrnn_pool_create_rates: n_rates = %d is outside [1, BSRNN_BANK_PAIRS_MAX = %d]", n_rates, BANK_PAIRS_MAX);
    if (!rates) return fail(BSRNN_EARG, "bsrnn_pool_create_rates: null list of the %d rates", n_rates);
    int32_t model[BANK_PAIRS_MAX];
    ResampleRatio qin[BANK_PAIRS_MAX];
    for (int k = 0; k < n_rates; ++k) {
        model[k] = POOL_MODEL_RATE;
        ResampleRatio q;
        if (int rc = resample_check_rates(rates[k], POOL_MODEL_RATE, "bsrnn_pool_create_rates", qin[k])) return rc;
        if (int rc = resample_check_rates(POOL_MODEL_RATE, rates[k], "bsrnn_pool_create_rates", q)) return rc;
    }
    if (max_block < 1 || max_block > ((int64_t)1 << 24))
        return fail(BSRNN_EARG, "bsrnn_pool_create_rates: max_block = %lld samples is outside [1, 2^24]", (long long)max_block);
    bsrnn_pool* pl = nullptr;
    if (int rc = pool_create(c, slots, rows_per_session, max_hops, true, &pl)) return rc;
    const int C = pl->C;
    pl->n_rates = n_rates;
    for (int k = 0; k < n_rates; ++k) pl->rate[k] = rates[k];
    pl->max_block = max_block;
    pl->cap_in = pool_rates_cap_in(qin, n_rates, max_block);
    pl->cap_out = pool_rates_cap_out(pl->cap_in);
    int rc = bsrnn_resampler_bank_create(c, C, rates, model, n_rates, &pl->bin);
    if (!rc) rc = bsrnn_resampler_bank_create(c, C, model, rates, n_rates, &pl->bout);
    if (!rc) {
        const size_t floats = (size_t)C * (pl->cap_in + pl->cap_out), bytes = floats * sizeof(float) + 2 * (size_t)C * sizeof(void*);
        ++g_dbg[DBG_ALLOC];
        hipError_t e = hipMalloc((void**)&pl->conv_base, bytes);
        if (e == hipSuccess) e = hipMemset(pl->conv_base, 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail(BSRNN_EHIP, "bsrnn_pool_create_rates: %s", hipGetErrorString(e));
        pl->conv_in = pl->conv_base;
        pl->conv_out = pl->conv_in + (size_t)C * pl->cap_in;
        pl->d_ptrs = reinterpret_cast<char*>(pl->conv_out + (size_t)C * pl->cap_out);
    }
    if (rc) { bsrnn_pool_destroy(pl); return rc; }
    *out = pl;
    return 0;
}

int bsrnn_pool_open_rate(bsrnn_pool* pl, int32_t sample_rate, int32_t* slot_out)
{
    if (!pl || !slot_out) return fail(BSRNN_EARG, "bsrnn_pool_open_rate: null %s", !pl ? "pool" : "slot_out");
    if (sample_rate == POOL_MODEL_RATE) return pool_open(pl, -1, slot_out);
    for (int k = 0; k < pl->n_rates; ++k)
        if (pl->rate[k] == sample_rate) return pool_open(pl, k, slot_out);
    return fail(BSRNN_EARG, "bsrnn_pool_open_rate: sample_rate %d is not one of the %d rates the pool was created with", sample_rate, pl->n_rates);
}

int32_t bsrnn_pool_rate_of(const bsrnn_pool* pl, int32_t slot)
{
    if (!pl || !pool_slot_is_open(pl->sl, slot)) return -1;
    return pl->pair[slot] < 0 ? POOL_MODEL_RATE : pl->rate[pl->pair[slot]];
}

static PoolRateSess pool_rate_sess(const bsrnn_pool* pl, int32_t slot)
{
    const int row0 = slot * pl->rows;
    return PoolRateSess{pl->bin->pos[row0], pl->bout->pos[row0], pl->skip[slot]};
}

int64_t bsrnn_pool_ready(const bsrnn_pool* pl, int32_t slot, int64_t n_in)
{
    if (!pl || !pool_slot_is_open(pl->sl, slot) || n_in < 0 || n_in > (INT64_MAX >> 12)) return -1;
    const int k = pl->pair[slot];
    if (k < 0) return pool_plain_feed(pl->sl.pending[slot], n_in).n_out;
    if (n_in > pl->max_block) return -1;
    return pool_rate_feed(pl->bin->q[k], pl->bout->q[k], pool_rate_sess(pl, slot), pl->sl.pending[slot], n_in).n_out;
}

static PoolRateDrain pool_drain_plan(const bsrnn_pool* pl, int32_t slot)
{
    const int k = pl->pair[slot];
    return k < 0 ? pool_plain_drain(pl->sl.pending[slot])
                 : pool_rate_drain(pl->bin->q[k], pl->bout->q[k], pool_rate_sess(pl, slot), pl->sl.pending[slot]);
}

int64_t bsrnn_pool_drain_len(const bsrnn_pool* pl, int32_t slot)
{
    if (!pl || !pool_slot_is_open(pl->sl, slot)) return -1;
    return pool_drain_plan(pl, slot).n_out;
}

int bsrnn_pool_drain(bsrnn_pool* pl, int32_t slot, float* out, int64_t out_stride, int64_t* n_out_host, float mix, void* stream)
{
    if (!pl) return fail(BSRNN_EARG, "bsrnn_pool_drain: null pool");
    if (!n_out_host) return fail(BSRNN_EARG, "bsrnn_pool_drain: session in slot %d: nowhere to report the sample count (null n_out_host)", slot);
    if (!pool_slot_is_open(pl->sl, slot)) return fail(BSRNN_EARG, "bsrnn_pool_drain: session in slot %d: the slot is not open", slot);
    const int k = pl->pair[slot], R = pl->rows, C = pl->C, row0 = slot * R;
    const PoolRateDrain g = pool_drain_plan(pl, slot);
    if (out_stride < g.n_out)
        return fail(BSRNN_EARG, "bsrnn_pool_drain: session in slot %d: out_stride = %lld is below the %lld samples it gets", slot,
                    (long long)out_stride, (long long)g.n_out);
    if (g.n_out > 0 && !out) return fail(BSRNN_EARG, "bsrnn_pool_drain: session in slot %d gets %lld samples at a null pointer", slot, (long long)g.n_out);
    bsrnn_ctx* c = pl->ctx;
    if (int rc = check_ready(c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ENTER_CALL(c, s);
    if (pl->reset_queued && pl->last != s) HIP_TRY(hipStreamSynchronize(pl->last));
    pl->reset_queued = false;
    pl->last = s;
    const size_t SI = (size_t)(pl->max_hops + 1) * POOL_HOP;
    const size_t zeros = (size_t)(g.pad + POOL_HOP) * sizeof(float);
    float* const* d_first = reinterpret_cast<float* const*>(pl->d_ptrs);
    float* const* d_second = d_first + C;
    if (k < 0) {
        // at the model's rate: the zeros come from the slot's rows of the host form's device staging (pad + 1024 <= 2047 floats of a row)
        float* z = pl->d_hin + (size_t)row0 * SI;
        HIP_TRY(hipMemset2DAsync(z, SI * sizeof(float), 0, zeros, R, s));
        pl->view[0] = {z, out, (int64_t)SI, out_stride, g.n_feed, 0};
    } else {
        // both pointer tables of the outbound launches go up at once: where the flush writes (behind the n1 samples), where the process does
        const float** p_flush = nullptr;
        float** p_proc = nullptr;
        int m = 0;
        if (int rc = pool_rates_pointers(pl, &p_flush, &p_proc, &m)) return rc;
        for (int rr = 0; rr < R; ++rr) {
            p_proc[row0 + rr] = out ? out + (size_t)rr * out_stride : nullptr;
            p_flush[row0 + rr] = out ? out + (size_t)rr * out_stride + g.n1 : nullptr;
        }
        if (int rc = pool_rates_upload(pl, m, s)) return rc;
        // 1. the inbound rows are flushed into conv_in; 2. and 3. zeros to a whole hop and one more hop behind them
        pool_rates_hold_all(pl);
        for (int r = row0; r < row0 + R; ++r)
            if (bank_row_flush(pl->bin->q[k], pl->bin->pos[r], pl->bin->desc[r], pl->bin->next[r]) != BANK_OK)
                return fail(BSRNN_ESTATE, "bsrnn_pool_drain: session in slot %d: the inbound flush is too long (internal error)", slot);
        if (int rc = pool_rates_launch(pl, pl->bin, nullptr, 0, nullptr, pl->conv_in, pl->cap_in, nullptr, s)) return rc;
        float* x = pl->conv_in + (size_t)row0 * pl->cap_in;
        HIP_TRY(hipMemset2DAsync(x + g.owed_in, (size_t)pl->cap_in * sizeof(float), 0, zeros, R, s));
        pl->view[0] = {x, pl->conv_out + (size_t)row0 * pl->cap_out, pl->cap_in, pl->cap_out, g.n_feed, g.drop};
    }
    // 4. those hops, every other session held
    if (int rc = pool_feed_rounds(pl, 1, &slot, g.hops, nullptr, mix, s, false)) return rc;
    if (k >= 0) {
        // 5. the outbound rows take them, and are flushed
        pool_rates_hold_all(pl);
        for (int r = row0; r < row0 + R; ++r)
            if (bank_row_process(pl->bout->q[k], pl->bout->pos[r], g.b, pl->bout->desc[r], pl->bout->next[r]) != BANK_OK)
                return fail(BSRNN_ESTATE, "bsrnn_pool_drain: session in slot %d: the outbound block is too long (internal error)", slot);
        if (int rc = pool_rates_launch(pl, pl->bout, pl->conv_out, pl->cap_out, nullptr, nullptr, 0, d_second, s)) return rc;
        pool_rates_hold_all(pl);
        for (int r = row0; r < row0 + R; ++r)
            if (bank_row_flush(pl->bout->q[k], pl->bout->pos[r], pl->bout->desc[r], pl->bout->next[r]) != BANK_OK)
                return fail(BSRNN_ESTATE, "bsrnn_pool_drain: session in slot %d: the outbound flush is too long (internal error)", slot);
        if (int rc = pool_rates_launch(pl, pl->bout, nullptr, 0, nullptr, nullptr, 0, d_first, s)) return rc;
    }
    // the session stands at the beginning of a new piece of audio: its stream rows in this stream's order, the rest is host state
    for (int rr = 0; rr < R; ++rr) pl->counts[rr] = row0 + rr;
    if (int rc = bsrnn_stream_reset_rows(pl->st, pl->counts.data(), R, s)) return rc;
    pool_rates_assign(pl, slot, k);
    pl->sl.pending[slot] = 0;
    *n_out_host = g.n_out;
    return 0;
}

}  // extern "C"
