// Asks speechseparation_amd/csrc/critic_ragged_host.h (compiled alone, no HIP) what tests/test_critic_ragged_host.py checks; prints JSON.
// A batch is given as: I Tmax order n_clips frames_0 rows_0 frames_1 rows_1 ...   (R is the sum of the rows unless given)
//   critic_ragged_check rows  BATCH          -> per row: frames, clip, the chain, the live tiles of the two kernels; and what a walk of
//                                               the two kernels' workgroups covers, reads and writes, as counts of violations
//   critic_ragged_check plan  BATCH          -> the CrgPlan
//   critic_ragged_check why   R grad BATCH   -> {"why": n, "clip": c}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "critic_ragged_host.h"

using namespace bsrnn;

struct Batch { int I, Tmax, order, n_clips, R; std::vector<int32_t> frames, rows; };

static bool parse(int argc, char** argv, int at, Batch* b)
{
    if (argc < at + 4) return false;
    b->I = atoi(argv[at]); b->Tmax = atoi(argv[at + 1]); b->order = atoi(argv[at + 2]); b->n_clips = atoi(argv[at + 3]);
    b->R = 0;
    for (int c = 0; c < b->n_clips; ++c) {
        if (argc < at + 6 + 2 * c) return false;
        b->frames.push_back(atoi(argv[at + 4 + 2 * c]));
        b->rows.push_back(atoi(argv[at + 5 + 2 * c]));
        b->R += b->rows.back();
    }
    return true;
}

int main(int argc, char** argv)
{
    Batch b;
    if (argc >= 2 && !strcmp(argv[1], "rows") && parse(argc, argv, 2, &b)) {
        const CrgPlan p = crg_plan(b.I, b.R, b.Tmax, b.n_clips);
        const CscPlan& f = p.g.f;
        std::vector<CrgRow> rows(b.R);
        std::vector<CrgClip> clips(b.n_clips);
        crg_tables(b.frames.data(), b.rows.data(), b.n_clips, rows.data(), clips.data());
        long long cover_wrong = 0, dead_covers = 0, reads_behind = 0, writers_wrong = 0, nonzero_behind = 0, reach_wrong = 0, fwd_reach_wrong = 0,
                  clip_wrong = 0;
        int64_t live_fwd = 0, live_dx = 0;
        printf("{\"rows\": [");
        for (int r = 0; r < b.R; ++r) {
            const int Tr = rows[r].frames;
            int len[CRITIC_LAYERS];
            critic_chain(Tr, len);
            const CrgClip& cl = clips[rows[r].clip];
            if (r < cl.row0 || r >= cl.row0 + cl.rows || cl.frames != Tr) ++clip_wrong;
            if (crg_t_out(Tr) != len[0] || crg_t4(Tr) != len[3]) ++clip_wrong;
            // the forward as the kernel walks it: a live tile stages frame t when t < T1_r and then reads x[3 t .. 3 t + 15]
            std::vector<int> covered(f.len[0], 0);
            printf("%s{\"frames\": %d, \"clip\": %d, \"chain\": [%d, %d, %d, %d], \"fwd_live\": [", r ? ", " : "", Tr, rows[r].clip, len[0], len[1],
                   len[2], len[3]);
            bool first = true;
            for (int bt = 0; bt < f.t_tiles; ++bt) {
                if (!crg_fwd_tile_live(Tr, bt)) continue;
                printf("%s%d", first ? "" : ", ", bt); first = false;
                ++live_fwd;
                for (int t = bt * CSC_TILE_T; t < (bt + 1) * CSC_TILE_T; ++t) {
                    if (t >= crg_t_out(Tr)) continue;
                    if (t >= f.len[0]) { ++dead_covers; continue; }
                    ++covered[t];
                    if (CRITIC_STRIDE * t + CRITIC_TAPS - 1 >= Tr) ++reads_behind;
                }
            }
            for (int t = 0; t < f.len[0]; ++t) if (covered[t] != (t < len[0] ? 1 : 0)) ++cover_wrong;
            // the dx kernel: every (i, s < Tmax) of the row has one writer; a dead tile and the positions behind the row's frames get zeros
            printf("], \"dx_live\": [");
            first = true;
            std::vector<int> writers((size_t)b.I * b.Tmax, 0);
            for (int bs = 0; bs < p.g.s_tiles; ++bs) {
                const bool live = crg_dx_tile_live(Tr, bs);
                if (live) { printf("%s%d", first ? "" : ", ", bs); first = false; ++live_dx; }
                for (int bi = 0; bi < p.g.i_tiles; ++bi)
                    for (int ch = 0; ch < CGD_CH; ++ch)
                        for (int d = 0; d < CGD_TILE_S; ++d) {
                            const int i = bi * CGD_CH + ch, s = cgd_tile_first(bs) + d;
                            if (i >= b.I || s >= b.Tmax) continue;
                            ++writers[(size_t)csc_channel_row(b.I, i, b.order) * b.Tmax + s];
                            if (!live && s < Tr) ++nonzero_behind;          // a dead tile writes zeros: it must own no position of the row's frames
                        }
            }
            for (size_t v = 0; v < writers.size(); ++v) if (writers[v] != 1) ++writers_wrong;
            printf("]}");
            // the zero-propagation argument, layers 4 .. 2 (and the first): a position s >= len_r of a layer's input collects only frames
            // >= T_out_r of its output; and a frame t < T_out_r reads positions below len_r only
            int in_r = Tr, in_max = b.Tmax;
            for (int l = 0; l < CRITIC_LAYERS; ++l) {
                const int out_r = len[l], out_max = f.len[l];
                for (int s = in_r; s < in_max; ++s)
                    for (int k = 0; k < CRITIC_TAPS; ++k) {
                        if (s - k < 0 || (s - k) % CRITIC_STRIDE) continue;
                        const int t = (s - k) / CRITIC_STRIDE;
                        if (t < out_max && t < out_r) ++reach_wrong;
                    }
                for (int t = 0; t < out_r; ++t) if (CRITIC_STRIDE * t + CRITIC_TAPS - 1 >= in_r) ++fwd_reach_wrong;
                in_r = out_r; in_max = out_max;
            }
        }
        int64_t lf = 0, ld = 0;
        crg_live_tiles(p, b.frames.data(), b.rows.data(), &lf, &ld);
        printf("], \"t_tiles\": %d, \"s_tiles\": %d, \"live_fwd\": %lld, \"live_dx\": %lld, \"live_fwd_reported\": %lld, \"live_dx_reported\": %lld, "
               "\"cover_wrong\": %lld, \"dead_covers\": %lld, \"reads_behind\": %lld, \"writers_wrong\": %lld, \"nonzero_behind\": %lld, "
               "\"reach_wrong\": %lld, \"fwd_reach_wrong\": %lld, \"clip_wrong\": %lld}\n",
               f.t_tiles, p.g.s_tiles, (long long)live_fwd, (long long)live_dx, (long long)lf, (long long)ld, cover_wrong, dead_covers, reads_behind,
               writers_wrong, nonzero_behind, reach_wrong, fwd_reach_wrong, clip_wrong);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "plan") && parse(argc, argv, 2, &b)) {
        const CrgPlan p = crg_plan(b.I, b.R, b.Tmax, b.n_clips);
        const CscPlan ref = csc_plan(b.I, b.R, b.Tmax);
        printf("{\"len\": [%d, %d, %d, %d], \"slabs\": %d, \"ch_per_slab\": %d, \"rect_slabs\": %d, \"rect_ch_per_slab\": %d, "
               "\"off_y\": [%lld, %lld, %lld, %lld], \"off_shared\": %lld, \"fwd_ws\": %lld, \"fwd_ws_exact\": %lld, "
               "\"off_dp\": [%lld, %lld, %lld, %lld], \"off_pool\": %lld, \"off_max\": %lld, \"ws\": %lld, \"off_xp\": %lld, \"off_dxp\": %lld, "
               "\"ws_exact\": %lld, \"table_bytes\": %lld, \"row_bytes\": %d, \"clip_bytes\": %d}\n",
               p.g.f.len[0], p.g.f.len[1], p.g.f.len[2], p.g.f.len[3], p.g.f.slabs, p.g.f.ch_per_slab, ref.slabs, ref.ch_per_slab,
               (long long)p.g.f.off_y[0], (long long)p.g.f.off_y[1], (long long)p.g.f.off_y[2], (long long)p.g.f.off_y[3], (long long)p.g.f.off_shared,
               (long long)p.g.f.ws_floats, (long long)p.g.f.ws_exact_floats, (long long)p.g.off_dp[0], (long long)p.g.off_dp[1],
               (long long)p.g.off_dp[2], (long long)p.g.off_dp[3], (long long)p.off_pool, (long long)p.off_max, (long long)p.ws_floats,
               (long long)p.off_xp, (long long)p.off_dxp, (long long)p.ws_exact_floats, (long long)p.table_bytes, (int)sizeof(CrgRow),
               (int)sizeof(CrgClip));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "why") && parse(argc, argv, 4, &b)) {
        int bad = -1;
        const int why = crg_check(b.I, atoll(argv[2]), b.Tmax, b.frames.data(), b.rows.data(), b.n_clips, b.order, atoi(argv[3]) != 0, &bad);
        printf("{\"why\": %d, \"clip\": %d}\n", why, bad);
        return 0;
    }
    fprintf(stderr, "usage: critic_ragged_check rows BATCH | plan BATCH | why R grad BATCH     BATCH = I Tmax order n_clips (frames rows)...\n");
    return 2;
}
