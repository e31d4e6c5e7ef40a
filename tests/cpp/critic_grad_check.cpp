// Asks speechseparation_amd/csrc/critic_grad_host.h (compiled alone, no HIP) what tests/test_critic_grad_host.py checks; prints JSON.
//   critic_grad_check image I         -> the bijection check of the dx image's index map, done here
//   critic_grad_check tiles I C T     -> ownership of every (c, i, s), the fold's frame sets against the definition, the row map: counts
//   critic_grad_check plan I C T      -> the CgdPlan
//   critic_grad_check why I C T order -> {"why": n}
//   critic_grad_check scale BITS      -> {"e": n}: the exponent for a maximum with these bits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "critic_grad_host.h"

using namespace bsrnn;

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "image")) {
        const int I = atoi(argv[2]);
        const int64_t n = cgd_image_halves(I);
        std::vector<unsigned char> hit((size_t)n, 0);
        long long twice = 0, out_of_range = 0, inverse_wrong = 0, padding_hit = 0, padding = 0, unaligned = 0;
        for (int o = 0; o < CSC_O; ++o)
            for (int i = 0; i < I; ++i)
                for (int k = 0; k < CRITIC_TAPS; ++k)
                    for (int pc = 0; pc < 2; ++pc) {
                        const int64_t p = cgd_image_index(I, o, i, k, pc);
                        if (p < 0 || p >= n) { ++out_of_range; continue; }
                        if (hit[(size_t)p]++) ++twice;
                        int o2, i2, k2, pc2;
                        if (!cgd_image_source(I, p, &o2, &i2, &k2, &pc2) || o2 != o || i2 != i || k2 != k || pc2 != pc) ++inverse_wrong;
                        if (o % 8 == 0 && p % 8 != 0) ++unaligned;          // the eight output channels of a lane are one aligned 16-byte unit
                        if (o % 8 && p != cgd_image_index(I, o - 1, i, k, pc) + 1) ++unaligned;
                    }
        for (int64_t p = 0; p < n; ++p)
            if (!hit[(size_t)p]) {
                int o2, i2, k2, pc2;
                ++padding;
                if (cgd_image_source(I, p, &o2, &i2, &k2, &pc2)) ++padding_hit;      // a position nobody maps to must read as padding (zero)
            }
        printf("{\"halves\": %lld, \"i_pad\": %d, \"block\": %d, \"twice\": %lld, \"out_of_range\": %lld, \"inverse_wrong\": %lld, "
               "\"padding\": %lld, \"padding_not_zero\": %lld, \"unaligned\": %lld}\n",
               (long long)n, cgd_i_pad(I), CSC_BLOCK, twice, out_of_range, inverse_wrong, padding, padding_hit, unaligned);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "tiles")) {
        const int I = atoi(argv[2]), C = atoi(argv[3]), T = atoi(argv[4]);
        const CgdPlan g = cgd_plan(I, C, T);
        const int T1 = g.f.len[0];
        // every (c, i, s) is written by exactly one (row, channel tile, position tile): walk the tiles as the kernel does
        std::vector<unsigned char> owner((size_t)C * I * T, 0);
        long long twice = 0, fold_wrong = 0, column_outside = 0, tile_of_wrong = 0, row_twice = 0;
        for (int rmap = 0; rmap < 2; ++rmap) {
            if (rmap && I % 2) break;
            std::fill(owner.begin(), owner.end(), 0);
            for (int c = 0; c < C; ++c)
                for (int bi = 0; bi < g.i_tiles; ++bi)
                    for (int bs = 0; bs < g.s_tiles; ++bs)
                        for (int ch = 0; ch < CGD_CH; ++ch)
                            for (int d = 0; d < CGD_TILE_S; ++d) {
                                const int i = bi * CGD_CH + ch, s = cgd_tile_first(bs) + d;
                                if (i >= I || s >= T) continue;
                                if (cgd_tile_of(s) != bs) ++tile_of_wrong;
                                if (owner[((size_t)c * I + csc_channel_row(I, i, rmap)) * T + s]++) ++twice;
                            }
            for (size_t v = 0; v < owner.size(); ++v) if (owner[v] != 1) ++row_twice;
        }
        // the fold of position s: the (tap, frame) pairs it adds, in order, against the definition of include/bsrnn_hip.h:
        // the taps k with (s - k) % 3 == 0 and 0 <= (s - k) / 3 < T1, ascending; pairs with a frame outside [0, T1) add a zero
        for (int s = 0; s < T; ++s) {
            const int bs = cgd_tile_of(s), d = s - cgd_tile_first(bs), f0 = cgd_tile_frame0(bs);
            std::vector<int> got, want;
            for (int k = d % CRITIC_STRIDE; k < CRITIC_TAPS; k += CRITIC_STRIDE) {
                const int col = cgd_fold_column(d, k), t = f0 + col;
                if (col < 0 || col >= CGD_TILE_T) ++column_outside;
                if (t >= 0 && t < T1) { got.push_back(k); got.push_back(t); }
            }
            for (int k = 0; k < CRITIC_TAPS; ++k)
                if (s - k >= 0 && (s - k) % CRITIC_STRIDE == 0 && (s - k) / CRITIC_STRIDE < T1) { want.push_back(k); want.push_back((s - k) / CRITIC_STRIDE); }
            if (got != want) ++fold_wrong;
        }
        printf("{\"i_tiles\": %d, \"s_tiles\": %d, \"twice\": %lld, \"not_once\": %lld, \"tile_of_wrong\": %lld, \"fold_wrong\": %lld, "
               "\"column_outside\": %lld}\n", g.i_tiles, g.s_tiles, twice, row_twice, tile_of_wrong, fold_wrong, column_outside);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "plan")) {
        const int I = atoi(argv[2]), C = atoi(argv[3]), T = atoi(argv[4]);
        const CgdPlan g = cgd_plan(I, C, T);
        printf("{\"len\": [%d, %d, %d, %d], \"i_tiles\": %d, \"s_tiles\": %d, \"ch\": %d, \"tile_s\": %d, \"tile_t\": %d, \"halo\": %d, "
               "\"fwd_ws\": %lld, \"off_shared\": %lld, \"off_dp\": [%lld, %lld, %lld, %lld], \"off_pool\": %lld, \"off_max\": %lld, \"ws\": %lld, "
               "\"off_xp\": %lld, \"off_dxp\": %lld, \"ws_exact\": %lld, \"image_halves\": %lld}\n",
               g.f.len[0], g.f.len[1], g.f.len[2], g.f.len[3], g.i_tiles, g.s_tiles, CGD_CH, CGD_TILE_S, CGD_TILE_T, CGD_HALO,
               (long long)g.f.ws_floats, (long long)g.f.off_shared, (long long)g.off_dp[0], (long long)g.off_dp[1], (long long)g.off_dp[2],
               (long long)g.off_dp[3], (long long)g.off_pool, (long long)g.off_max, (long long)g.ws_floats, (long long)g.off_xp,
               (long long)g.off_dxp, (long long)g.ws_exact_floats, (long long)cgd_image_halves(I));
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "why")) {
        printf("{\"why\": %d}\n", cgd_check(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5])));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "scale")) {
        printf("{\"e\": %d}\n", cgd_scale_exponent((uint32_t)strtoul(argv[2], nullptr, 0)));
        return 0;
    }
    fprintf(stderr, "usage: critic_grad_check image I | tiles I C T | plan I C T | why I C T order | scale BITS\n");
    return 2;
}
