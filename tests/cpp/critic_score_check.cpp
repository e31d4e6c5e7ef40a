// Asks speechseparation_amd/csrc/critic_score_host.h (compiled alone, no HIP) what tests/test_critic_score_host.py checks; prints JSON.
//   critic_score_check image I        -> the bijection check of the image index map, done here (the image has 131 072 I_pad positions)
//   critic_score_check rows I order   -> {"rows": [I]}: the row of x every channel reads
//   critic_score_check plan I C T     -> the CscPlan, the slabs' ranges, the exact layers' scratch sizes
//   critic_score_check why I C T order -> {"why": n}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "critic_score_host.h"

using namespace bsrnn;

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "image")) {
        const int I = atoi(argv[2]);
        const int64_t n = csc_image_halves(I);
        std::vector<unsigned char> hit((size_t)n, 0);
        long long twice = 0, out_of_range = 0, inverse_wrong = 0, padding_hit = 0, padding = 0, unaligned = 0;
        for (int o = 0; o < CSC_O; ++o)
            for (int i = 0; i < I; ++i)
                for (int k = 0; k < CRITIC_TAPS; ++k)
                    for (int pc = 0; pc < 2; ++pc) {
                        const int64_t p = csc_image_index(I, o, i, k, pc);
                        if (p < 0 || p >= n) { ++out_of_range; continue; }
                        if (hit[(size_t)p]++) ++twice;
                        int o2, i2, k2, pc2;
                        if (!csc_image_source(I, p, &o2, &i2, &k2, &pc2) || o2 != o || i2 != i || k2 != k || pc2 != pc) ++inverse_wrong;
                        if (k % 8 == 0 && p % 8 != 0) ++unaligned;          // the eight taps of a lane are one aligned 16-byte unit
                        if (k % 8 && p != csc_image_index(I, o, i, k - 1, pc) + 1) ++unaligned;
                    }
        for (int64_t p = 0; p < n; ++p)
            if (!hit[(size_t)p]) {
                int o2, i2, k2, pc2;
                ++padding;
                if (csc_image_source(I, p, &o2, &i2, &k2, &pc2)) ++padding_hit;      // a position nobody maps to must read as padding (zero)
            }
        printf("{\"halves\": %lld, \"i_pad\": %d, \"block\": %d, \"twice\": %lld, \"out_of_range\": %lld, \"inverse_wrong\": %lld, "
               "\"padding\": %lld, \"padding_not_zero\": %lld, \"unaligned\": %lld}\n",
               (long long)n, csc_i_pad(I), CSC_BLOCK, twice, out_of_range, inverse_wrong, padding, padding_hit, unaligned);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "rows")) {
        const int I = atoi(argv[2]), order = atoi(argv[3]);
        printf("{\"rows\": [");
        for (int i = 0; i < I; ++i) printf("%s%d", i ? ", " : "", csc_channel_row(I, i, order));
        printf("]}\n");
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "plan")) {
        const int I = atoi(argv[2]), C = atoi(argv[3]), T = atoi(argv[4]);
        const CscPlan p = csc_plan(I, C, T);
        printf("{\"len\": [%d, %d, %d, %d], \"t_tiles\": %d, \"o_tiles\": %d, \"slabs\": %d, \"ch_per_slab\": %d, \"ch\": %d, \"min_slab\": %d, "
               "\"fill\": %d, \"off_y\": [%lld, %lld, %lld, %lld], \"off_shared\": %lld, \"ws\": %lld, \"ws_exact\": %lld, \"slab_ranges\": [",
               p.len[0], p.len[1], p.len[2], p.len[3], p.t_tiles, p.o_tiles, p.slabs, p.ch_per_slab, CSC_CH, CSC_MIN_SLAB, CSC_FILL,
               (long long)p.off_y[0], (long long)p.off_y[1], (long long)p.off_y[2], (long long)p.off_y[3], (long long)p.off_shared,
               (long long)p.ws_floats, (long long)p.ws_exact_floats);
        for (int s = 0; s < p.slabs; ++s) {
            const int lo = s * p.ch_per_slab, hi = lo + p.ch_per_slab < I ? lo + p.ch_per_slab : I;
            printf("%s[%d, %d]", s ? ", " : "", lo, hi);
        }
        printf("], \"exact_scratch\": [");
        int in = I, t = T;
        for (int l = 0; l < CRITIC_LAYERS; ++l) {
            printf("%s%lld", l ? ", " : "", (long long)critic_forward_scratch_floats(C, in, t, CRITIC_WIDTHS[l]));
            in = CRITIC_WIDTHS[l]; t = p.len[l];
        }
        printf("]}\n");
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "why")) {
        printf("{\"why\": %d}\n", csc_check(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5])));
        return 0;
    }
    fprintf(stderr, "usage: critic_score_check image I | rows I order | plan I C T | why I C T order\n");
    return 2;
}
