// Asks speechseparation_amd/csrc/critic_spectrum_host.h (compiled alone, no HIP) what tests/test_critic_spectrum_reference.py checks.
//   critic_spectrum_check frames n                -> T
//   critic_spectrum_check reflect n t             -> the 4096 clip indices of frame t, one per line
//   critic_spectrum_check plan R n                -> JSON: the CsPlan, every slab, the constants
//   critic_spectrum_check check R n stride scale  -> the verdict of cs_check (scale: a number, "inf" or "nan")
//   critic_spectrum_check self                    -> "ok" after the program's own sweep: every (row, frame) in exactly one slab, the scratch
//                                                    under its cap, every reflected index inside the clip
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "critic_spectrum_host.h"

using namespace bsrnn;

static int self_check()
{
    const int64_t cap = (int64_t)CS_CAP_UNITS * CS_TILE_T * CS_CHANNELS;
    const int Rs[] = {1, 2, 3, 4, 5, 63, 64, 65, 80, 127, 128, 129, 255, 256, 257, 1000};
    const int64_t ns[] = {2049, 2050, 3071, 3072, 4095, 4096, 31 * 1024, 32 * 1024 - 1, 32 * 1024, 33 * 1024 + 5, 600 * 1024, 1023 * 1024 + 7,
                          1024 * 1024, 2646000, 4096 * 1024 + 1};
    for (int R : Rs)
        for (int64_t n : ns) {
            const int why = cs_check(R, n, n, 1.0f);
            if (why == CS_TOO_LARGE && (int64_t)R * CS_CHANNELS * (1 + n / 1024) > CS_MAX_ELEMS) continue;
            if (why != CS_OK) return 1;
            const CsPlan p = cs_plan(R, n);
            if (p.T != 1 + n / 1024 || p.slabs != p.row_blocks * p.frame_slabs || p.scratch_floats > cap || p.scratch_floats < 1) return 2;
            if (p.frames_per_slab % CS_TILE_T || p.frames_per_slab % CS_CHUNK || (int64_t)p.rows_per_block * p.frames_per_slab > (int64_t)CS_CAP_UNITS * CS_TILE_T)
                return 3;
            std::vector<unsigned char> seen((size_t)R * p.T, 0);
            for (int s = 0; s < p.slabs; ++s) {
                const CsSlab q = cs_slab(p, R, s);
                if (q.r0 < 0 || q.r1 > R || q.r0 >= q.r1 || q.t0 < 0 || q.t1 > p.T || q.t0 >= q.t1) return 4;
                if ((int64_t)(q.r1 - q.r0) * (q.t1 - q.t0) * CS_CHANNELS > p.scratch_floats) return 5;
                if (q.t0 % CS_CHUNK || q.t0 % CS_TILE_T) return 6;
                // workgroups of the slab's two launches: chunks x rows, and 32-bit grid dimensions
                if ((int64_t)((q.t1 - q.t0 + CS_CHUNK - 1) / CS_CHUNK) * (q.r1 - q.r0) > 1024) return 7;
                for (int r = q.r0; r < q.r1; ++r)
                    for (int t = q.t0; t < q.t1; ++t)
                        if (seen[(size_t)r * p.T + t]++) return 8;
            }
            for (unsigned char v : seen)
                if (v != 1) return 9;
            // the first and the last two frames reach over the ends
            const int64_t ts[] = {0, 1, 2, p.T - 2, p.T - 1};
            for (int64_t t : ts)
                for (int i = 0; i < CS_NFFT; ++i) {
                    if (t < 0) continue;
                    const int64_t at = cs_sample(t, i, n);
                    if (at < 0 || at >= n) return 10;
                }
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "frames")) {
        printf("%lld\n", (long long)cs_frames(atoll(argv[2])));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "reflect")) {
        const long long n = atoll(argv[2]), t = atoll(argv[3]);
        for (int i = 0; i < CS_NFFT; ++i) printf("%lld\n", (long long)cs_sample(t, i, n));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "plan")) {
        const int R = atoi(argv[2]);
        const long long n = atoll(argv[3]);
        const CsPlan p = cs_plan(R, n);
        printf("{\"T\": %d, \"rows_per_block\": %d, \"row_blocks\": %d, \"frames_per_slab\": %d, \"frame_slabs\": %d, \"slabs\": %d, \"scratch_floats\": %lld, "
               "\"chunk\": %d, \"tile_t\": %d, \"tile_b\": %d, \"cap_units\": %d, \"channels\": %d, \"list\": [",
               p.T, p.rows_per_block, p.row_blocks, p.frames_per_slab, p.frame_slabs, p.slabs, (long long)p.scratch_floats, CS_CHUNK, CS_TILE_T,
               CS_TILE_B, CS_CAP_UNITS, CS_CHANNELS);
        for (int s = 0; s < p.slabs; ++s) {
            const CsSlab q = cs_slab(p, R, s);
            printf("%s[%d, %d, %d, %d]", s ? ", " : "", q.r0, q.r1, q.t0, q.t1);
        }
        printf("]}\n");
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "check")) {
        printf("%d\n", cs_check(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), strtof(argv[5], nullptr)));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "self")) {
        const int rc = self_check();
        if (rc) { printf("failed: %d\n", rc); return 1; }
        printf("ok\n");
        return 0;
    }
    fprintf(stderr, "usage: critic_spectrum_check frames n | reflect n t | plan R n | check R n stride scale | self\n");
    return 2;
}
