// Test helper: asks the host-only call plan (speechseparation_amd/csrc/plan_host.h) how many tiles of 16 sequences a workgroup of the
// band-pair launch takes, and prints one JSON line.
//   band_tiles_check rule N cus force         band_pair_tiles, band_pair_slots, band_pair_grid for N sequences
//   band_tiles_check plan K C T cus force     what plan_call puts into the Flow of a call of C rows x T frames (default knobs otherwise)
#include "plan_host.h"

#include <cstdio>
#include <cstdlib>
#include <string>
using namespace bsrnn;

int main(int argc, char** argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    auto arg = [&](int i) { return atoi(argv[i]); };
    if (cmd == "rule" && argc == 5) {
        const int N = arg(2), tiles = band_pair_tiles(N, arg(3), arg(4));
        printf("{\"tiles\": %d, \"slots\": %d, \"grid\": %d}\n", tiles, band_pair_slots(N, tiles), band_pair_grid(N, tiles));
    } else if (cmd == "plan" && argc == 7) {
        PlanKnobs kn = {true, true, true, -1, GEMM_FP16X2, LSTM_FP16X2, arg(5)};
        kn.band_tiles = arg(6);
        const Flow f = plan_call(arg(2), arg(3), arg(4), true, true, kn, PlanState{false, true, false, true, false});
        static const char* const kBand[] = {"SMALL", "PAIR_PARTS", "PAIR", "LAYERS"};
        printf("{\"band\": \"%s\", \"band_tiles\": %d}\n", kBand[f.band], f.band_tiles);
    } else {
        fprintf(stderr, "usage: band_tiles_check rule N cus force | plan K C T cus force\n");
        return 2;
    }
    return 0;
}
