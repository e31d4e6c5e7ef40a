// Test helper: asks the host-only call plan (speechseparation_amd/csrc/plan_host.h) what it decides and prints one JSON line.
//   call_plan_check plan K C T gemv overlap  band_pair band_parts time_fused seq8 gemm_mode lstm_mode cus  exact fused band_pair_off overlap_env overlap_off
//   call_plan_check cuts n                    every cut of a clip of n samples, for seg = 1 .. T
//   call_plan_check blocks K cus R T          the row blocks of a bsrnn_separate call under the default knobs
//   call_plan_check flags parts Rmax Tmax     the flag placement of `parts` row blocks, for R = 2 .. Rmax, T = 1 .. Tmax
//   call_plan_check orders <weights.bsrnnw> C T nwg cus      the dispatch orders of the overlapped dual path
//   call_plan_check workspace rows LDP LDA K
//   call_plan_check state C K
#include "commit_host.h"
#include "plan_host.h"
#include "weight_file.h"
using namespace bsrnn;

static const PlanKnobs kDefaultKnobs = {true, true, true, -1, GEMM_FP16X2, LSTM_FP16X2, 256};

template <class V>
static void print_list(const char* name, const V& v, const char* end = ", ")
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? ", " : "", (long long)v[i]);
    printf("]%s", end);
}

int main(int argc, char** argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    auto arg = [&](int i) { return atoll(argv[i]); };
    if (cmd == "plan" && argc == 19) {
        const PlanKnobs kn = {arg(7) != 0, arg(8) != 0, arg(9) != 0, (int)arg(10), (int)arg(11), (int)arg(12), (int)arg(13)};
        const PlanState st = {arg(14) != 0, arg(15) != 0, arg(16) != 0, arg(17) != 0, arg(18) != 0};
        const Flow f = plan_call((int)arg(2), (int)arg(3), (int)arg(4), arg(5) != 0, arg(6) != 0, kn, st);
        static const char* const kBand[] = {"SMALL", "PAIR_PARTS", "PAIR", "LAYERS"};
        printf("{\"exact\": %d, \"lstm_f32\": %d, \"gemv\": %d, \"chains\": %d, \"band\": \"%s\", \"time_fc\": %d, \"seqs\": %d, \"nwg\": %d, \"overlap\": %d}\n",
               f.exact, f.lstm_f32, f.gemv, f.chains, kBand[f.band], f.time_fc, f.seqs, f.nwg, f.overlap);
    } else if (cmd == "cuts" && argc == 3) {
        const int64_t n = arg(2);
        const int T = 1 + (int)(n / HOPS);
        printf("{\"T\": %d, \"segs\": {", T);
        for (int seg = 1; seg <= T; ++seg) {
            int ms[2];
            const int nms = long_frame_rows(3, T, seg, ms);
            printf("%s\"%d\": {\"window_floats\": %zu, \"block_floats\": %zu, ", seg > 1 ? ", " : "", seg, staging_window_floats(seg), staging_block_floats(seg));
            print_list("frame_rows_of_3", std::vector<int>(ms, ms + nms));
            printf("\"cuts\": [");
            for (int i = 0; i < (T + seg - 1) / seg; ++i) {
                const SegmentCut q = segment_cut(n, T, seg, i);
                printf("%s[%d, %d, %d, %d, %lld, %lld]", i ? ", " : "", q.ta, q.te, q.hop0, q.nh, (long long)q.lo, (long long)q.wl);
            }
            printf("]}");
        }
        printf("}}\n");
    } else if (cmd == "blocks" && argc == 6) {
        PlanKnobs kn = kDefaultKnobs;
        kn.cus = (int)arg(3);
        const int R = (int)arg(4), T = (int)arg(5);
        const Flow whole = plan_call((int)arg(2), R, T, false, true, kn, PlanState{false, true, false, true, false});
        const RowBlocks b = row_blocks(R, T, row_block_count(R, T, whole.nwg, kn.cus));
        printf("{\"parts\": %d, ", b.parts);
        print_list("r0", std::vector<int>(b.r0, b.r0 + b.parts + 1));
        print_list("ms", std::vector<int>(b.ms, b.ms + b.parts), "}\n");
    } else if (cmd == "flags" && argc == 5) {
        const int parts = (int)arg(2);
        if (parts < 1 || parts > MAX_PARTS) die("parts");
        printf("{\"max_parts\": %d, \"cases\": [", MAX_PARTS);
        for (int R = 2; R <= arg(3); ++R)
            for (int T = 1; T <= arg(4); ++T) {
                const RowBlocks b = row_blocks(R, T, parts);
                std::vector<size_t> off, used;
                std::vector<int> share;
                for (int j = 0; j < parts; ++j) {
                    off.push_back(flag_offset((size_t)b.r0[j] * T, j));
                    used.push_back(flag_ints_used((size_t)b.ms[j]));
                    if (j) share.push_back(row_blocks_share_flags(b, T, j));
                }
                printf("%s{\"R\": %d, \"T\": %d, ", R > 2 || T > 1 ? ", " : "", R, T);
                print_list("r0", std::vector<int>(b.r0, b.r0 + parts + 1));
                print_list("offset", off);
                print_list("used", used);
                print_list("share", share);
                printf("\"reserved\": %zu}", flag_ints_reserved((size_t)R * T));
            }
        printf("]}\n");
    } else if (cmd == "orders" && argc == 7) {
        const WeightFile wf = read_weight_file(argv[2]);
        const BandColumns bc = band_columns(wf.widths);
        const WeightImage im = build_weight_image([&](const std::string& key) -> const std::vector<float>& { return wf.params.at(key); }, wf.widths,
                                                  bc.aoff, bc.poff, CommitKnobs{GEMM_FP16X2, false, false, false, true});
        if (!im.fused) die("the table does not take the fused chains");
        std::vector<ChainDesc> ds;
        std::vector<int> rows, constant, flat;
        for (const ChainRec& r : im.chains[CHAIN_MASK]) { ds.push_back(r.d); rows.push_back(chain_rows(r.d)); constant.push_back(r.d.constant); }
        const int C = (int)arg(3), T = (int)arg(4), nwg = (int)arg(5);
        const OvlOrders o = ovl_orders(C * T, T, nwg, (int)arg(6), ds);
        for (const ChainTask& t : o.mask_tasks) { flat.push_back(t.desc); flat.push_back(t.row0); }
        printf("{\"stride\": %d, \"head\": %d, ", ovl_stride(nwg), OVL_HEAD);
        print_list("rows", rows);
        print_list("constant", constant);
        print_list("band_order", o.band_order);
        print_list("mask_tasks", flat, "}\n");
    } else if (cmd == "workspace" && argc == 6) {
        size_t s[WS_SEGS];
        workspace_segments((size_t)arg(2), (int)arg(3), (int)arg(4), (int)arg(5), s);
        printf("{");
        print_list("sizes", std::vector<size_t>(s, s + WS_SEGS), "}\n");
    } else if (cmd == "state" && argc == 4) {
        printf("{\"state\": %zu, \"slab\": %zu}\n", state_floats((int)arg(2), (int)arg(3)), state_slab_floats((int)arg(2), (int)arg(3)));
    } else {
        die("usage: call_plan_check plan | cuts | blocks | flags | orders | workspace | state ...");
    }
    return 0;
}
