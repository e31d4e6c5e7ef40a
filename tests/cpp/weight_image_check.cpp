// Test helper: builds the committed weight image (speechseparation_amd/csrc/commit_host.h) of a flat weight file on the host.
//   weight_image_check <weights.bsrnnw> <gemm mode 0..3> <mlp_layers> <no48> <no80> <rag> <dump file>
// writes the whole image to <dump file> - pointers as arena offsets, little endian:
//   u64 n, n x f32 arena | u64 n, n x {i32 N, K, x_off, y_off, r_off, m_off, wrow, u64 W, bias, Wp} jobs | u64 n, n x {i32 job, tile} tiles
//   | i32[NSLOT] job0, njobs, tile0, ntiles, tile_n | i32 fused
//   | per chain: u64 n, n x {ChainLayer[5], i32 nbias .. zpad (11), u64 wstream, bias, i64 cost} | per block: u64[13] BlockSegs
// and prints one JSON line: arena size, fused, build time, the segment offsets and, per chain and band, bsrnn_chain_geometry's answer.
#include "commit_host.h"
#include "weight_file.h"
#include <chrono>
using namespace bsrnn;

int main(int argc, char** argv)
{
    if (argc != 8) die("usage");
    const WeightFile wf = read_weight_file(argv[1]);
    const std::vector<int>& widths = wf.widths;
    const auto& params = wf.params;
    const CommitKnobs kn = {atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]) != 0, atoi(argv[5]) != 0, atoi(argv[6]) != 0};
    const BandColumns bc = band_columns(widths);
    const auto t0 = std::chrono::steady_clock::now();
    const WeightImage im = build_weight_image([&](const std::string& key) -> const std::vector<float>& { return params.at(key); },
                                              widths, bc.aoff, bc.poff, kn);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

    FILE* f = fopen(argv[7], "wb");
    if (!f) die("cannot open the dump file");
    auto w64 = [&](uint64_t v) { fwrite(&v, 8, 1, f); };
    auto w32 = [&](int32_t v) { fwrite(&v, 4, 1, f); };
    w64(im.arena.size()); fwrite(im.arena.data(), 4, im.arena.size(), f);
    w64(im.jobs.size());
    for (const JobRec& r : im.jobs) {
        const GemmJob& j = r.j;
        w32(j.N); w32(j.K); w32(j.x_off); w32(j.y_off); w32(j.r_off); w32(j.m_off); w32(j.wrow);
        w64(r.w); w64(r.b); w64(r.wp);
    }
    w64(im.tiles.size());
    for (const GemmTile& t : im.tiles) { w32(t.job); w32(t.tile); }
    const SlotTables& s = im.slots;
    for (const int* a : {s.job0, s.njobs, s.tile0, s.ntiles, s.tile_n}) fwrite(a, 4, NSLOT, f);
    w32(im.fused ? 1 : 0);
    for (int ch = 0; ch < 2; ++ch) {
        w64(im.chains[ch].size());
        for (const ChainRec& r : im.chains[ch]) {
            fwrite(r.d.L, sizeof(ChainLayer), CHAIN_LAYERS, f);
            for (int v : {r.d.nbias, r.d.NW, r.d.RT, r.d.plane_units, r.d.in_off, r.d.K0, r.d.p_off, r.d.a8, r.d.z_off, r.d.constant, r.d.zpad}) w32(v);
            w64(r.w); w64(r.b);
            const int64_t cost = r.cost;
            fwrite(&cost, 8, 1, f);
        }
    }
    std::string segs;
    for (int blk = 0; blk < 2; ++blk) {
        const BlockSegs& b = im.blk[blk];
        segs += blk ? ", [" : "[";
        for (size_t v : {b.bandW[0], b.bandW[1], b.bandB[0], b.bandB[1], b.bandW16[0], b.bandW16[1], b.bandFc16, b.bandFcB, b.timeW, b.timeB,
                         b.timeW16, b.timeFc16, b.timeFcB}) {
            w64(v);
            segs += std::to_string(v) + ", ";
        }
        segs.replace(segs.size() - 2, 2, "]");
    }
    if (fclose(f)) die("write failed");

    printf("{\"arena_floats\": %zu, \"fused\": %s, \"build_ms\": %.3f, \"segs\": [%s], \"geometry\": [", im.arena.size(), im.fused ? "true" : "false", ms, segs.c_str());
    for (int ch = 0; ch < 2; ++ch) {
        printf("%s[", ch ? ", " : "");
        for (size_t band = 0; band < widths.size(); ++band) {
            int g[6];
            for (int& v : g) v = im.fused ? 0 : -1;
            if (im.fused && widths[band] > 0)
                for (const ChainRec& r : im.chains[ch])
                    if (!r.d.constant && r.d.z_off == (int)band * HID) chain_geometry_answer(r.d, g);
            printf("%s[%d, %d, %d, %d, %d, %d]", band ? ", " : "", g[0], g[1], g[2], g[3], g[4], g[5]);
        }
        printf("]");
    }
    printf("]}\n");
    return 0;
}
