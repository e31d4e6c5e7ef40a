// Test helper shared by the programs in this directory: reads a flat weight file (speechseparation_amd/weights.py, save_flat) into the
// band table and the parameters by their state_dict keys.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

[[noreturn]] static void die(const char* why) { fprintf(stderr, "tests/cpp: %s\n", why); exit(2); }

struct WeightFile { std::vector<int> widths; std::map<std::string, std::vector<float>> params; };
static WeightFile read_weight_file(const char* path)
{
    WeightFile wf;
    FILE* f = fopen(path, "rb");
    if (!f) die("cannot open the weight file");
    auto rd = [&](void* p, size_t n) { if (fread(p, 1, n, f) != n) die("truncated weight file"); };
    char magic[8];
    uint32_t nb, nt;
    rd(magic, 8);
    if (memcmp(magic, "BSRNNW01", 8)) die("bad magic");
    rd(&nb, 4);
    wf.widths.resize(nb);
    for (uint32_t i = 0; i < nb; ++i) { uint32_t w; rd(&w, 4); wf.widths[i] = (int)w; }
    rd(&nt, 4);
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t kl, nd;
        rd(&kl, 4);
        std::string key(kl, ' ');
        rd(&key[0], kl);
        rd(&nd, 4);
        uint64_t n = 1, d;
        for (uint32_t i = 0; i < nd; ++i) { rd(&d, 8); n *= d; }
        std::vector<float>& v = wf.params[key];
        v.resize(n);
        rd(v.data(), 4 * n);
    }
    fclose(f);
    return wf;
}
