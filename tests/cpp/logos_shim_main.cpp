// tests/test_cpp_logos_shim.py: mi355::matchLOGOS and mi355::matchLOGOSBatch (sfm-gms_amd/include/mi355_gms.hpp) on the cases of
// an input file, printing per case the survivors' count and an FNV-1a checksum of their bytes, single calls first, then the batch.
// Input (little-endian): int32 n_cases, then per case int32 n1, n2, float x, y, size, angle per keypoint of frame 1 then frame 2,
// int32 words of frame 1 then frame 2. No arguments: prints usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "logos_shim_main CASES.bin");
    if (!f) return 2;
    int32_t n_cases = 0;
    if (std::fread(&n_cases, 4, 1, f) != 1) return 2;
    std::vector<std::vector<mi355::KeyPoint>> kps;
    std::vector<std::vector<int>> words;
    for (int c = 0; c < 2 * n_cases; c += 2) {
        int32_t n[2];
        if (std::fread(n, 4, 2, f) != 2) return 2;
        for (int k = 0; k < 2; ++k) {
            std::vector<float> a((size_t)n[k] * 4);
            if (n[k] && std::fread(a.data(), 4, a.size(), f) != a.size()) return 2;
            std::vector<mi355::KeyPoint> kp((size_t)n[k]);
            for (int i = 0; i < n[k]; ++i) {
                kp[i].pt.x = a[4 * i];
                kp[i].pt.y = a[4 * i + 1];
                kp[i].size = a[4 * i + 2];
                kp[i].angle = a[4 * i + 3];
            }
            kps.push_back(kp);
        }
        for (int k = 0; k < 2; ++k) {
            std::vector<int> w((size_t)n[k]);
            if (n[k] && std::fread(w.data(), 4, w.size(), f) != w.size()) return 2;
            words.push_back(w);
        }
    }
    std::fclose(f);
    try {
        std::vector<std::pair<int, int>> pairs;
        for (int c = 0; c < n_cases; ++c) {
            std::vector<mi355::DMatch> m;
            mi355::matchLOGOS(kps[2 * c], kps[2 * c + 1], words[2 * c], words[2 * c + 1], m);
            std::printf("%zu %llu\n", m.size(), fnv_words(m));
            pairs.push_back({2 * c, 2 * c + 1});
        }
        std::vector<std::vector<mi355::DMatch>> out;
        std::vector<bool> ok;
        mi355::matchLOGOSBatch(kps, words, 50, pairs, out, &ok);
        for (int c = 0; c < n_cases; ++c) std::printf("%zu %llu %d\n", out[c].size(), fnv_words(out[c]), ok[c] ? 1 : 0);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
