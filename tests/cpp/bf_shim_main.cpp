// tests/test_cpp_bf_shim.py: mi355::bruteForceMatch and mi355::bruteForceMatchBatch (sfm-gms_amd/include/mi355_gms.hpp) on the
// frames and pairs of an input file, printing per pair the survivors' count and an FNV-1a checksum of their bytes, single calls
// first, then the batch. Input (little-endian): int32 kind (0: 32-byte rows, 1: 128-float rows), int32 n_frames, per frame int32 n
// and its rows, int32 n_pairs, int32 (a, b) per pair. No arguments: prints usage and exits 2 (the CPU test links this without a
// device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

template <typename T>
static int run(FILE* f, size_t width)
{
    int32_t nf = 0;
    if (std::fread(&nf, 4, 1, f) != 1) return 2;
    std::vector<std::vector<T>> rows((size_t)nf);
    for (auto& r : rows) {
        int32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1) return 2;
        r.resize((size_t)n * width);
        if (n && std::fread(r.data(), sizeof(T), r.size(), f) != r.size()) return 2;
    }
    int32_t np = 0;
    if (std::fread(&np, 4, 1, f) != 1) return 2;
    std::vector<std::pair<int, int>> pairs((size_t)np);
    for (auto& p : pairs) {
        int32_t ab[2];
        if (std::fread(ab, 4, 2, f) != 2) return 2;
        p = {ab[0], ab[1]};
    }
    for (const auto& p : pairs) {
        std::vector<mi355::DMatch> m;
        mi355::bruteForceMatch(rows[(size_t)p.first], rows[(size_t)p.second], m);
        std::printf("%zu %llu\n", m.size(), fnv_words(m));
    }
    std::vector<std::vector<mi355::DMatch>> all;
    std::vector<bool> ok;
    mi355::bruteForceMatchBatch(rows, pairs, all, true, 4.0, 500, &ok);
    for (size_t p = 0; p < pairs.size(); ++p) std::printf("%zu %llu %d\n", all[p].size(), fnv_words(all[p]), ok[p] ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "bf_shim_main CASES.bin");
    if (!f) return 2;
    int32_t kind = -1;
    if (std::fread(&kind, 4, 1, f) != 1) return 2;
    const int rc = kind == 0 ? run<uint8_t>(f, 32) : run<float>(f, 128);
    std::fclose(f);
    return rc;
}
