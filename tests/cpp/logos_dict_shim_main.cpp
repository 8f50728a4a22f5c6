// tests/test_cpp_logos_dict_shim.py: mi355::trainLogosDictionary (sfm-gms_amd/include/mi355_gms.hpp) on the rows of an input file,
// printing FNV-1a checksums of the dictionary's and the labels' bytes and the record. Input (little-endian): int32 kind (0: 32-byte
// rows, 1: 128-float rows), int32 n, int32 n_words, int32 attempts, int32 max_iters, uint64 seed, then the rows. No arguments:
// prints usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <cstring>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

template <typename T>
static int run(FILE* f, size_t width, const int32_t* head, uint64_t seed)
{
    std::vector<T> rows((size_t)head[0] * width);
    if (!rows.empty() && std::fread(rows.data(), sizeof(T), rows.size(), f) != rows.size()) return 2;
    std::vector<int> labels;
    gms_logos_dict_result res{};
    const std::vector<T> dict = mi355::trainLogosDictionary(rows, head[1], head[2], head[3], seed, &labels, &res);
    std::printf("%llu %llu %d %d %d %llu\n", fnv(dict.data(), dict.size() * sizeof(T)), fnv(labels.data(), labels.size() * sizeof(int)),
                res.attempt, res.iterations, res.empty_clusters, (unsigned long long)res.compactness);
    bool thrown = false;  // more words than rows: the shim throws
    try {
        (void)mi355::trainLogosDictionary(rows, head[0] + 1);
    } catch (const std::runtime_error&) {
        thrown = true;
    }
    std::printf("%d\n", thrown ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "logos_dict_shim_main CASE.bin");
    if (!f) return 2;
    int32_t kind = -1, head[4];
    uint64_t seed = 0;
    if (std::fread(&kind, 4, 1, f) != 1 || std::fread(head, 4, 4, f) != 4 || std::fread(&seed, 8, 1, f) != 1) return 2;
    const int rc = kind == 0 ? run<uint8_t>(f, 32, head, seed) : run<float>(f, 128, head, seed);
    std::fclose(f);
    return rc;
}
