// tests/test_cpp_speckle_shim.py: mi355::filterSpeckles (sfm-gms_amd/include/mi355_gms.hpp) on the case of an input file, printing
// the number of pixels changed and an FNV-1a checksum of the filtered map. Input: the format of tests/cpp/speckle_host.cpp (int32
// width, height, new_val, max_speckle_size, max_diff, then the int16 map). No arguments: prints usage and exits 2 (the CPU test links
// this without a device). A refused call prints the exception and exits 3.
#include <cstdio>
#include <exception>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "speckle_shim_main CASE.bin");
    if (!f) return 2;
    int32_t h[5];
    if (std::fread(h, 4, 5, f) != 5 || h[0] < 1 || h[0] > 8192 || h[1] < 1 || h[1] > 8192) return 2;
    std::vector<int16_t> disp((size_t)h[0] * (size_t)h[1]);
    if (std::fread(disp.data(), 2, disp.size(), f) != disp.size()) return 2;
    std::fclose(f);
    try {
        const int removed = mi355::filterSpeckles(disp, h[0], h[1], h[2], h[3], h[4]);
        std::printf("%d\n%llu\n", removed, fnv(disp.data(), 2 * disp.size()));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
