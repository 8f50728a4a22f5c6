// tests/test_cpp_stereo_sgm_shim.py: mi355::stereo_match_sgm and mi355::stereoSGM (sfm-gms_amd/include/mi355_gms.hpp) on the pair of an
// input file, printing an FNV-1a checksum of the 8-bit map (reference parameters) and of the int16 map (the params form with four
// paths). Input (little-endian): int32 width, int32 height, the left image, the right image (row-major bytes). No arguments: prints
// usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "stereo_sgm_shim_main PAIR.bin");
    if (!f) return 2;
    int32_t wh[2];
    if (std::fread(wh, 4, 2, f) != 2) return 2;
    const size_t n = (size_t)wh[0] * (size_t)wh[1];
    std::vector<uint8_t> left(n), right(n);
    if (std::fread(left.data(), 1, n, f) != n || std::fread(right.data(), 1, n, f) != n) return 2;
    std::fclose(f);
    std::vector<uint8_t> d8;
    mi355::stereo_match_sgm(left, right, wh[0], wh[1], d8);
    gms_stereo_sgm_params four = mi355::stereo_sgm_reference_params();
    four.n_paths = 4;
    std::vector<int16_t> d16;
    mi355::stereoSGM(left, right, wh[0], wh[1], four, d16);
    std::printf("%llu\n%llu\n", fnv(d8.data(), d8.size()), fnv(reinterpret_cast<const unsigned char*>(d16.data()), d16.size() * 2));
    return 0;
}
