// tests/test_cpp_warp_shim.py: mi355::resize, mi355::warpAffine and mi355::img_rotate (sfm-gms_amd/include/mi355_gms.hpp) on the image
// of an input file, printing an FNV-1a checksum of: the image resized to 101 x 67, img_rotate by 180 degrees, warpAffine by
// getRotationMatrix2D((30, 20), 30, 0.8) into 90 x 50, and the first channel alone resized to half its size. Input (little-endian):
// int32 width, int32 height (both even), the BGR image (3 bytes per pixel, row-major). No arguments: prints usage and exits 2 (the
// CPU test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "warp_shim_main IMAGE.bin");
    if (!f) return 2;
    int32_t wh[2];
    if (std::fread(wh, 4, 2, f) != 2) return 2;
    const size_t n = (size_t)wh[0] * (size_t)wh[1];
    std::vector<uint8_t> img(3 * n), first(n);
    if (std::fread(img.data(), 1, 3 * n, f) != 3 * n) return 2;
    std::fclose(f);
    std::vector<uint8_t> small, turned, warped, half;
    mi355::resize(img, wh[0], wh[1], 3, 101, 67, small);
    mi355::img_rotate(img, wh[0], wh[1], 3, 180.0, turned);
    mi355::warpAffine(img, wh[0], wh[1], 3, mi355::getRotationMatrix2D(30, 20, 30, 0.8), 90, 50, warped);
    for (size_t i = 0; i < n; ++i) first[i] = img[3 * i];
    mi355::resize(first, wh[0], wh[1], 1, wh[0] / 2, wh[1] / 2, half);
    std::printf("%llu\n%llu\n%llu\n%llu\n", fnv(small), fnv(turned), fnv(warped), fnv(half));
    return 0;
}
