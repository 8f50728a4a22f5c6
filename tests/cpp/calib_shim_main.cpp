// tests/test_cpp_calib_shim.py: mi355::addChessboardPoints and mi355::calibrateCamera (sfm-gms_amd/include/mi355_gms.hpp) on the grey
// images of an input file, as the reference's main() runs them (main.cpp:53-68), printing: the successes; the first and last corner of
// every found board; fx fy cx cy; the five distortion coefficients; the RMS -- with 17 significant digits. Input (little-endian):
// int32 n, width, height, nx, ny, then n grey images (1 byte per pixel, row-major). No arguments: prints usage and exits 2 (the CPU
// test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "calib_shim_main IMAGES.bin");
    if (!f) return 2;
    int32_t hd[5];
    if (std::fread(hd, 4, 5, f) != 5) return 2;
    const size_t px = (size_t)hd[1] * (size_t)hd[2];
    std::vector<std::vector<uint8_t>> images((size_t)hd[0], std::vector<uint8_t>(px));
    for (auto& im : images)
        if (std::fread(im.data(), 1, px, f) != px) return 2;
    std::fclose(f);
    std::vector<std::vector<mi355::ObjectPoint>> obj;
    std::vector<std::vector<mi355::ImagePoint>> img;
    const int ok = mi355::addChessboardPoints(images, hd[1], hd[2], mi355::Size(hd[3], hd[4]), obj, img);
    std::printf("%d\n", ok);
    for (const auto& c : img) std::printf("%.17g %.17g %.17g %.17g\n", c.front().x, c.front().y, c.back().x, c.back().y);
    if (ok == 0) return 0;
    const mi355::CameraCalibration c = mi355::calibrateCamera(obj, img, mi355::Size(hd[1], hd[2]));
    std::printf("%.17g %.17g %.17g %.17g\n", c.K[0], c.K[4], c.K[2], c.K[5]);
    std::printf("%.17g %.17g %.17g %.17g %.17g\n", c.dist[0], c.dist[1], c.dist[2], c.dist[3], c.dist[4]);
    std::printf("%.17g\n", c.rms);
    return 0;
}
