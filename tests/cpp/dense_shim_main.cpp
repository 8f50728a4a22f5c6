// tests/test_cpp_dense_shim.py: mi355::stereoRectify, mi355::undistort and mi355::denseStereo (sfm-gms_amd/include/mi355_gms.hpp) on
// the pair of an input file, printing the plan's turn and output size and FNV-1a checksums of: the plan record, image 1 undistorted,
// the int16 map, the points, their pixels and their colours. Input (little-endian): int32 width, int32 height, 9 doubles of the
// camera (fx, fy, cx, cy, k1, k2, p1, p2, k3), 9 doubles R, 3 doubles t, then the two grey images (row-major). No arguments: prints
// usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <cstring>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "dense_shim_main PAIR.bin");
    if (!f) return 2;
    int32_t wh[2];
    double num[21];
    if (std::fread(wh, 4, 2, f) != 2 || std::fread(num, 8, 21, f) != 21) return 2;
    const size_t n = (size_t)wh[0] * (size_t)wh[1];
    std::vector<uint8_t> img1(n), img2(n);
    if (std::fread(img1.data(), 1, n, f) != n || std::fread(img2.data(), 1, n, f) != n) return 2;
    std::fclose(f);
    gms_camera cam;
    std::memcpy(&cam, num, sizeof cam);
    std::array<double, 9> R;
    std::array<double, 3> t;
    std::memcpy(R.data(), num + 9, sizeof R);
    std::memcpy(t.data(), num + 18, sizeof t);
    gms_stereo_sgm_params prm = GMS_STEREO_SGM_PARAMS_DENSE;
    prm.bm.num_disparities = 32;
    const gms_rectify_plan plan = mi355::stereoRectify(cam, R, t, wh[0], wh[1]);
    std::vector<uint8_t> und;
    mi355::undistort(img1, wh[0], wh[1], 1, cam, und);
    const mi355::DenseCloud c = mi355::denseStereo(img1, img2, wh[0], wh[1], 1, cam, R, t, 16, -1, &prm);
    std::printf("%d %d %d %d\n", plan.turn, plan.out_w, plan.out_h, c.count);
    std::printf("%llu\n%llu\n%llu\n%llu\n%llu\n%llu\n", fnv(&plan, sizeof plan), fnv(und.data(), und.size()), fnv(c.disp16.data(), 2 * c.disp16.size()),
                fnv(c.points.data(), 4 * c.points.size()), fnv(c.pixel.data(), 4 * c.pixel.size()), fnv(c.colors.data(), c.colors.size()));
    return 0;
}
