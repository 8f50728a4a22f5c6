// tests/test_cpp_sfm_pair_pose_shim.py: mi355::pairPosesFromViews (sfm-gms_amd/include/mi355_gms.hpp) on the arrays of an input file,
// written back as the bytes of its two_view and reg vectors. Input (little-endian): int32 n_frames, n_pairs; gms_sfm_view [n_frames];
// int32 [n_pairs][2] frame pairs. No arguments: prints usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "sfm_pair_pose_shim_main CASE.bin RESULT.bin", 2);
    if (!f) return 2;
    int32_t head[2];
    if (std::fread(head, 4, 2, f) != 2 || head[0] < 1 || head[1] < 1) return 2;
    std::vector<gms_sfm_view> views((size_t)head[0]);
    std::vector<int32_t> fp(2 * (size_t)head[1]);
    if (std::fread(views.data(), sizeof(gms_sfm_view), views.size(), f) != views.size() || std::fread(fp.data(), 4, fp.size(), f) != fp.size()) return 2;
    std::fclose(f);
    std::vector<std::pair<int, int>> frame_pairs;
    for (size_t i = 0; i < (size_t)head[1]; ++i) frame_pairs.emplace_back(fp[2 * i], fp[2 * i + 1]);
    const mi355::PairPoses r = mi355::pairPosesFromViews(views, frame_pairs);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const bool ok = std::fwrite(r.two_view.data(), sizeof(gms_two_view), r.two_view.size(), o) == r.two_view.size() &&
                    std::fwrite(r.reg.data(), sizeof(gms_sfm_pair_reg), r.reg.size(), o) == r.reg.size();
    return std::fclose(o) == 0 && ok ? 0 : 1;
}
