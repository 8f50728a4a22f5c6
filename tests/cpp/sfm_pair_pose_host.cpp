// tests/test_sfm_pair_pose_ref.py: sfm-gms_amd/csrc/sfm_pair_pose_core.h built for the host as a stand-alone program (also under
// sanitizers), so that the arithmetic the kernel runs can be held against tests/sfm_pair_pose_ref.py without a device.
// usage: sfm_pair_pose_host <case file> <result file>. The case: int32 n_frames, n_pairs; gms_sfm_view [n_frames]; gms_pair [n_pairs].
// The result: gms_two_view [n_pairs], gms_sfm_pair_reg [n_pairs], both pre-filled with 0xFF so that an unwritten byte shows.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sfm_pair_pose_core.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[2];
    if (std::fread(head, 4, 2, f) != 2 || !ppose::call_args_ok(head[0], head[1])) return 4;
    const size_t F = (size_t)head[0], P = (size_t)head[1];
    std::vector<gms_sfm_view> views(F);
    std::vector<gms_pair> pairs(P);
    if (std::fread(views.data(), sizeof(gms_sfm_view), F, f) != F || (P && std::fread(pairs.data(), sizeof(gms_pair), P, f) != P)) return 5;
    std::fclose(f);
    std::vector<gms_two_view> tv(P);
    std::vector<gms_sfm_pair_reg> rg(P);
    if (P) {
        std::memset(tv.data(), 0xFF, sizeof(gms_two_view) * P);
        std::memset(rg.data(), 0xFF, sizeof(gms_sfm_pair_reg) * P);
    }
    ppose::pair_poses_host(views.data(), head[0], pairs.data(), head[1], tv.data(), rg.data());
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    if (P && (std::fwrite(tv.data(), sizeof(gms_two_view), P, o) != P || std::fwrite(rg.data(), sizeof(gms_sfm_pair_reg), P, o) != P)) return 7;
    return std::fclose(o) == 0 ? 0 : 8;
}
