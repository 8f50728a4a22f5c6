// tests/test_cpp_sfm_register_shim.py: mi355::registerViews (sfm-gms_amd/include/mi355_gms.hpp) on the arrays of an input file, printing
// an FNV-1a checksum of each output in the order views, pairs, points_world, track, cloud, cloud_id, cloud_obs, cloud_est, cloud_spread,
// summary. Input (little-endian): int32 n_frames, n_pairs, root, min_links; int64 total match slots; frame_off int64 [n_frames + 1];
// gms_pair [n_pairs]; gms_dmatch [total]; mask uint8 [total]; points3d double [total][3]; gms_two_view [n_pairs]. No arguments: prints
// usage and exits 2 (the CPU test links this without a device).
#include <cstdio>
#include <vector>

#include "mi355_gms.hpp"
#include "test_main_util.h"

int main(int argc, char** argv)
{
    FILE* f = open_input(argc, argv, "sfm_register_shim_main RECORDS.bin");
    if (!f) return 2;
    int32_t head[4];
    int64_t total;
    if (std::fread(head, 4, 4, f) != 4 || std::fread(&total, 8, 1, f) != 1 || head[0] < 1 || head[1] < 0 || total < 0) return 2;
    std::vector<int64_t> frame_off((size_t)head[0] + 1);
    std::vector<gms_pair> pairs((size_t)head[1]);
    std::vector<gms_dmatch> matches((size_t)total);
    std::vector<uint8_t> mask((size_t)total);
    std::vector<double> points(3 * (size_t)total);
    std::vector<gms_two_view> tv((size_t)head[1]);
    if (!read_all(f, frame_off) || !read_all(f, pairs) || !read_all(f, matches) || !read_all(f, mask) || !read_all(f, points) || !read_all(f, tv)) return 2;
    std::fclose(f);
    const mi355::Registration r = mi355::registerViews(frame_off, pairs, matches, mask, points, tv, head[2], head[3]);
    print_sum(r.views);
    print_sum(r.pairs);
    print_sum(r.points_world);
    print_sum(r.track);
    print_sum(r.cloud);
    print_sum(r.cloud_id);
    print_sum(r.cloud_obs);
    print_sum(r.cloud_est);
    print_sum(r.cloud_spread);
    std::printf("%llu\n", fnv(&r.summary, sizeof r.summary));
    return 0;
}
