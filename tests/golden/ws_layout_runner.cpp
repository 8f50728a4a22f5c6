// ws_layout_runner.cpp -- prints what the BUILT library says about its device workspaces' sizes, one line per argument tuple:
// six public gms_*_workspace_bytes functions and the four per-pair figures plan_workspace divides its budget by. No device is
// needed. make_ws_layout_fixture.py compiles it against sfm-gms_amd/csrc and libgms_hip.so and keeps the output as
// tests/golden/ws_layout_sizes.txt, which tests/cpp/ws_layout_check.cpp and tests/test_ws_layout.py compare the layouts of
// ws_layout.h with. The fixture in the repository was recorded from the library of commit 063d3a7, the last one whose size
// functions were sums written by hand; its `refined` lines (gms_detect_dog_refined_workspace_bytes over the pyramid lines' tuples, at
// the end: the file only ever grows) from the library of commit e96d1ca, the last one with a refined layout of its own.
#include <array>
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <random>
#include <vector>

#include "gms_kernels.h"

int main()
{
    std::mt19937_64 rng(20261018);
    auto pick = [&](std::initializer_list<long long> v) { return v.begin()[rng() % v.size()]; };
    const int ns[] = {1, 2, 3, 63, 64, 255, 257};
    const int sides[][2] = {{33, 33}, {35, 33}, {97, 65}, {640, 480}, {1921, 1081}, {8192, 8192}, {65535, 65535}, {32, 33}, {0, 5}};

    std::vector<std::array<int, 5>> pyramid_tuples;
    // public: detect and the pyramid (images up to 65 535 a side: n x w x h passes 4 GiB)
    for (const auto& s : sides)
        for (int n : ns)
            for (int maxkp : {0, 1, 7, 5000}) {
                std::printf("detect %d %d %d %d %zu\n", s[0], s[1], n, maxkp, gms_detect_workspace_bytes(s[0], s[1], n, maxkp));
                for (int levels : {1, 2, 16}) {
                    pyramid_tuples.push_back({s[0], s[1], n, maxkp, levels});
                    std::printf("pyramid %d %d %d %d %d %zu\n", s[0], s[1], n, maxkp, levels,
                                gms_detect_pyramid_workspace_bytes(s[0], s[1], n, maxkp, levels));
                }
            }
    for (int i = 0; i < 40; ++i) {
        const int w = (int)(rng() % 3000) - 10, h = (int)(rng() % 3000) - 10, n = (int)pick({-1, 0, 1, 2, 3, 63, 64, 255, 257});
        const int maxkp = (int)pick({-1, 0, 1, 7, 4096}), levels = (int)pick({0, 1, 2, 5, 16, 17});
        std::printf("detect %d %d %d %d %zu\n", w, h, n, maxkp, gms_detect_workspace_bytes(w, h, n, maxkp));
        pyramid_tuples.push_back({w, h, n, maxkp, levels});
        std::printf("pyramid %d %d %d %d %d %zu\n", w, h, n, maxkp, levels, gms_detect_pyramid_workspace_bytes(w, h, n, maxkp, levels));
    }
    // public: StereoBM and portrait mode under the reference's parameters, sides up to 8192
    for (const auto& s : sides)
        for (int n : {0, 1, 2, 3, 63, 64, 255, 257, 65535, 65536}) {
            std::printf("stereo %d %d %d %zu\n", s[0], s[1], n, gms_stereo_bm_workspace_bytes(s[0], s[1], n, nullptr));
            std::printf("portrait %d %d %d %zu\n", s[0], s[1], n, gms_portrait_workspace_bytes(s[0], s[1], n, nullptr));
        }
    for (int i = 0; i < 40; ++i) {
        const int w = (int)(rng() % 2000) + 20, h = (int)(rng() % 2000) + 20, n = (int)pick({1, 2, 3, 63, 64, 255, 257});
        std::printf("stereo %d %d %d %zu\n", w, h, n, gms_stereo_bm_workspace_bytes(w, h, n, nullptr));
        std::printf("portrait %d %d %d %zu\n", w, h, n, gms_portrait_workspace_bytes(w, h, n, nullptr));
    }
    // public: bruteForceMatch's selection
    for (int n : {0, 1, 2, 3, 63, 64, 255, 257, -1})
        for (int rows : {0, 1, 37, 500, 4095, 4096, 4097, 1 << 22, (1 << 22) + 1})
            for (long long back : {0ll, 1ll, 15ll, 16ll, 17ll, 3ll * 37, (long long)n * rows, 1ll << 33, -1ll})
                std::printf("bfsel %d %d %lld %zu\n", n, rows, back, gms_bf_select_workspace_bytes(n, rows, back));

    // internal: the per-pair figures, over big_mcap's range (multiples of 64 from 16 448 to kBigMaxMatches) and around multiples of 4096
    gms::FilterParams p{};
    const double ratio[5] = {1.0, 1.0 / 2, 1.0 / std::sqrt(2.0), std::sqrt(2.0), 2.0};  // the right grids of the product (gms_capi.cpp)
    for (int s = 0; s < 5; ++s) p.right_w[s] = p.right_h[s] = (int)std::lrint(gms::kLeftW * ratio[s]);
    std::vector<int> mcaps = {gms::big_mcap(16385), gms::big_mcap(gms::kBigMaxMatches), 20416, 20480, 20544, 65472, 65536, 65600, 262144, 1 << 20};
    for (int i = 0; i < 20; ++i) mcaps.push_back(gms::big_mcap(16385 + (int)(rng() % (gms::kBigMaxMatches - 16385))));
    for (int mcap : mcaps) {
        for (int mask = 0; mask < 2; ++mask) {
            std::printf("band %d %d %zu\n", mcap, mask, gms::band_ws_bytes_per_pair(mcap, mask != 0));
            for (int scale = 0; scale < 2; ++scale) {
                p.with_scale = scale;
                std::printf("tile %d %d %d %zu\n", scale, mcap, mask, gms::tile_ws_bytes_per_pair(p, mcap, mask != 0));
            }
        }
        for (int scale = 0; scale < 2; ++scale) {
            p.with_scale = scale;
            std::printf("stream %d %d %zu\n", scale, mcap, gms::stream_ws_bytes_per_pair(p, mcap, true));
        }
        std::printf("dense %d %zu\n", mcap, gms::stream_dense_ws_bytes_per_pair(mcap));
    }
    // public: the refined DoG call's pyramid, on the pyramid lines' tuples
    for (const auto& t : pyramid_tuples)
        std::printf("refined %d %d %d %d %d %zu\n", t[0], t[1], t[2], t[3], t[4], gms_detect_dog_refined_workspace_bytes(t[0], t[1], t[2], t[3], t[4]));
    return 0;
}
