// logos_words_dist.h -- the device functions of the words call (gms_logos_words_device, logos_batch_kernels.hip) that the dictionary
// trainer (logos_dict_kernels.hip) shares with it: lane l of a wave computes, alone and in the sequential order of the definition
// (DESIGN.md §6b), the distance of the wave's current row to word (tile + l); a wave-wide (distance, index) minimum leaves the lowest
// index among equal distances.
#pragma once
#include <hip/hip_runtime.h>

namespace gms {
namespace logos {

constexpr int kWordTile = 64;

__device__ __forceinline__ void wave_argmin(float& d, int& w)
{
    for (int s = 1; s < 64; s <<= 1) {
        const float od = __shfl_xor(d, s);
        const int ow = __shfl_xor(w, s);
        if (od < d || (od == d && ow < w)) {
            d = od;
            w = ow;
        }
    }
}

__device__ __forceinline__ float l2_words_dist(const float* __restrict__ row, const float (*tile)[kWordTile], int lane)
{
    float acc = 0.0f;
    for (int g = 0; g < 128; g += 4) {
        const float d0 = row[g] - tile[g][lane], d1 = row[g + 1] - tile[g + 1][lane];
        const float d2 = row[g + 2] - tile[g + 2][lane], d3 = row[g + 3] - tile[g + 3][lane];
        const float s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s3 = d3 * d3;
        const float grp = ((s0 + s1) + s2) + s3;
        acc = acc + grp;
    }
    return acc;
}

}  // namespace logos
}  // namespace gms
