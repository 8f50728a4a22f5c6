// speckle_core.h -- what the speckle filter's kernels (speckle_kernels.hip), the C ABI and a host compiler share:
// the link predicate, the argument check, the tile constants, and a plain sequential statement of the filter that
// tests/cpp/speckle_host.cpp compiles alone. No HIP header.
//
// The definition (integer, free of any scan order). On an int16 map [H, W]: two pixels are linked when they are 4-neighbours,
// neither equals new_val, and |a - b| <= max_diff, the difference taken in 32 bits. Components are the transitive closure of the
// links. Every pixel that is not new_val and whose component has at most max_speckle_size pixels becomes new_val; nothing else
// changes. max_diff is in the map's own units.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SPK_HD __host__ __device__ __forceinline__
#else
#define SPK_HD inline
#endif

namespace spk {

// One workgroup labels one tile in LDS: 2 bytes of value and 8 of label and size per pixel, 20 KiB.
constexpr int kTileW = 64, kTileH = 32, kTilePx = kTileW * kTileH;
constexpr int kBlock = 256;
constexpr int kMaxSide = 8192, kMaxImages = 65535;

// |a - b| is at most 65535: no wrap in 32 bits
SPK_HD bool linked(int a, int b, int new_val, int max_diff)
{
    const int d = a > b ? a - b : b - a;
    return a != new_val && b != new_val && d <= max_diff;
}

inline bool args_ok(int width, int height, int n, int new_val, int max_speckle_size, int max_diff)
{
    return width >= 1 && width <= kMaxSide && height >= 1 && height <= kMaxSide && n >= 1 && n <= kMaxImages && new_val >= -32768 &&
           new_val <= 32767 && max_speckle_size >= 0 && max_diff >= 0;
}

// The statement: a raster scan; every unlabelled pixel that is not new_val starts a flood fill over an explicit stack, which counts
// its component; a second walk over the same component writes new_val when the count is small. Returns the pixels changed.
inline int filter_host(int16_t* img, int width, int height, int new_val, int max_speckle_size, int max_diff)
{
    const size_t px = (size_t)width * (size_t)height;
    std::vector<uint8_t> seen(px, 0);
    std::vector<int32_t> stack, members;
    int removed = 0;
    for (size_t s = 0; s < px; ++s) {
        if (seen[s] || img[s] == new_val) continue;
        members.clear();
        stack.assign(1, (int32_t)s);
        seen[s] = 1;
        while (!stack.empty()) {
            const int32_t p = stack.back();
            stack.pop_back();
            members.push_back(p);
            const int y = p / width, x = p - y * width, v = img[p];
            const int32_t nb[4] = {x > 0 ? p - 1 : -1, x + 1 < width ? p + 1 : -1, y > 0 ? p - width : -1, y + 1 < height ? p + width : -1};
            for (int k = 0; k < 4; ++k) {
                const int32_t q = nb[k];
                if (q >= 0 && !seen[q] && linked(v, img[q], new_val, max_diff)) {
                    seen[q] = 1;
                    stack.push_back(q);
                }
            }
        }
        if (members.size() <= (size_t)max_speckle_size) {
            for (int32_t p : members) img[p] = (int16_t)new_val;
            removed += (int)members.size();
        }
    }
    return removed;
}

}  // namespace spk
