// dog_core.h -- the arithmetic of the difference-of-Gaussians (DoG) detector (numpy statement tests/dog_ref.py): blob
// candidates on one level image of the pyramid keypoint source, in integer arithmetic only. It is this library's own definition, not
// cv::SIFT's: one layer per pyramid level, no sub-pixel or sub-scale refinement, and the detector's centroid direction afterwards.
//
// Plain functions of their arguments, so that the SAME source is what dog_kernels.hip runs and what tests/cpp/dog_host.cpp compiles
// with g++ for the CPU tests.
//
// On a level image p (uint8):
//   blurs      four separable blurs B_0..B_3, sigma_j = 1.6 * 1.2^(j - 1.5) (1.217, 1.461, 1.753, 2.103), radius r_j = ceil(3 sigma_j) =
//              4 + j, integer taps K_j that sum to 4096 (the numbers below ARE the definition; the CPU test checks them against
//              round(4096 g_i / sum g), the centre adjusted to the sum).
//              horizontal first  H = (sum K[i] p[x + i] + 8) >> 4        Q8, <= 65280: u16
//              then vertical     B = (sum K[i] H[y + i] + 2048) >> 12    Q8, u16; the sum <= 4096 * 65280 < 2^31
//              No clamping at the edges: a value is used only where every tap is inside the image.
//   layers     D_k = B_{k+1} - B_k, k = 0, 1, 2: int32 in Q8, |D| <= 65280
//   candidate  at 16 <= x < w - 16, 16 <= y < h - 16 (GMS_DETECT_BORDER; the farthest read is 1 + 7 pixels away), with c = D_1(x, y):
//              |c| > contrast; c strictly greater than all 26 neighbours (8 in D_1, 9 each in D_0 and D_2) or strictly less than all;
//              and the edge test on D_1 in int64: dxx = D(x+1) + D(x-1) - 2c, dyy likewise,
//              dxy4 = D(x+1,y+1) - D(x-1,y+1) - D(x+1,y-1) + D(x-1,y-1), tr = dxx + dyy, det16 = 16 dxx dyy - dxy4^2;
//              keep when det16 > 0 and 160 tr^2 < 121 det16 (SIFT's r = 10: tr^2 / det < 11^2 / 10). A tie gives no keypoint.
//              |dxx|, |dyy| <= 4 * 65280, |dxy4| <= 4 * 65280: det16 and 160 tr^2 stay below 2^46.
//   score      max(1, min(255, |c| >> 4)): u8 in 1/16 grey level; 0 = no candidate -- the format of the detector's candidate plane.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef GMS_HD
#if defined(__HIPCC__)
#define GMS_HD __host__ __device__ __forceinline__
#else
#define GMS_HD inline
#endif
#endif
#ifndef GMS_UNROLL
#if defined(__HIPCC__)
#define GMS_UNROLL _Pragma("unroll")
#else
#define GMS_UNROLL
#endif
#endif

namespace gms {
namespace dog {

constexpr int kBorder = 16;          // = GMS_DETECT_BORDER
constexpr int kBlurs = 4, kLayers = 3;
constexpr int kMaxRadius = 7, kMaxTaps = 2 * kMaxRadius + 1;
constexpr int kTapSum = 4096;
constexpr int kReach = 1 + kMaxRadius;   // the farthest pixel a candidate reads
constexpr int kMaxContrast = 65535;
static_assert(kReach <= kBorder, "every tap of a candidate is inside the image");

constexpr int radius(int j) { return 4 + j; }

// K_j[i], i = 0 .. 2 r_j (rows padded with zeros)
GMS_HD int tap(int j, int i)
{
    static constexpr int16_t t[kBlurs][kMaxTaps] = {
        {6, 64, 348, 958, 1344, 958, 348, 64, 6, 0, 0, 0, 0, 0, 0},
        {3, 26, 136, 438, 885, 1120, 885, 438, 136, 26, 3, 0, 0, 0, 0},
        {3, 16, 69, 216, 486, 792, 932, 792, 486, 216, 69, 16, 3, 0, 0},
        {3, 13, 46, 127, 281, 495, 694, 778, 694, 495, 281, 127, 46, 13, 3}};
    return t[j][i];
}

// sum over i = -r_J .. r_J of K_J[i + r_J] * at(i), the symmetric taps folded; at(i) <= 65280, so the sum fits int32
template <int J, class F>
GMS_HD int weighted_sum(F at)
{
    constexpr int r = radius(J);
    int s = tap(J, r) * at(0);
GMS_UNROLL
    for (int i = 1; i <= r; ++i) s += tap(J, r - i) * (at(-i) + at(i));
    return s;
}
GMS_HD int round_h(int s) { return (s + 8) >> 4; }
GMS_HD int round_v(int s) { return (s + 2048) >> 12; }

GMS_HD int score_of(int c)
{
    const int a = (c < 0 ? -c : c) >> 4;
    return a < 1 ? 1 : (a > 255 ? 255 : a);
}

// The candidate rule at one pixel: d(k, dx, dy) = D_k at the pixel + (dx, dy), dx, dy in -1..1. Returns the score, or 0.
template <class F>
GMS_HD int candidate(int contrast, F d)
{
    const int c = d(1, 0, 0);
    if ((c < 0 ? -c : c) <= contrast) return 0;
    bool above = true, below = true;   // c against the 26 neighbours
GMS_UNROLL
    for (int k = 0; k < kLayers; ++k)
GMS_UNROLL
        for (int dy = -1; dy <= 1; ++dy)
GMS_UNROLL
            for (int dx = -1; dx <= 1; ++dx) {
                if (k == 1 && dx == 0 && dy == 0) continue;
                const int v = d(k, dx, dy);
                above = above && c > v;
                below = below && c < v;
            }
    if (!above && !below) return 0;
    const int64_t dxx = (int64_t)d(1, 1, 0) + d(1, -1, 0) - 2 * (int64_t)c;
    const int64_t dyy = (int64_t)d(1, 0, 1) + d(1, 0, -1) - 2 * (int64_t)c;
    const int64_t dxy4 = (int64_t)d(1, 1, 1) - d(1, -1, 1) - d(1, 1, -1) + d(1, -1, -1);
    const int64_t tr = dxx + dyy, det16 = 16 * dxx * dyy - dxy4 * dxy4;
    if (det16 <= 0 || 160 * tr * tr >= 121 * det16) return 0;
    return score_of(c);
}

// ---- whole planes, for the host build (the kernel does the same through LDS tiles) ----------------------------------------------------
// H_j and B_j of an image: values where a tap would leave the image are 0 and never used
template <int J>
inline void blur_plane(const uint8_t* img, int w, int h, uint16_t* H, uint16_t* B)
{
    constexpr int r = radius(J);
    for (size_t i = 0; i < (size_t)w * h; ++i) H[i] = B[i] = 0;
    for (int y = 0; y < h; ++y)
        for (int x = r; x < w - r; ++x) {
            const uint8_t* p = img + (size_t)y * w + x;
            H[(size_t)y * w + x] = (uint16_t)round_h(weighted_sum<J>([p](int i) { return (int)p[i]; }));
        }
    for (int y = r; y < h - r; ++y)
        for (int x = r; x < w - r; ++x) {
            const uint16_t* q = H + (size_t)y * w + x;
            B[(size_t)y * w + x] = (uint16_t)round_v(weighted_sum<J>([q, w](int i) { return (int)q[(ptrdiff_t)i * w]; }));
        }
}

// the candidate plane (score, or 0) of an image from its four blur planes
inline void candidate_plane(const uint16_t* const B[kBlurs], int w, int h, int contrast, uint8_t* cand)
{
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int sc = 0;
            if (x >= kBorder && x < w - kBorder && y >= kBorder && y < h - kBorder) {
                const size_t at = (size_t)y * w + x;
                sc = candidate(contrast, [&](int k, int dx, int dy) {
                    const ptrdiff_t o = (ptrdiff_t)at + (ptrdiff_t)dy * w + dx;
                    return (int)B[k + 1][o] - (int)B[k][o];
                });
            }
            cand[(size_t)y * w + x] = (uint8_t)sc;
        }
}

}  // namespace dog
}  // namespace gms
