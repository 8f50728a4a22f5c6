// dog_core.h -- the arithmetic of the difference-of-Gaussians (DoG) detector (numpy statement tests/dog_ref.py): blob
// candidates on one level image of the pyramid keypoint source, in integer arithmetic only. It is this library's own definition, not
// cv::SIFT's: one layer per pyramid level, one refinement step that clamps where SIFT re-centres (`refine` below; the plain call has
// none), and the detector's centroid direction afterwards.
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
//   refine     at a candidate (numpy statement tests/dog_refine_ref.py), with the candidate rule's dxx, dyy, dxy4, det16 > 0:
//              position  gx2 = D(x+1) - D(x-1), gy2 likewise in y; nx = -(8 dyy gx2 - 2 dxy4 gy2), ny = -(8 dxx gy2 - 2 dxy4 gx2): -H^-1 g
//                        scaled so that nx / det16 is the offset in pixels. ox = floor((32 nx + det16) / (2 det16)): 1/16 pixel, rounded
//                        half up, then clamped to [-8, 8] (SIFT re-centres beyond half a pixel; this rule clamps); oy likewise.
//                        |gx2| <= 2 * 65280: |nx| <= 10 * (4 * 65280) * (2 * 65280) < 2^39, det16 < 2^40: the numerator stays below 2^45.
//              scale     a = D_2 - D_0, b = D_0 + D_2 - 2c at (x, y); b != 0 and |a| < |b| because c is a strict extremum over both.
//                        n = a if b < 0 else -a, q = 2 |b|; os = floor((32 n + q) / (2 q)): 1/16 layer, |os| <= 8 without a clamp.
//              FLOOR divisions (the divisors are positive), not C++ truncation. Only the clamped quotient is needed, which
//              floor_div_clamped gets exactly from an fp32 guess and one int64 remainder: no 64-bit division on the device.
//              code      1 + (ox + 8) + 17 (oy + 8) + 289 (os + 8): 1 .. 4913, u16; 0 = no candidate.
//              record    px = (float)x + (float)ox * 0.0625f (exact), X = (px + 0.5f) * fx - 0.5f, size = (31.0f * fx) * kScale[os + 8],
//                        kScale[i] = float32(1.2^((i - 8) / 16)) (the layers of a level are a factor 1.2 apart); kScale[8] = 1.
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

// ---- refinement of a candidate to 1/16 pixel and 1/16 layer ----------------------------------------------------------------------------
constexpr int kOffsetMax = 8, kOffsetSteps = 2 * kOffsetMax + 1;   // offsets -8 .. 8 in 1/16
constexpr int kMaxCode = kOffsetSteps * kOffsetSteps * kOffsetSteps;

// floor(a / b) for b > 0, clamped to [-lim, lim], lim < 2^20, without a 64-bit division: an fp32 quotient clamped to [-lim - 1, lim + 1]
// is within 1 of the floor (its relative error is below 2^-22, so its absolute error below 1), or the floor lies beyond the clamp on
// that side; one exact remainder in int64 (|g b| < 2^62 for the b of this header, b < 2^42) corrects it.
GMS_HD int floor_div_clamped(int64_t a, int64_t b, int lim)
{
    float f = (float)a / (float)b;
    f = f < (float)(-lim - 1) ? (float)(-lim - 1) : (f > (float)(lim + 1) ? (float)(lim + 1) : f);
    int g = (int)f;
    g -= (float)g > f;   // floor of the clamped quotient
    const int64_t r = a - (int64_t)g * b;
    g += (r >= b) - (r < 0);
    return g < -lim ? -lim : (g > lim ? lim : g);
}
// round(16 n / q) with halves up, q > 0, clamped to [-kOffsetMax, kOffsetMax]
GMS_HD int sixteenths(int64_t n, int64_t q) { return floor_div_clamped(32 * n + q, 2 * q, kOffsetMax); }

struct Offsets {
    int ox, oy, os;   // 1/16 pixel, 1/16 pixel, 1/16 layer; each in -8 .. 8
    GMS_HD int code() const { return 1 + (ox + kOffsetMax) + kOffsetSteps * (oy + kOffsetMax) + kOffsetSteps * kOffsetSteps * (os + kOffsetMax); }
};
GMS_HD Offsets offsets_of(int code)   // code in 1 .. kMaxCode
{
    const int v = code - 1;
    return {v % kOffsetSteps - kOffsetMax, v / kOffsetSteps % kOffsetSteps - kOffsetMax, v / (kOffsetSteps * kOffsetSteps) - kOffsetMax};
}

// The offsets of a pixel that candidate() kept (so det16 > 0 and c is a strict extremum); d as candidate() takes it.
template <class F>
GMS_HD Offsets refine(F d)
{
    const int c = d(1, 0, 0);
    const int64_t dxx = (int64_t)d(1, 1, 0) + d(1, -1, 0) - 2 * (int64_t)c;
    const int64_t dyy = (int64_t)d(1, 0, 1) + d(1, 0, -1) - 2 * (int64_t)c;
    const int64_t dxy4 = (int64_t)d(1, 1, 1) - d(1, -1, 1) - d(1, 1, -1) + d(1, -1, -1);
    const int64_t det16 = 16 * dxx * dyy - dxy4 * dxy4;
    const int64_t gx2 = (int64_t)d(1, 1, 0) - d(1, -1, 0), gy2 = (int64_t)d(1, 0, 1) - d(1, 0, -1);
    const int64_t nx = -(8 * dyy * gx2 - 2 * dxy4 * gy2), ny = -(8 * dxx * gy2 - 2 * dxy4 * gx2);
    const int ox = sixteenths(nx, det16), oy = sixteenths(ny, det16);
    const int64_t a = (int64_t)d(2, 0, 0) - d(0, 0, 0), b = (int64_t)d(0, 0, 0) + d(2, 0, 0) - 2 * (int64_t)c;
    const int os = sixteenths(b < 0 ? a : -a, 2 * (b < 0 ? -b : b));
    return {ox, oy, os};   // (os is within the clamp by itself: |a| < |b|)
}

// kScale[i] = float32(1.2^((i - 8) / 16)); the numbers are the definition, the CPU test checks them against the rule
GMS_HD float scale_of(int os)
{
    static constexpr float t[kOffsetSteps] = {0.91287094f, 0.9233327f, 0.9339143f, 0.9446172f, 0.9554428f, 0.9663924f, 0.97746754f, 0.9886696f, 1.0f,
                                              1.0114603f, 1.0230519f, 1.0347763f, 1.0466352f, 1.0586299f, 1.070762f, 1.0830332f, 1.0954452f};
    return t[os + kOffsetMax];
}
// a refined coordinate on level 0: integer level coordinate v, offset o in 1/16 pixel, factor f; every operation rounded once (-ffp-contract=off)
GMS_HD float refined_coord(int v, int o, float f) { return (((float)v + (float)o * 0.0625f) + 0.5f) * f - 0.5f; }
GMS_HD float refined_size(int os, float fx) { return (31.0f * fx) * scale_of(os); }

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


// the candidate plane and the code plane (refine's code at a candidate, else 0) together
inline void candidate_and_code_plane(const uint16_t* const B[kBlurs], int w, int h, int contrast, uint8_t* cand, uint16_t* codes)
{
    candidate_plane(B, w, h, contrast, cand);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t at = (size_t)y * w + x;
            codes[at] = 0;
            if (cand[at] == 0) continue;
            codes[at] = (uint16_t)refine([&](int k, int dx, int dy) {
                            const ptrdiff_t o = (ptrdiff_t)at + (ptrdiff_t)dy * w + dx;
                            return (int)B[k + 1][o] - (int)B[k][o];
                        }).code();
        }
}

}  // namespace dog
}  // namespace gms
