// grad_desc_core.h -- the arithmetic of the gradient descriptor (numpy statement tests/grad_desc_ref.py): a row of
// SIFT's structure and format -- 4 x 4 cells x 8 orientations = 128 values, float32 holding integers 0..255 -- at a keypoint of the
// detector (detect_kernels.hip), on the keypoint's own pyramid level. It is this library's own definition in integer arithmetic, not
// cv::SIFT's: every sample's contribution is an integer, so the sums do not depend on the order of the additions.
//
// Plain functions of their arguments, so that the SAME source is what grad_desc_kernels.hip runs and what tests/cpp/grad_desc_host.cpp
// compiles with g++ for the CPU tests.
//
// Per keypoint (x, y, direction bin b of 32) with (c, s) = (dir_c(b), dir_s(b)) in Q12, S = the detector's 5 x 5 box sum (u16):
//   samples    all integer (dx, dy) with dx^2 + dy^2 <= 169 (a disc: unchanged by rotation), 529 of them, raster order. Radius 13, + 1
//              for the gradient, + 2 for the box = 16 = GMS_DETECT_BORDER: every read is inside the image and the defined part of S.
//   gradient   gx = S(u + 1, v) - S(u - 1, v), gy = S(u, v + 1) - S(u, v - 1) at (u, v) = (x + dx, y + dy); |gx|, |gy| <= 25 * 255 = 6375
//   frame      rx = dx c + dy s, ry = -dx s + dy c; fx = gx c + gy s, fy = -gx s + gy c: Q12, nothing rounded.
//              |rx|, |ry| <= 13 (|c| + |s|) <= 13 * 5793 = 75 309;  |fx|, |fy| <= 6375 * 5793 = 36 930 375 < 2^31
//   cells      six pixels wide, centres at -1.5, -0.5, 0.5, 1.5 cells. t = rx + kBinOffset (5.5 cells of 6 * 4096 = 135 168 > 75 309, so
//              t > 0); i0 = t / 24576 - 4 in [-1, 3]; w1 = (t % 24576) / 96 in 0..255, w0 = 256 - w1; cell i0 gets w0, cell i0 + 1 gets w1;
//              a cell outside 0..3 is dropped. The same for ry (cell row).
//   bins       ax = |fx| >> 12, ay = |fy| >> 12 -- the one shift, before any weight; ax, ay <= 9016. hi = max, lo = min. The gradient
//              is split on the two of the eight directions that enclose it (no atan, no sqrt): in the first octant (0 <= fy <= fx)
//              g = (fx - fy) e_0 + (sqrt2 fy) e_1. So the axis bin (0 or 4 by fx's sign when ax >= ay, else 2 or 6 by fy's) gets hi - lo
//              <= 9016, and the quadrant's diagonal bin (1, 3, 5, 7) gets (lo * 5793) >> 12 <= 12 751.
//   weight     W = (window_weight(dx^2 + dy^2) * wx * wy) >> 16 <= 256; accumulator[(cell row * 4 + cell column) * 8 + bin] += part * W
//   bound      the sum of W over the samples one cell sees depends on b alone and is at most kMaxCellWeight = 8281 (tests/
//              test_grad_desc_ref.py recomputes it), so an accumulator stays below 8281 * 12 751 = 105 591 031 < 2^27: int32 holds it,
//              and the 128 squares sum to less than 2^61.
//   normalise  n = isqrt(sum v^2); v = min(v, n / 5); n' = isqrt(sum v^2); out = min(255, (512 v + n' / 2) / n'); all 0 when n' = 0
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

namespace gms {
namespace gd {

constexpr int kBorder = 16;                                  // = GMS_DETECT_BORDER
constexpr int kRadius = 13, kR2 = 169, kSamples = 529;
constexpr int kDim = 128;
constexpr int kCellQ12 = 6 * 4096;                           // a cell's width in Q12 pixels
constexpr int kBinOffset = 4 * kCellQ12 + 3 * kCellQ12 / 2;  // 1.5 cells (centres at +-0.5, +-1.5) + 4 cells (non-negative)
constexpr int kSqrt2Q12 = 5793;
constexpr int kMaxCellWeight = 8281;
constexpr int kMaxPart = (int)(((int64_t)((25 * 255 * kSqrt2Q12) >> 12) * kSqrt2Q12) >> 12);   // 12 751
static_assert(kRadius + 1 + 2 == kBorder, "samples + gradient + box stay inside the detector's border");
static_assert(13 * kSqrt2Q12 < kBinOffset, "the cell split sees no negative number");
static_assert((int64_t)kMaxCellWeight * kMaxPart < (1 << 27), "an accumulator fits int32 and the 128 squares fit 64 bits");

// the detector's 32 directions in Q12 (detect_kernels.hip's table)
GMS_HD int dir_c(int b)
{
    static constexpr int16_t t[32] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799, 0, -799, -1567, -2276, -2896, -3406, -3784, -4017,
                                      -4096, -4017, -3784, -3406, -2896, -2276, -1567, -799, 0, 799, 1567, 2276, 2896, 3406, 3784, 4017};
    return t[b];
}
GMS_HD int dir_s(int b) { return dir_c((b + 24) & 31); }   // sin(a) = cos(a - 90 degrees): the table turned by eight bins

// round(256 * exp(-r2 / (2 * 12^2))), r2 = 0 .. 169: numbers, so that no two math libraries are asked
GMS_HD int window_weight(int r2)
{
    static constexpr uint16_t t[kR2 + 1] = {
        256, 255, 254, 253, 252, 252, 251, 250, 249, 248, 247, 246, 246, 245, 244, 243, 242,
        241, 240, 240, 239, 238, 237, 236, 236, 235, 234, 233, 232, 231, 231, 230, 229, 228,
        227, 227, 226, 225, 224, 224, 223, 222, 221, 220, 220, 219, 218, 217, 217, 216, 215,
        214, 214, 213, 212, 211, 211, 210, 209, 209, 208, 207, 206, 206, 205, 204, 204, 203,
        202, 201, 201, 200, 199, 199, 198, 197, 197, 196, 195, 195, 194, 193, 193, 192, 191,
        191, 190, 189, 189, 188, 187, 187, 186, 185, 185, 184, 183, 183, 182, 182, 181, 180,
        180, 179, 178, 178, 177, 177, 176, 175, 175, 174, 174, 173, 172, 172, 171, 171, 170,
        169, 169, 168, 168, 167, 166, 166, 165, 165, 164, 164, 163, 162, 162, 161, 161, 160,
        160, 159, 159, 158, 157, 157, 156, 156, 155, 155, 154, 154, 153, 153, 152, 152, 151,
        150, 150, 149, 149, 148, 148, 147, 147, 146, 146, 145, 145, 144, 144, 143, 143, 142};
    return t[r2];
}

// the samples in raster order, made at compile time
struct Samples { int8_t d[kSamples][2]; };
constexpr int count_samples()
{
    int n = 0;
    for (int dy = -kRadius; dy <= kRadius; ++dy)
        for (int dx = -kRadius; dx <= kRadius; ++dx) n += dx * dx + dy * dy <= kR2 ? 1 : 0;
    return n;
}
static_assert(count_samples() == kSamples, "the disc of radius 13 holds 529 integer points");
constexpr Samples make_samples()
{
    Samples t{};
    int n = 0;
    for (int dy = -kRadius; dy <= kRadius; ++dy)
        for (int dx = -kRadius; dx <= kRadius; ++dx)
            if (dx * dx + dy * dy <= kR2) {
                t.d[n][0] = (int8_t)dx; t.d[n][1] = (int8_t)dy;
                ++n;
            }
    return t;
}

// the detector's direction from the moments of the disc of radius 15: the largest integer dot product, the lowest bin among equals
GMS_HD int direction_bin(int m10, int m01)
{
    int best = 0;
    long long top = (long long)m10 * dir_c(0) + (long long)m01 * dir_s(0);
    for (int k = 1; k < 32; ++k) {
        const long long d = (long long)m10 * dir_c(k) + (long long)m01 * dir_s(k);
        if (d > top) { top = d; best = k; }
    }
    return best;
}

// (cell that gets w0, w1) of a frame coordinate; cell + 1 gets w1, w0 = 256 - w1
GMS_HD void split_cell(int r, int& cell, int& w1)
{
    const int t = r + kBinOffset;
    cell = t / kCellQ12 - 4;
    w1 = (t - (cell + 4) * kCellQ12) / 96;
}

// One sample's contributions: add(index, value) for each of at most eight accumulators. S: the box sums of the keypoint's image.
template <class Add>
GMS_HD void accumulate_sample(const uint16_t* S, int w, int x, int y, int c, int s, int i, Add&& add)
{
    static constexpr Samples smp = make_samples();
    const int dx = smp.d[i][0], dy = smp.d[i][1];
    const uint16_t* p = S + (size_t)(y + dy) * w + (x + dx);
    const int gx = (int)p[1] - (int)p[-1], gy = (int)p[w] - (int)p[-w];
    if (gx == 0 && gy == 0) return;
    const int rx = dx * c + dy * s, ry = -dx * s + dy * c;
    const int fx = gx * c + gy * s, fy = -gx * s + gy * c;
    int ix, iy, wx1, wy1;
    split_cell(rx, ix, wx1);
    split_cell(ry, iy, wy1);
    const int ax = (fx < 0 ? -fx : fx) >> 12, ay = (fy < 0 ? -fy : fy) >> 12;
    const int hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
    const int axis_bin = ax >= ay ? (fx < 0 ? 4 : 0) : (fy < 0 ? 6 : 2);
    const int diag_bin = fy >= 0 ? (fx >= 0 ? 1 : 3) : (fx >= 0 ? 7 : 5);
    const int part_axis = hi - lo, part_diag = (lo * kSqrt2Q12) >> 12;
    const int win = window_weight(dx * dx + dy * dy);
    for (int jy = 0; jy < 2; ++jy) {
        const int cy = iy + jy, wy = jy ? wy1 : 256 - wy1;
        if (cy < 0 || cy > 3) continue;
        for (int jx = 0; jx < 2; ++jx) {
            const int cx = ix + jx, wx = jx ? wx1 : 256 - wx1;
            if (cx < 0 || cx > 3) continue;
            const int W = (win * wx * wy) >> 16;
            if (W == 0) continue;
            const int cell = (cy * 4 + cx) * 8;
            if (part_axis != 0) add(cell + axis_bin, part_axis * W);
            if (part_diag != 0) add(cell + diag_bin, part_diag * W);
        }
    }
}

// floor(sqrt(x)) for x < 2^63: an estimate from the double square root, made exact by integer comparisons (so the estimate's own
// rounding, which may differ between a CPU and the GPU, never shows)
GMS_HD uint64_t isqrt64(uint64_t x)
{
    uint64_t r = (uint64_t)__builtin_sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

GMS_HD int32_t clip_value(int32_t v, uint64_t n) { const int64_t cap = (int64_t)(n / 5); return v < cap ? v : (int32_t)cap; }

// the output value of a clipped accumulator; n2 = isqrt of the clipped values' sum of squares
GMS_HD float quantise(int32_t v, uint64_t n2)
{
    if (n2 == 0) return 0.0f;
    const uint64_t q = (512ull * (uint64_t)v + n2 / 2) / n2;
    return (float)(q < 255 ? q : 255);
}

// the whole row on one thread (the host build's path; the kernel spreads the same steps over a wave)
inline void describe_row(const uint16_t* S, int w, int x, int y, int bin, float* out)
{
    int32_t acc[kDim] = {};
    const int c = dir_c(bin), s = dir_s(bin);
    for (int i = 0; i < kSamples; ++i) accumulate_sample(S, w, x, y, c, s, i, [&acc](int k, int v) { acc[k] += v; });
    uint64_t sum = 0;
    for (int k = 0; k < kDim; ++k) sum += (uint64_t)((int64_t)acc[k] * acc[k]);
    const uint64_t n = isqrt64(sum);
    sum = 0;
    for (int k = 0; k < kDim; ++k) {
        acc[k] = clip_value(acc[k], n);
        sum += (uint64_t)((int64_t)acc[k] * acc[k]);
    }
    const uint64_t n2 = isqrt64(sum);
    for (int k = 0; k < kDim; ++k) out[k] = quantise(acc[k], n2);
}

}  // namespace gd
}  // namespace gms
