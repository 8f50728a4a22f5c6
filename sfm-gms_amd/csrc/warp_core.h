// warp_core.h -- cv::resize (INTER_LINEAR, 8-bit) and cv::warpAffine (INTER_LINEAR, BORDER_CONSTANT 0, 8-bit) as integer arithmetic
// on taps that come from a few IEEE fp32 / fp64 operations: what the kernels (warp_kernels.hip), the C ABI
// (capi_image.cpp) and the host test build (tests/cpp/warp_host.cpp) share. tests/warp_ref.py states the same in numpy. Built with
// -ffp-contract=off: no product below may be fused into a sum.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WARP_HD __host__ __device__ inline
#else
#define WARP_HD inline
#endif

namespace warp {

constexpr int kMaxSide = 8192;

// the sizes and layouts stated here (the others are GMS_ERR_BAD_ARG)
WARP_HD bool side_ok(int v) { return v >= 1 && v <= kMaxSide; }
WARP_HD bool args_ok(int n, int sw, int sh, int channels, long long src_pitch, int dw, int dh, long long dst_pitch)
{
    return n >= 1 && n <= 65535 && (channels == 1 || channels == 3) && side_ok(sw) && side_ok(sh) && side_ok(dw) && side_ok(dh) &&
           src_pitch >= (long long)channels * sw && dst_pitch >= (long long)channels * dw && src_pitch <= 0x7fffffffll &&
           dst_pitch <= 0x7fffffffll;
}

// ---- resize ---------------------------------------------------------------------------------------------------------------------
// 1 / (dn / sn), as OpenCV forms it (not sn / dn: the two differ in the last bit for some sizes)
WARP_HD double axis_scale(int dn, int sn) { return 1.0 / ((double)dn / (double)sn); }
// the 2 x 2 mean replaces the taps when both axes halve exactly
WARP_HD bool is_area2(int sw, int sh, int dw, int dh) { return axis_scale(dw, sw) == 2.0 && axis_scale(dh, sh) == 2.0; }

// saturate_cast<short>(float): round half to even, then clamp
WARP_HD int round_short(float v)
{
    const float r = rintf(v);
    return r < -32768.f ? -32768 : r > 32767.f ? 32767 : (int)r;
}

struct Tap {
    int s;       // the first source index (may be -1 or sn - 1 for a row tap: the caller clamps s and s + 1)
    int w0, w1;  // weights of s and s + 1, 11 fractional bits
};

// destination index d of an axis of dn samples made from sn. Columns (clamp = true): a tap left of the image becomes column 0 with
// fraction 0, a tap at or right of the last column becomes the last column alone (weight 2048; s + 1 is never read: w1 = 0).
// Rows (clamp = false) keep their fraction; the caller clamps the two row indices.
WARP_HD Tap axis_tap(int d, double scale, int sn, bool clamp)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp) {
        if (s < 0) {
            s = 0;
            f = 0.f;
        }
        if (s >= sn - 1) {
            s = sn - 1;
            f = 0.f;
        }
    }
    Tap t;
    t.s = s;
    t.w0 = round_short((1.f - f) * 2048.f);
    t.w1 = round_short(f * 2048.f);
    return t;
}

WARP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the horizontal pass of one byte and the vertical pass of two such sums
WARP_HD int resize_h(int v0, int v1, const Tap& a) { return v0 * a.w0 + v1 * a.w1; }
WARP_HD int resize_v(int h0, int h1, const Tap& b) { return (((b.w0 * (h0 >> 4)) >> 16) + ((b.w1 * (h1 >> 4)) >> 16) + 2) >> 2; }
WARP_HD int area2(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

// ---- warpAffine -------------------------------------------------------------------------------------------------------------------
// cvRound(double) for values inside int32 (others are outside the domain: clamped, so that nothing is undefined)
WARP_HD int round_i32(double v)
{
    const double r = rint(v);
    return !(r >= -2147483648.0) ? INT32_MIN : r >= 2147483647.0 ? INT32_MAX : (int)r;
}

// getRotationMatrix2D: the centre as float32, the rest in double
WARP_HD void rotation_matrix_2d(double cx, double cy, double angle, double scale, double* M)
{
    const double x = (double)(float)cx, y = (double)(float)cy;
    const double a = angle * 3.14159265358979323846 / 180.0;
    const double alpha = cos(a) * scale, beta = sin(a) * scale;
    M[0] = alpha;
    M[1] = beta;
    M[2] = (1 - alpha) * x - beta * y;
    M[3] = -beta;
    M[4] = alpha;
    M[5] = beta * x + (1 - alpha) * y;
}

// the forward matrix F -> the map from destination to source, step by step as OpenCV's invertAffineTransform-in-place does
WARP_HD void invert_affine(const double* F, double* M)
{
    double D = F[0] * F[4] - F[1] * F[3];
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = F[4] * D, A22 = F[0] * D;
    M[0] = A11;
    M[1] = F[1] * (-D);
    M[3] = F[3] * (-D);
    M[4] = A22;
    M[2] = -M[0] * F[2] - M[1] * F[5];
    M[5] = -M[3] * F[2] - M[4] * F[5];
}

// the per-column and per-row parts of the fixed-point source position (10 fractional bits, then 5 kept)
WARP_HD int col_delta(double m, int x) { return round_i32(m * (double)x * 1024.0); }
WARP_HD long long row_base(double m, double b, int y) { return (long long)round_i32((m * (double)y + b) * 1024.0) + 16; }

struct Pos {
    int ix, iy;  // integer position, saturated to int16
    int fx, fy;  // fractions, 5 bits
};
WARP_HD Pos position(long long X0, long long Y0, int ad, int bd)   // (64-bit sums: a matrix outside the domain cannot overflow them)
{
    const long long X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5;
    const long long ix = X >> 5, iy = Y >> 5;
    Pos p;
    p.ix = (int)(ix < -32768 ? -32768 : ix > 32767 ? 32767 : ix);
    p.iy = (int)(iy < -32768 ? -32768 : iy > 32767 ? 32767 : iy);
    p.fx = (int)(X & 31);
    p.fy = (int)(Y & 31);
    return p;
}
// the four taps v00 (ix, iy), v01 (ix + 1, iy), v10 (ix, iy + 1), v11; a tap outside the source is 0
WARP_HD int blend(int v00, int v01, int v10, int v11, int fx, int fy)
{
    return (v00 * (32 - fx) * (32 - fy) + v01 * fx * (32 - fy) + v10 * (32 - fx) * fy + v11 * fx * fy + 512) >> 10;
}

// ---- one byte at a time: the definition in C++, for host tests; the kernels restate these loops per tile ---------------------------
// byte c of pixel (x, y), 0 outside the image
WARP_HD int tap_at(const uint8_t* src, int sw, int sh, int C, long long pitch, int x, int y, int c)
{
    return (x >= 0 && x < sw && y >= 0 && y < sh) ? src[(long long)y * pitch + (long long)x * C + c] : 0;
}

inline void resize_image(const uint8_t* src, int sw, int sh, int C, long long sp, uint8_t* dst, int dw, int dh, long long dp)
{
    if (is_area2(sw, sh, dw, dh)) {
        for (int y = 0; y < dh; y++)
            for (int x = 0; x < dw; x++)
                for (int c = 0; c < C; c++) {
                    const uint8_t* r0 = src + (long long)(2 * y) * sp + (long long)(2 * x) * C + c;
                    dst[(long long)y * dp + (long long)x * C + c] = (uint8_t)area2(r0[0], r0[C], r0[sp], r0[sp + C]);
                }
        return;
    }
    const double scx = axis_scale(dw, sw), scy = axis_scale(dh, sh);
    for (int y = 0; y < dh; y++) {
        const Tap b = axis_tap(y, scy, sh, false);
        const uint8_t* r0 = src + (long long)clampi(b.s, 0, sh - 1) * sp;
        const uint8_t* r1 = src + (long long)clampi(b.s + 1, 0, sh - 1) * sp;
        for (int x = 0; x < dw; x++) {
            const Tap a = axis_tap(x, scx, sw, true);
            const long long o0 = (long long)a.s * C, o1 = (long long)(a.s + 1 < sw ? a.s + 1 : a.s) * C;
            for (int c = 0; c < C; c++)
                dst[(long long)y * dp + (long long)x * C + c] =
                    (uint8_t)resize_v(resize_h(r0[o0 + c], r0[o1 + c], a), resize_h(r1[o0 + c], r1[o1 + c], a), b);
        }
    }
}

inline void warp_affine_image(const uint8_t* src, int sw, int sh, int C, long long sp, const double* F, uint8_t* dst, int dw, int dh,
                              long long dp)
{
    double M[6];
    invert_affine(F, M);
    for (int y = 0; y < dh; y++) {
        const long long X0 = row_base(M[1], M[2], y), Y0 = row_base(M[4], M[5], y);
        for (int x = 0; x < dw; x++) {
            const Pos p = position(X0, Y0, col_delta(M[0], x), col_delta(M[3], x));
            for (int c = 0; c < C; c++)
                dst[(long long)y * dp + (long long)x * C + c] =
                    (uint8_t)blend(tap_at(src, sw, sh, C, sp, p.ix, p.iy, c), tap_at(src, sw, sh, C, sp, p.ix + 1, p.iy, c),
                                   tap_at(src, sw, sh, C, sp, p.ix, p.iy + 1, c), tap_at(src, sw, sh, C, sp, p.ix + 1, p.iy + 1, c), p.fx,
                                   p.fy);
        }
    }
}

}  // namespace warp
