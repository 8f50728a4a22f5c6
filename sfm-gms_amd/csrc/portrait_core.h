// portrait_core.h -- portrait mode's parameter check, neighbour numbering and border walk: what the C ABI
// (capi_image.cpp), the kernels (portrait_kernels.hip) and host tests share. tests/portrait_ref.py states the same in numpy.
#pragma once
#include <stdint.h>

#include "gms.h"

#if defined(__HIPCC__)
#define PM_HD __host__ __device__ inline
#else
#define PM_HD inline
#endif

namespace pm {

constexpr int kMaxContours = 64;

// the parameter sets and sizes stated here (the others are GMS_ERR_BAD_ARG)
PM_HD bool params_ok(const gms_portrait_params& p, int W, int H)
{
    return p.threshold >= 0 && p.threshold <= 255 && p.dilate_iterations >= 0 && p.dilate_iterations <= 8 && p.num_contours >= 1 &&
           p.num_contours <= kMaxContours && p.median_ksize >= 3 && p.median_ksize <= 31 && (p.median_ksize & 1) && W >= 1 &&
           W <= GMS_PORTRAIT_MAX_SIDE && H >= 1 && H <= GMS_PORTRAIT_MAX_SIDE;
}
PM_HD bool median_ok(int W, int H, int channels, int ksize)
{
    return (channels == 1 || channels == 3) && ksize >= 3 && ksize <= 31 && (ksize & 1) && W >= 1 && W <= GMS_PORTRAIT_MAX_SIDE &&
           H >= 1 && H <= GMS_PORTRAIT_MAX_SIDE;
}

// neighbour s of a pixel: 0 east, then counter-clockwise on the screen (1 north-east, 2 north, ..., 7 south-east)
PM_HD int dx(int s) { return (int8_t)(0x0100FFFFFF000101ull >> (8 * s)); }
PM_HD int dy(int s) { return (int8_t)(0x01010100FFFFFF00ull >> (8 * s)); }

// The Suzuki-Abe walk of one border on a plane of neighbour codes: bit s of nb[y * W + x] says that neighbour s of the non-zero pixel
// (x, y) is non-zero (neighbours outside the image are zero). The border starts at (x0, y0); hole = a hole border (the walk first
// looks clockwise from the east neighbour, which is zero) or an outer border (from the west neighbour). edge(x, y, xn, yn) sees every
// step of the closed chain, the step back to the start included; an isolated pixel gives edge(x0, y0, x0, y0) once. Returns the
// chain's doubled signed area.
template <typename Edge>
PM_HD long long walk_border(const uint8_t* nb, int W, int x0, int y0, bool hole, Edge edge)
{
    const unsigned c0 = nb[(long long)y0 * W + x0];
    if (c0 == 0) {
        edge(x0, y0, x0, y0);
        return 0;
    }
    int s = hole ? 0 : 4;
    do s = (s - 1) & 7;
    while (!((c0 >> s) & 1));
    const int x1 = x0 + dx(s), y1 = y0 + dy(s);
    int x = x0, y = y0;
    unsigned c = c0;
    long long a2 = 0;
    for (;;) {
        do s = (s + 1) & 7;
        while (!((c >> s) & 1));
        const int xn = x + dx(s), yn = y + dy(s);
        edge(x, y, xn, yn);
        a2 += (long long)x * yn - (long long)xn * y;
        if (xn == x0 && yn == y0 && x == x1 && y == y1) return a2;
        x = xn;
        y = yn;
        c = nb[(long long)y * W + x];
        s = (s + 4) & 7;
    }
}

}  // namespace pm
