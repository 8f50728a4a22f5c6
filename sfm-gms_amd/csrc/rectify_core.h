// rectify_core.h -- a posed pair made readable for the stereo matchers, and a disparity map made into points: the
// rectifying plan of a pair (two rotations and one new camera), the map from a rectified pixel to a source position with the
// distortion model applied, and the reprojection of a disparity into the frame of the pair's sparse points. The library's own
// definition; it follows cv::stereoRectify, initUndistortRectifyMap, remap and reprojectImageTo3D in structure only. What the kernels
// (rectify_kernels.hip), the C ABI (capi_image.cpp) and the host test build (tests/cpp/rectify_host.cpp) share; tests/rectify_ref.py
// states the same in numpy. fp64, only + - * / sqrt rint, every sum in the order written here, built with -ffp-contract=off: the GPU,
// the host and numpy agree bit for bit. No sin / cos / acos: the device's are not the host's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gms.h"
#include "twoview_core.h"
#include "warp_core.h"

#if defined(__HIPCC__)
#define RECT_HD __host__ __device__ inline
#else
#define RECT_HD inline
#endif

namespace rect {

using gms::tv::Camera;

constexpr int kMaxSide = warp::kMaxSide;
constexpr int kScanBlock = 1024;  // pixels per workgroup of the cloud's ordered compaction: 256 lanes x 4 adjacent pixels

RECT_HD Camera camera_of(const gms_camera& c) { return Camera{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3}; }

// the sizes and layouts stated here (the others are GMS_ERR_BAD_ARG)
RECT_HD bool image_args_ok(int n, int sw, int sh, int channels, long long src_pitch, int dw, int dh, long long dst_pitch)
{
    return warp::args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch);
}

RECT_HD double absd(double v) { return v < 0 ? -v : v; }

// C = A B, c = A v, c = A^T v: each entry a sum of three products, added left to right
RECT_HD void mul33(const double* A, const double* B, double* C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
RECT_HD void mul3v(const double* A, const double* v, double* o)
{
    for (int r = 0; r < 3; ++r) o[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
RECT_HD void mul3tv(const double* A, const double* v, double* o)
{
    for (int c = 0; c < 3; ++c) o[c] = A[c] * v[0] + A[3 + c] * v[1] + A[6 + c] * v[2];
}

RECT_HD void zero_plan(gms_rectify_plan& p, int status)
{
    for (int i = 0; i < 9; ++i) p.R1[i] = p.R2[i] = 0.0;
    p.fx = p.fy = p.cx = p.cy = p.B = 0.0;
    p.out_w = p.out_h = p.turn = 0;
    p.status = status;
}

// the mean of the four source corners of one camera, undistorted, turned by Rk and projected; false: a corner is not in front
RECT_HD bool corner_mean(const Camera& cam, const double* Rk, int W, int H, double& mx, double& my)
{
    const double cu[4] = {0.0, (double)(W - 1), (double)(W - 1), 0.0}, cv[4] = {0.0, 0.0, (double)(H - 1), (double)(H - 1)};
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < 4; ++i) {
        double v[3], p[3];
        gms::tv::undistort_point(cam, cu[i], cv[i], v[0], v[1]);
        v[2] = 1.0;
        mul3v(Rk, v, p);
        if (!(p[2] > 0.0)) return false;
        const double x = p[0] / p[2], y = p[1] / p[2];
        sx += x;
        sy += y;
    }
    mx = sx * 0.25;
    my = sy * 0.25;
    return true;
}

// The plan of the pair X2 = R X1 + t seen by `cam` in W x H images. out_w / out_h <= 0: the default size, (W, H), or (H, W) for the
// quarter turns. Not rectifiable (a zeroed plan, GMS_ERR_NO_MODEL): a relative rotation of 90 degrees or more, a baseline more than
// 45 degrees out of the turned image plane, or a source corner that is not in front of its rectified camera.
RECT_HD void make_plan(const Camera& cam, const double* R, const double* t, int W, int H, int out_w, int out_h, gms_rectify_plan& P)
{
    zero_plan(P, GMS_ERR_NO_MODEL);
    // R^(-1/2): the conjugate of the half-angle quaternion
    const double tr = R[0] + R[4] + R[8];
    if (!(tr > 0.0)) return;
    const double w = sqrt(1.0 + tr) / 2.0, d4 = 4.0 * w;
    const double x0 = (R[7] - R[5]) / d4, y0 = (R[2] - R[6]) / d4, z0 = (R[3] - R[1]) / d4, w0 = 1.0 + w;
    const double qn = sqrt(w0 * w0 + x0 * x0 + y0 * y0 + z0 * z0);
    const double qw = w0 / qn, qx = x0 / qn, qy = y0 / qn, qz = z0 / qn;
    double Rh[9];
    Rh[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
    Rh[1] = 2.0 * (qx * qy + qw * qz);
    Rh[2] = 2.0 * (qx * qz - qw * qy);
    Rh[3] = 2.0 * (qx * qy - qw * qz);
    Rh[4] = 1.0 - 2.0 * (qx * qx + qz * qz);
    Rh[5] = 2.0 * (qy * qz + qw * qx);
    Rh[6] = 2.0 * (qx * qz + qw * qy);
    Rh[7] = 2.0 * (qy * qz - qw * qx);
    Rh[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    // the baseline in the half-way frame, and the quarter turn that brings it nearest +x
    double rt[3], b[3], g[3];
    mul3v(Rh, t, rt);
    for (int i = 0; i < 3; ++i) b[i] = -rt[i];
    int turn;
    if (absd(b[0]) >= absd(b[1]))
        turn = b[0] > 0.0 ? 0 : 1;
    else
        turn = b[1] > 0.0 ? 2 : 3;
    double Z[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1.0};
    if (turn == 0) Z[0] = 1.0, Z[4] = 1.0;
    if (turn == 1) Z[0] = -1.0, Z[4] = -1.0;
    if (turn == 2) Z[1] = 1.0, Z[3] = -1.0;
    if (turn == 3) Z[1] = -1.0, Z[3] = 1.0;
    mul3v(Z, b, g);
    if (!(g[0] > 0.0) || !(g[0] >= absd(g[2]))) return;
    const double B = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    // the rotation that takes the baseline's direction onto +x about the axis perpendicular to both
    const double ay = g[1] / B, az = g[2] / B, h = 1.0 + g[0] / B;
    double A[9], Wm[9];
    A[0] = 1.0 - (ay * ay + az * az) / h;
    A[1] = ay;
    A[2] = az;
    A[3] = -ay;
    A[4] = 1.0 - (ay * ay) / h;
    A[5] = -(ay * az) / h;
    A[6] = -az;
    A[7] = -(ay * az) / h;
    A[8] = 1.0 - (az * az) / h;
    mul33(A, Z, Wm);
    double R1[9], R2[9];
    mul33(Wm, Rh, R2);
    mul33(R2, R, R1);
    // the new camera: both principal points from the corners' means, then shared, so that a point at infinity has disparity 0
    const int ow = out_w > 0 && out_h > 0 ? out_w : turn < 2 ? W : H, oh = out_w > 0 && out_h > 0 ? out_h : turn < 2 ? H : W;
    const double f = cam.fx < cam.fy ? cam.fx : cam.fy;
    double m1x, m1y, m2x, m2y;
    if (!corner_mean(cam, R1, W, H, m1x, m1y) || !corner_mean(cam, R2, W, H, m2x, m2y)) return;
    const double hx = (double)(ow - 1) / 2.0, hy = (double)(oh - 1) / 2.0;
    const double c1x = hx - f * m1x, c1y = hy - f * m1y, c2x = hx - f * m2x, c2y = hy - f * m2y;
    for (int i = 0; i < 9; ++i) {
        P.R1[i] = R1[i];
        P.R2[i] = R2[i];
    }
    P.fx = P.fy = f;
    P.cx = (c1x + c2x) * 0.5;
    P.cy = (c1y + c2y) * 0.5;
    P.B = B;
    P.out_w = ow;
    P.out_h = oh;
    P.turn = turn;
    P.status = GMS_OK;
}

// cv::undistort as a plan: no rotation, the new camera equal to the camera
RECT_HD void identity_plan(const Camera& cam, int W, int H, gms_rectify_plan& P)
{
    zero_plan(P, GMS_OK);
    P.R1[0] = P.R1[4] = P.R1[8] = P.R2[0] = P.R2[4] = P.R2[8] = 1.0;
    P.fx = cam.fx;
    P.fy = cam.fy;
    P.cx = cam.cx;
    P.cy = cam.cy;
    P.out_w = W;
    P.out_h = H;
}

// ---- a rectified pixel -> its source position ------------------------------------------------------------------------------------------
// The ray of destination pixel (u, v) under rotation Rk is Rk^T ((u - cx') / fx', (v - cy') / fy', 1) = col(u) + row(v):
//   col = (Rk[0], Rk[1], Rk[2]) xn          row = (Rk[3] yn + Rk[6], Rk[4] yn + Rk[7], Rk[5] yn + Rk[8])
// so that a tile works out the column part once per column and the row part once per row.
RECT_HD double norm_coord(int u, double c, double f) { return ((double)u - c) / f; }
RECT_HD void col_terms(const double* Rk, double xn, double* o) { o[0] = Rk[0] * xn, o[1] = Rk[1] * xn, o[2] = Rk[2] * xn; }
RECT_HD void row_terms(const double* Rk, double yn, double* o) { o[0] = Rk[3] * yn + Rk[6], o[1] = Rk[4] * yn + Rk[7], o[2] = Rk[5] * yn + Rk[8]; }

struct Src {
    int ix, iy;  // integer position, saturated to int16
    int fx, fy;  // fractions, 5 bits
    int front;   // 0: the ray does not point into the source camera (the byte is 0, valid 0)
};
RECT_HD int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
RECT_HD Src source_pos(const Camera& cam, const double* col, const double* row)
{
    Src s = {0, 0, 0, 0, 0};
    const double r0 = col[0] + row[0], r1 = col[1] + row[1], r2 = col[2] + row[2];
    if (!(r2 > 0.0)) return s;
    const double x = r0 / r2, y = r1 / r2, rr = x * x + y * y;
    const double kr = 1.0 + ((cam.k3 * rr + cam.k2) * rr + cam.k1) * rr;
    const double xd = x * kr + 2.0 * cam.p1 * x * y + cam.p2 * (rr + 2.0 * x * x);
    const double yd = y * kr + cam.p1 * (rr + 2.0 * y * y) + 2.0 * cam.p2 * x * y;
    const int SX = warp::round_i32((cam.fx * xd + cam.cx) * 32.0), SY = warp::round_i32((cam.fy * yd + cam.cy) * 32.0);
    s.ix = sat16(SX >> 5);
    s.iy = sat16(SY >> 5);
    s.fx = SX & 31;
    s.fy = SY & 31;
    s.front = 1;
    return s;
}
// byte c of the rectified pixel: warp_core.h's blend of the four taps, a tap outside the source 0 (every tap is bounds-checked before
// its address is formed); and whether all four taps are inside
RECT_HD int sample(const uint8_t* src, int sw, int sh, int C, long long pitch, const Src& s, int c)
{
    if (!s.front) return 0;
    return warp::blend(warp::tap_at(src, sw, sh, C, pitch, s.ix, s.iy, c), warp::tap_at(src, sw, sh, C, pitch, s.ix + 1, s.iy, c),
                       warp::tap_at(src, sw, sh, C, pitch, s.ix, s.iy + 1, c), warp::tap_at(src, sw, sh, C, pitch, s.ix + 1, s.iy + 1, c),
                       s.fx, s.fy);
}
RECT_HD int all_taps_inside(const Src& s, int sw, int sh) { return s.front && s.ix >= 0 && s.ix + 1 < sw && s.iy >= 0 && s.iy + 1 < sh; }

// ---- the definition one image at a time, for the host tests; the kernel restates the loops per tile -------------------------------------
inline void rectify_image(const uint8_t* src, int sw, int sh, int C, long long sp, const Camera& cam, const gms_rectify_plan& P, int which,
                          uint8_t* dst, int dw, int dh, long long dp, uint8_t* valid)
{
    const double* Rk = which == 2 ? P.R2 : P.R1;
    for (int v = 0; v < dh; ++v) {
        double row[3], col[3];
        row_terms(Rk, norm_coord(v, P.cy, P.fy), row);
        for (int u = 0; u < dw; ++u) {
            col_terms(Rk, norm_coord(u, P.cx, P.fx), col);
            Src s = {0, 0, 0, 0, 0};
            if (P.status == GMS_OK) s = source_pos(cam, col, row);
            for (int c = 0; c < C; ++c) dst[(long long)v * dp + (long long)u * C + c] = (uint8_t)sample(src, sw, sh, C, sp, s, c);
            if (valid) valid[(long long)v * dw + u] = (uint8_t)all_taps_inside(s, sw, sh);
        }
    }
}

// ---- a disparity -> a point -------------------------------------------------------------------------------------------------------------
// a pixel is a point when its disparity is not the matcher's FILTERED code, is at least min_disp16 (>= 1) and its valid byte is set
RECT_HD bool is_point(int d16, int filtered16, int min_disp16, int valid) { return d16 != filtered16 && d16 >= min_disp16 && valid != 0; }

// The point of rectified pixel (u, v) with disparity d16 / 16, in camera 1's frame and the unit of t (the pair's sparse points3d);
// with a registration (S > 0 and the view G of frame_a) in the world frame, as gms_sfm_register_device defines d_points_world.
RECT_HD void cloud_point(const gms_rectify_plan& P, int u, int v, int d16, const double* S, const gms_sfm_view* G, float* xyz)
{
    const double Zc = P.fx * P.B * 16.0 / (double)d16;
    double c[3], p[3];
    c[0] = ((double)u - P.cx) * Zc / P.fx;
    c[1] = ((double)v - P.cy) * Zc / P.fx;
    c[2] = Zc;
    mul3tv(P.R1, c, p);
    if (G) {
        double q[3];
        for (int i = 0; i < 3; ++i) q[i] = *S * p[i] - G->t[i];
        mul3tv(G->R, q, p);
    }
    for (int i = 0; i < 3; ++i) xyz[i] = (float)p[i];
}

// reprojectImageTo3D's Q for disparities in pixels (d16 / 16): (X, Y, Z, W) = Q (u, v, d, 1), the point (X, Y, Z) / W in the rectified
// camera 1's frame
inline void plan_q(const gms_rectify_plan& P, double* Q)
{
    for (int i = 0; i < 16; ++i) Q[i] = 0.0;
    Q[0] = Q[5] = 1.0;
    Q[3] = -P.cx;
    Q[7] = -P.cy;
    Q[11] = P.fx;
    Q[14] = P.B != 0.0 ? 1.0 / P.B : 0.0;
}

}  // namespace rect
