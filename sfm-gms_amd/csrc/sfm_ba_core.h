// sfm_ba_core.h -- bundle adjustment behind the registration: the arithmetic of one observation -- residual, the
// 2 x 6 and 2 x 3 Jacobians, Huber's weight and cost -- Rodrigues' formula, the closed-form symmetric 3 x 3 inverse, the 6 x 6 Cholesky
// solve and one ray's share of a re-triangulation. What the kernels (sfm_ba_kernels.hip) and the host build
// (tests/cpp/sfm_ba_host.cpp) share; tests/sfm_ba_ref.py states the same in numpy. This is the library's own definition: the reference
// stops at one pair (SfMUtil.cpp:4-83).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gms.h"

#if defined(__HIPCC__)
#define SBA_HD __host__ __device__ inline
#else
#define SBA_HD inline
#endif

namespace sba {

// gms_sfm_ba track statuses
constexpr int32_t kRefined = 0, kMulti = 1, kFew = 2, kKept = 3;

SBA_HD bool finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// Pc = R X + t; active when finite and in front; r = f (pi(Pc) - (u, v)), 0 when inactive
SBA_HD bool residual(const double* R, const double* t, const double* X, double u, double v, double f, double* Pc, double* r)
{
    for (int i = 0; i < 3; i++) Pc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
    const bool active = finite3(Pc) && Pc[2] > 0.0;
    r[0] = r[1] = 0.0;
    if (active) {
        const double iz = 1.0 / Pc[2];
        r[0] = f * (Pc[0] * iz - u);
        r[1] = f * (Pc[1] * iz - v);
    }
    return active;
}

// Jc [2][6] = dr / d(omega, tau) for R <- exp([omega]x) R, t <- t + tau; Jp [2][3] = dr / dX. For an active observation.
SBA_HD void jacobians(const double* R, const double* t, const double* Pc, double f, double* Jc, double* Jp)
{
    const double iz = 1.0 / Pc[2];
    const double x = Pc[0] * iz, y = Pc[1] * iz;
    const double D[2][3] = {{f * iz, 0.0, -f * x * iz}, {0.0, f * iz, -f * y * iz}};
    const double a[3] = {Pc[0] - t[0], Pc[1] - t[1], Pc[2] - t[2]};  // R X
    for (int k = 0; k < 2; k++) {
        Jc[6 * k + 0] = D[k][2] * a[1] - D[k][1] * a[2];
        Jc[6 * k + 1] = D[k][0] * a[2] - D[k][2] * a[0];
        Jc[6 * k + 2] = D[k][1] * a[0] - D[k][0] * a[1];
        Jc[6 * k + 3] = D[k][0];
        Jc[6 * k + 4] = D[k][1];
        Jc[6 * k + 5] = D[k][2];
        for (int c = 0; c < 3; c++) Jp[3 * k + c] = D[k][0] * R[c] + D[k][1] * R[3 + c] + D[k][2] * R[6 + c];
    }
}

// Huber at h px (h <= 0: none): the weight w and the cost rho of a residual
SBA_HD void huber(const double* r, double h, double& w, double& rho)
{
    const double n2 = r[0] * r[0] + r[1] * r[1];
    const double n = sqrt(n2);
    w = 1.0;
    rho = n2;
    if (h > 0.0 && n > h) {
        w = h / n;
        rho = 2.0 * h * n - h * h;
    }
}

// E = exp([w]x) = I + A [w]x + B [w]x^2
SBA_HD void rodrigues(const double* w, double* E)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A = 1.0, B = 0.5;
    if (th2 >= 1e-20) {
        const double th = sqrt(th2);
        const double h = sin(0.5 * th) / (0.5 * th);
        A = sin(th) / th;
        B = 0.5 * h * h;
    }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double kk = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
            E[3 * r + c] = (r == c ? 1.0 : 0.0) + A * K[3 * r + c] + B * kk;
        }
}
SBA_HD void mat3_mul(const double* A, const double* B, double* C)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// The inverse of the symmetric V (row-major 3 x 3): adjugate over determinant. Zeros, and false, when the determinant is not a
// positive finite number or an entry of the inverse is not finite.
SBA_HD bool inv3_sym(const double* V, double* I)
{
    const double a = V[0], b = V[1], c = V[2], d = V[4], e = V[5], f = V[8];
    const double A = d * f - e * e, B = c * e - b * f, C = b * e - c * d;
    const double det = a * A + b * B + c * C;
    I[0] = A / det;
    I[1] = I[3] = B / det;
    I[2] = I[6] = C / det;
    I[4] = (a * f - c * c) / det;
    I[5] = I[7] = (b * c - a * e) / det;
    I[8] = (a * d - b * b) / det;
    bool ok = isfinite(det) && det > 0.0;
    for (int k = 0; k < 9; k++) ok = ok && isfinite(I[k]);
    if (!ok)
        for (int k = 0; k < 9; k++) I[k] = 0.0;
    return ok;
}
SBA_HD void mat3_vec(const double* M, const double* v, double* o)
{
    for (int r = 0; r < 3; r++) o[r] = M[3 * r] * v[0] + M[3 * r + 1] * v[1] + M[3 * r + 2] * v[2];
}

// The lower Cholesky factor of the symmetric M (row-major 6 x 6); false when a pivot is not a positive finite number.
SBA_HD bool chol6(const double* M, double* L)
{
    for (int k = 0; k < 36; k++) L[k] = 0.0;
    for (int j = 0; j < 6; j++) {
        double s = M[6 * j + j];
        for (int k = 0; k < j; k++) s = s - L[6 * j + k] * L[6 * j + k];
        if (!(isfinite(s) && s > 0.0)) return false;
        L[6 * j + j] = sqrt(s);
        for (int i = j + 1; i < 6; i++) {
            double v = M[6 * i + j];
            for (int k = 0; k < j; k++) v = v - L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = v / L[6 * j + j];
        }
    }
    return true;
}
SBA_HD void chol6_solve(const double* L, const double* b, double* x)
{
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - L[6 * i + k] * y[k];
        y[i] = s / L[6 * i + i];
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < 6; k++) s = s - L[6 * k + i] * x[k];
        x[i] = s / L[6 * i + i];
    }
}

// One observation's share of a re-triangulation: A += I - d d^T, b += (I - d d^T) c, with c = -R^T t the camera's centre and
// d = R^T (u, v, 1) / |.| the ray, both in the world frame. A: row-major 3 x 3.
SBA_HD void ray_add(const double* R, const double* t, double u, double v, double* A, double* b)
{
    double c[3], d[3];
    for (int i = 0; i < 3; i++) {
        c[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
        d[i] = R[i] * u + R[3 + i] * v + R[6 + i];
    }
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int i = 0; i < 3; i++) d[i] = d[i] / n;
    double P[9];
    for (int r = 0; r < 3; r++)
        for (int k = 0; k < 3; k++) P[3 * r + k] = (r == k ? 1.0 : 0.0) - d[r] * d[k];
    for (int k = 0; k < 9; k++) A[k] += P[k];
    for (int r = 0; r < 3; r++) b[r] += P[3 * r] * c[0] + P[3 * r + 1] * c[1] + P[3 * r + 2] * c[2];
}

SBA_HD bool params_ok(const gms_sfm_ba_params& p)
{
    return p.n_iters >= 0 && p.n_cg >= 1 && isfinite(p.lambda0) && p.lambda0 >= 0.0 && isfinite(p.cg_tol) && p.cg_tol >= 0.0 &&
           isfinite(p.ftol) && p.ftol >= 0.0 && isfinite(p.huber_px) && p.huber_px >= 0.0;
}

}  // namespace sba
