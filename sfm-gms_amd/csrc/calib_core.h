// calib_core.h -- camera calibration from chessboard photographs: what the kernels (calib_kernels.hip), the C ABI
// (capi_calib.cpp) and the host test build (tests/cpp/calib_host.cpp) share. tests/calib_ref.py states the same in numpy.
//   corner candidates   an integer saddle response, its 17 x 17 peaks, the strongest of them: this library's own definition
//   order_board         the candidates onto the nx x ny grid, host only, fp64
//   subpix_refine       cv::cornerSubPix (OpenCV 4.5.2, read from its source) for one corner, fp64, host and device
//   calibrate_camera    closed-form start + Levenberg-Marquardt on the reprojection error, host only, fp64
// Built with -ffp-contract=off. Parity with an OpenCV build is unpinned.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CALIB_HD __host__ __device__ inline
#else
#define CALIB_HD inline
#endif

#include <algorithm>
#include <vector>

namespace calib {

constexpr int kBorder = 16;          // GMS_DETECT_BORDER: R = 0 closer than this to an edge
constexpr int kArm = 4;              // d of the second differences
constexpr int kNmsR = 8;             // peaks are maxima of 17 x 17
constexpr int kMaxCandidates = 4096;
constexpr int kMaxSide = 8192;       // so that a raster index fits 26 bits

// the bounds of the response: B <= 25 * 255, S <= 25 * 25 * 255; a second difference of S is at most 2 S_max in size
constexpr int64_t kSMax = 255 * 25 * 25, kDiffMax = 2 * kSMax;
static_assert(kSMax == 159375 && kDiffMax == 318750, "the stated bounds");
static_assert(kDiffMax * kDiffMax + 4 * kDiffMax * kDiffMax < (int64_t(1) << 39), "sxy^2 - 4 sxx syy stays below 2^39");
static_assert(((kDiffMax * kDiffMax + 4 * kDiffMax * kDiffMax) >> 10) < (int64_t(1) << 29), "R stays below 2^29: a uint32");

// R from the nine values of S it reads: (x, y), the four at +-d on the axes, the four at (+-d, +-d)
CALIB_HD uint32_t response_of(int s, int sxp, int sxm, int syp, int sym, int spp, int smm, int spm, int smp)
{
    const int64_t sxx = (int64_t)sxp + sxm - 2 * (int64_t)s, syy = (int64_t)syp + sym - 2 * (int64_t)s;
    const int64_t sxy = (int64_t)spp + smm - spm - smp;
    const int64_t v = sxy * sxy - 4 * sxx * syy;
    return (uint32_t)((v > 0 ? v : 0) >> 10);
}

CALIB_HD bool inner(int x, int y, int w, int h) { return x >= kBorder && y >= kBorder && x < w - kBorder && y < h - kBorder; }

// two peaks are more than 8 apart in x or in y: every 9 x 9 cell of the inner region holds at most one
CALIB_HD int64_t peak_capacity(int w, int h)
{
    if (w <= 2 * kBorder || h <= 2 * kBorder) return 0;
    return (int64_t)((w - 2 * kBorder + 8) / 9) * ((h - 2 * kBorder + 8) / 9);
}

// candidates in descending R, then raster order: the larger key comes first; keys of one image are distinct
CALIB_HD uint64_t rank_key(uint32_t r, uint32_t raster) { return ((uint64_t)r << 32) | (uint64_t)(0xffffffffu - raster); }

CALIB_HD bool batch_ok(int n, int w, int h, int max_candidates)
{
    return n >= 1 && n <= 65535 && w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide && max_candidates >= 1 &&
           max_candidates <= kMaxCandidates;
}

// ---- cornerSubPix: one corner ---------------------------------------------------------------------------------------------------------
// exp(-(i / 5)^2), i = -5 .. 5 (tests/calib_ref.py holds the same digits, so that no math library is asked)
constexpr int kWin = 5, kWinN = 2 * kWin + 1;
#if defined(__HIP_DEVICE_COMPILE__)
__device__
#endif
static const double kMask11[kWinN] = {0.36787944117144233, 0.52729242404304855, 0.69767632607103103, 0.85214378896621135,
                                      0.96078943915232320, 1.0, 0.96078943915232320, 0.85214378896621135,
                                      0.69767632607103103, 0.52729242404304855, 0.36787944117144233};
enum { kSubpixRefined = 0, kSubpixTooFar = 1, kSubpixLeftImage = 2, kSubpixSingular = 3 };

// whether the (2 win + 3)^2 patch of bilinear samples around (x, y) reads only pixels of the image
CALIB_HD bool subpix_window_ok(int w, int h, double x, double y)
{
    const double x0 = floor(x - (kWin + 1)), y0 = floor(y - (kWin + 1));
    return x0 >= 0 && y0 >= 0 && x0 + (2 * kWin + 3) <= w - 1 && y0 + (2 * kWin + 3) <= h - 1;
}

struct SubpixSampler {
    const uint8_t* p;   // the pixel under the patch's first sample
    long long pitch;
    double w00, w01, w10, w11;
    // getRectSubPix's sample (i, j) of the patch, i and j from 0
    CALIB_HD double at(int i, int j) const
    {
        const uint8_t* q = p + i * pitch + j;
        return ((double)q[0] * w00 + (double)q[1] * w01) + ((double)q[pitch] * w10 + (double)q[pitch + 1] * w11);
    }
};

// cv::cornerSubPix's loop for one corner: returns the status, (ox, oy) the corner, last the last squared shift
CALIB_HD int subpix_refine(const uint8_t* img, int w, int h, long long pitch, double sx, double sy, int max_iter, double eps, double& ox,
                           double& oy, double& last)
{
    double cx = sx, cy = sy, err = 0.0;
    int it = 0, status = kSubpixRefined;
    for (;;) {
        if (!subpix_window_ok(w, h, cx, cy)) {
            status = kSubpixLeftImage;
            break;
        }
        const double x0 = cx - (kWin + 1), y0 = cy - (kWin + 1);
        const double fx0 = floor(x0), fy0 = floor(y0), a = x0 - fx0, b = y0 - fy0;
        const SubpixSampler s{img + (long long)fy0 * pitch + (long long)fx0, pitch, (1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b};
        double A = 0, B = 0, C = 0, bb1 = 0, bb2 = 0;
        for (int i = 0; i < kWinN; ++i) {
            const double py = i - kWin;
            for (int j = 0; j < kWinN; ++j) {
                const double m = kMask11[i] * kMask11[j];
                const double tgx = s.at(i + 1, j + 2) - s.at(i + 1, j), tgy = s.at(i + 2, j + 1) - s.at(i, j + 1);
                const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m, px = j - kWin;
                A += gxx;
                B += gxy;
                C += gyy;
                bb1 += gxx * px + gxy * py;
                bb2 += gxy * px + gyy * py;
            }
        }
        const double det = A * C - B * B;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) {
            status = kSubpixSingular;
            break;
        }
        const double scale = 1.0 / det;
        const double nx = cx + C * scale * bb1 - B * scale * bb2, ny = cy - B * scale * bb1 + A * scale * bb2;
        err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy);
        cx = nx;
        cy = ny;
        if (!(++it < max_iter && err > eps * eps)) break;
    }
    last = err;
    if (status == kSubpixLeftImage) {
        cx = sx;
        cy = sy;
    } else if (fabs(cx - sx) > kWin || fabs(cy - sy) > kWin) {
        cx = sx;
        cy = sy;
        status = kSubpixTooFar;
    }
    ox = cx;
    oy = cy;
    return status;
}

CALIB_HD bool subpix_args_ok(int w, int h, int win, int max_iter, double eps)
{
    return win == kWin && w >= 2 * kWin + 4 && h >= 2 * kWin + 4 && w <= kMaxSide && h <= kMaxSide && max_iter >= 1 && eps >= 0.0;
}

// ======== host only ====================================================================================================================
struct Candidate { int32_t x, y; uint32_t response; };

// ---- the candidates of one image, from the definition (the kernels' counterpart for tests/cpp/calib_host.cpp) ---------------------
inline void response_image(const uint8_t* img, int w, int h, std::vector<uint32_t>& R)
{
    auto box5 = [w, h](const std::vector<int>& a) {
        std::vector<int> o((size_t)w * h, 0);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                int s = 0;
                for (int v = std::max(y - 2, 0); v <= std::min(y + 2, h - 1); ++v)
                    for (int u = std::max(x - 2, 0); u <= std::min(x + 2, w - 1); ++u) s += a[(size_t)v * w + u];
                o[(size_t)y * w + x] = s;
            }
        return o;
    };
    std::vector<int> I((size_t)w * h);
    for (size_t i = 0; i < I.size(); ++i) I[i] = img[i];
    const std::vector<int> S = box5(box5(I));
    R.assign((size_t)w * h, 0u);
    auto s = [&](int x, int y) { return S[(size_t)y * w + x]; };
    for (int y = kBorder; y < h - kBorder; ++y)
        for (int x = kBorder; x < w - kBorder; ++x)
            R[(size_t)y * w + x] = response_of(s(x, y), s(x + kArm, y), s(x - kArm, y), s(x, y + kArm), s(x, y - kArm), s(x + kArm, y + kArm),
                                               s(x - kArm, y - kArm), s(x + kArm, y - kArm), s(x - kArm, y + kArm));
}

inline bool is_peak(const std::vector<uint32_t>& R, int w, int h, int x, int y)
{
    const uint32_t r = R[(size_t)y * w + x];
    if (r == 0) return false;
    for (int dy = -kNmsR; dy <= kNmsR; ++dy)
        for (int dx = -kNmsR; dx <= kNmsR; ++dx) {
            const int u = x + dx, v = y + dy;
            if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= w || v >= h) continue;
            const uint32_t nb = R[(size_t)v * w + u];
            const bool earlier = dy < 0 || (dy == 0 && dx < 0);
            if (earlier ? r <= nb : r < nb) return false;
        }
    return true;
}

inline std::vector<Candidate> candidates(const uint8_t* img, int w, int h, int max_candidates)
{
    std::vector<uint32_t> R;
    response_image(img, w, h, R);
    std::vector<uint64_t> keys;
    for (int y = kBorder; y < h - kBorder; ++y)
        for (int x = kBorder; x < w - kBorder; ++x)
            if (is_peak(R, w, h, x, y)) keys.push_back(rank_key(R[(size_t)y * w + x], (uint32_t)(y * w + x)));
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    if ((int)keys.size() > max_candidates) keys.resize((size_t)max_candidates);
    std::vector<Candidate> out;
    for (uint64_t k : keys) {
        const uint32_t raster = 0xffffffffu - (uint32_t)k;
        out.push_back({(int32_t)(raster % (uint32_t)w), (int32_t)(raster / (uint32_t)w), (uint32_t)(k >> 32)});
    }
    return out;
}

// ---- small dense linear algebra -------------------------------------------------------------------------------------------------------
// A x = b, Gaussian elimination with partial pivoting; A (n x n, row-major) and b are overwritten. false: singular
inline bool solve_linear(int n, std::vector<double>& A, std::vector<double>& b)
{
    for (int k = 0; k < n; ++k) {
        int piv = k;
        for (int i = k + 1; i < n; ++i)
            if (fabs(A[(size_t)i * n + k]) > fabs(A[(size_t)piv * n + k])) piv = i;
        if (A[(size_t)piv * n + k] == 0.0 || !std::isfinite(A[(size_t)piv * n + k])) return false;
        if (piv != k) {
            for (int j = 0; j < n; ++j) std::swap(A[(size_t)k * n + j], A[(size_t)piv * n + j]);
            std::swap(b[k], b[piv]);
        }
        for (int i = k + 1; i < n; ++i) {
            const double f = A[(size_t)i * n + k] / A[(size_t)k * n + k];
            if (f == 0.0) continue;
            for (int j = k; j < n; ++j) A[(size_t)i * n + j] -= f * A[(size_t)k * n + j];
            b[i] -= f * b[k];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        double s = b[k];
        for (int j = k + 1; j < n; ++j) s -= A[(size_t)k * n + j] * b[j];
        b[k] = s / A[(size_t)k * n + k];
    }
    return true;
}

// least squares by the normal equations: rows of m unknowns in `rows`, right sides in `rhs`
inline bool solve_normal(int m, const std::vector<double>& rows, const std::vector<double>& rhs, std::vector<double>& x)
{
    const size_t n = rhs.size();
    std::vector<double> N((size_t)m * m, 0.0);
    x.assign((size_t)m, 0.0);
    for (size_t r = 0; r < n; ++r)
        for (int i = 0; i < m; ++i) {
            const double ai = rows[r * m + i];
            if (ai == 0.0) continue;
            for (int j = 0; j < m; ++j) N[(size_t)i * m + j] += ai * rows[r * m + j];
            x[i] += ai * rhs[r];
        }
    return solve_linear(m, N, x);
}

struct P2 { double x, y; };

// the homography src -> dst with h33 = 1, least squares on the 2 n linear equations
inline bool fit_h(const std::vector<P2>& src, const std::vector<P2>& dst, double H[9])
{
    const size_t n = src.size();
    std::vector<double> rows(2 * n * 8, 0.0), rhs(2 * n), x;
    for (size_t i = 0; i < n; ++i) {
        double* a = &rows[i * 8];
        double* b = &rows[(n + i) * 8];
        a[0] = src[i].x; a[1] = src[i].y; a[2] = 1; a[6] = -dst[i].x * src[i].x; a[7] = -dst[i].x * src[i].y;
        b[3] = src[i].x; b[4] = src[i].y; b[5] = 1; b[6] = -dst[i].y * src[i].x; b[7] = -dst[i].y * src[i].y;
        rhs[i] = dst[i].x;
        rhs[n + i] = dst[i].y;
    }
    if (!solve_normal(8, rows, rhs, x)) return false;
    for (int i = 0; i < 8; ++i) H[i] = x[i];
    H[8] = 1.0;
    return true;
}

inline P2 apply_h(const double H[9], P2 p)
{
    const double z = H[6] * p.x + H[7] * p.y + H[8];
    return {(H[0] * p.x + H[1] * p.y + H[2]) / z, (H[3] * p.x + H[4] * p.y + H[5]) / z};
}

// points moved to their mean and divided by their mean distance from it; returns {cx, cy, s}
inline void normalise(const std::vector<P2>& p, std::vector<P2>& out, double& cx, double& cy, double& s)
{
    cx = cy = 0;
    for (const P2& q : p) { cx += q.x; cy += q.y; }
    cx /= (double)p.size();
    cy /= (double)p.size();
    s = 0;
    for (const P2& q : p) s += sqrt((q.x - cx) * (q.x - cx) + (q.y - cy) * (q.y - cy));
    s /= (double)p.size();
    if (!(s > 0)) s = 1.0;
    out.resize(p.size());
    for (size_t i = 0; i < p.size(); ++i) out[i] = {(p[i].x - cx) / s, (p[i].y - cy) / s};
}

// ---- ordering onto the board ------------------------------------------------------------------------------------------------------
// integer directions (a, b) of the rotated frames; the frame's axes are (a, b) and (-b, a)
constexpr int kFrames[10][2] = {{1, 0}, {5, 1}, {5, 2}, {5, 3}, {5, 4}, {1, 1}, {4, 5}, {3, 5}, {2, 5}, {1, 5}};
constexpr double kCellTol = 0.25;

// p: nx * ny points (x, y) -> true and `out` in findChessboardCorners' order (row by row, nx per row), or false. nx != ny.
inline bool order_board(const std::vector<P2>& p, int nx, int ny, std::vector<P2>& out)
{
    const int n = nx * ny;
    if (nx == ny || nx < 2 || ny < 2 || (int)p.size() != n) return false;
    // the four extreme points of the frame whose quadrilateral is largest, in integers
    std::vector<int64_t> X(n), Y(n);
    for (int i = 0; i < n; ++i) { X[i] = (int64_t)rint(p[i].x); Y[i] = (int64_t)rint(p[i].y); }
    int q[4] = {0, 0, 0, 0};
    int64_t best = -1;
    for (const auto& f : kFrames) {
        int c[4] = {0, 0, 0, 0};   // max a, max b, min a, min b: the first point on a tie
        for (int i = 1; i < n; ++i) {
            const int64_t a = f[0] * X[i] + f[1] * Y[i], b = -f[1] * X[i] + f[0] * Y[i];
            if (a > f[0] * X[c[0]] + f[1] * Y[c[0]]) c[0] = i;
            if (b > -f[1] * X[c[1]] + f[0] * Y[c[1]]) c[1] = i;
            if (a < f[0] * X[c[2]] + f[1] * Y[c[2]]) c[2] = i;
            if (b < -f[1] * X[c[3]] + f[0] * Y[c[3]]) c[3] = i;
        }
        int64_t area2 = 0;
        for (int i = 0; i < 4; ++i) area2 += X[c[i]] * Y[c[(i + 1) & 3]] - X[c[(i + 1) & 3]] * Y[c[i]];
        if (area2 < 0) area2 = -area2;
        if (area2 > best) {
            best = area2;
            for (int i = 0; i < 4; ++i) q[i] = c[i];
        }
    }
    if (best <= 0 || q[0] == q[1] || q[0] == q[2] || q[0] == q[3] || q[1] == q[2] || q[1] == q[3] || q[2] == q[3]) return false;
    std::vector<P2> pn;
    double mx, my, ms;
    normalise(p, pn, mx, my, ms);
    P2 quad[4] = {pn[q[0]], pn[q[1]], pn[q[2]], pn[q[3]]};
    double sg = 0;
    for (int i = 0; i < 4; ++i) sg += quad[i].x * quad[(i + 1) & 3].y - quad[(i + 1) & 3].x * quad[i].y;
    if (sg < 0) { std::swap(quad[0], quad[3]); std::swap(quad[1], quad[2]); }   // (c): the grid's corners run with positive area
    const std::vector<P2> grid = {{0, 0}, {(double)nx - 1, 0}, {(double)nx - 1, (double)ny - 1}, {0, (double)ny - 1}};
    bool found = false;
    std::vector<P2> cand((size_t)n), node((size_t)n);
    std::vector<int> idx((size_t)n), seen((size_t)n);
    for (int s = 0; s < 4; ++s) {
        double H[9];
        const std::vector<P2> src = {quad[s & 3], quad[(s + 1) & 3], quad[(s + 2) & 3], quad[(s + 3) & 3]};
        if (!fit_h(src, grid, H)) continue;
        bool ok = true;
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < n && ok; ++i) {
            const P2 g = apply_h(H, pn[i]);
            node[i] = {floor(g.x + 0.5), floor(g.y + 0.5)};
            ok = node[i].x >= 0 && node[i].x <= nx - 1 && node[i].y >= 0 && node[i].y <= ny - 1;   // (false for NaN)
            if (ok) {
                idx[i] = (int)node[i].y * nx + (int)node[i].x;
                ok = !seen[idx[i]];   // (a) one to one
                seen[idx[i]] = 1;
            }
        }
        if (!ok) continue;
        double Hall[9];
        if (!fit_h(pn, node, Hall)) continue;
        for (int i = 0; i < n && ok; ++i) {   // (b) within a quarter cell of its node, each axis
            const P2 g = apply_h(Hall, pn[i]);
            ok = fabs(g.x - node[i].x) <= kCellTol && fabs(g.y - node[i].y) <= kCellTol;
        }
        if (!ok) continue;
        for (int i = 0; i < n; ++i) cand[idx[i]] = p[i];
        const double e1x = cand[1].x - cand[0].x, e1y = cand[1].y - cand[0].y, e2x = cand[nx].x - cand[0].x, e2y = cand[nx].y - cand[0].y;
        if (!(e1x * e2y - e1y * e2x > 0)) continue;   // (c) right-handed
        // of the two half turns, the one whose first point is smaller in (y, x)
        if (!found || cand[0].y < out[0].y || (cand[0].y == out[0].y && cand[0].x < out[0].x)) out = cand;
        found = true;
    }
    return found;
}

// ---- calibrateCamera ------------------------------------------------------------------------------------------------------------------
inline void rodrigues(const double r[3], double R[9])
{
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    double k[3] = {r[0], r[1], r[2]}, s = 1.0, c = 0.0;   // th < 1e-12: I + [r]x
    if (th >= 1e-12) {
        for (double& v : k) v /= th;
        s = sin(th);
        c = 1 - cos(th);
    }
    const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0;
            for (int l = 0; l < 3; ++l) kk += K[i * 3 + l] * K[l * 3 + j];
            R[i * 3 + j] = (i == j ? 1.0 : 0.0) + s * K[i * 3 + j] + c * kk;
        }
}

// by way of the unit quaternion with the largest component taken first: angles near pi lose nothing
inline void rodrigues_inv(const double R[9], double r[3])
{
    const double t[4] = {R[0] + R[4] + R[8], R[0] - R[4] - R[8], R[4] - R[0] - R[8], R[8] - R[0] - R[4]};
    int k = 0;
    for (int i = 1; i < 4; ++i)
        if (t[i] > t[k]) k = i;
    const double s = 2 * sqrt(1 + t[k]);
    double q[4];
    if (k == 0) { q[0] = s / 4; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s; }
    else if (k == 1) { q[0] = (R[7] - R[5]) / s; q[1] = s / 4; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s; }
    else if (k == 2) { q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = s / 4; q[3] = (R[5] + R[7]) / s; }
    else { q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = s / 4; }
    if (q[0] < 0)
        for (double& v : q) v = -v;
    const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double f = n < 1e-300 ? 0.0 : 2 * atan2(n, q[0]) / n;
    for (int i = 0; i < 3; ++i) r[i] = q[i + 1] * f;
}

struct P3 { double x, y, z; };

// intr (fx, fy, cx, cy), dist (k1, k2, p1, p2, k3): the model gms_triangulate_device undoes
inline P2 project(const P3& o, const double R[9], const double t[3], const double* intr, const double* dist)
{
    const double X = R[0] * o.x + R[1] * o.y + R[2] * o.z + t[0], Y = R[3] * o.x + R[4] * o.y + R[5] * o.z + t[1],
                 Z = R[6] * o.x + R[7] * o.y + R[8] * o.z + t[2];
    const double x = X / Z, y = Y / Z, r2 = x * x + y * y;
    const double cd = 1 + ((dist[4] * r2 + dist[1]) * r2 + dist[0]) * r2;
    const double xd = x * cd + 2 * dist[2] * x * y + dist[3] * (r2 + 2 * x * x);
    const double yd = y * cd + dist[2] * (r2 + 2 * y * y) + 2 * dist[3] * x * y;
    return {intr[0] * xd + intr[2], intr[1] * yd + intr[3]};
}

inline void mat3_mul(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// plane -> image homography on normalised coordinates of both sides, scaled to h33 = 1
inline bool dlt_h(const std::vector<P2>& src, const std::vector<P2>& dst, double H[9])
{
    std::vector<P2> a, b;
    double ax, ay, as, bx, by, bs, Hn[9], T[9];
    normalise(src, a, ax, ay, as);
    normalise(dst, b, bx, by, bs);
    if (!fit_h(a, b, Hn)) return false;
    const double Ta[9] = {1 / as, 0, -ax / as, 0, 1 / as, -ay / as, 0, 0, 1}, Tbi[9] = {bs, 0, bx, 0, bs, by, 0, 0, 1};
    mat3_mul(Tbi, Hn, T);
    mat3_mul(T, Ta, H);
    for (int i = 0; i < 9; ++i) H[i] /= H[8] + 0.0;
    return std::isfinite(H[0]);
}

constexpr int kLmIters = 30;
constexpr double kLmStep = 1e-6;

struct Calibration {
    double K[9], dist[5], rms;
    std::vector<double> rvecs, tvecs;   // [n_views][3]
};

// obj / img: the views' points back to back, view v's are [off[v], off[v + 1]). tests/calib_ref.py: calibrate_camera
inline bool calibrate_camera(const std::vector<P3>& obj, const std::vector<P2>& img, const std::vector<int>& off, int width, int height,
                             Calibration& out)
{
    const int nv = (int)off.size() - 1;
    if (nv < 1 || obj.size() != img.size() || off[0] != 0 || (size_t)off[nv] != obj.size()) return false;
    const int np = 9 + 6 * nv, total = off[nv];
    std::vector<double> p((size_t)np, 0.0), Hs((size_t)nv * 9);
    // the start: homographies; the principal point at the centre; fx, fy from each view's vanishing directions, least squares
    const double cx = (width - 1) * 0.5, cy = (height - 1) * 0.5;
    std::vector<double> rows, rhs, f;
    for (int v = 0; v < nv; ++v) {
        if (off[v + 1] - off[v] < 4) return false;
        std::vector<P2> s, d(img.begin() + off[v], img.begin() + off[v + 1]);
        for (int i = off[v]; i < off[v + 1]; ++i) s.push_back({obj[i].x, obj[i].y});
        double* H = &Hs[(size_t)v * 9];
        if (!dlt_h(s, d, H)) return false;
        double G[9];
        for (int j = 0; j < 3; ++j) { G[j] = H[j] - H[6 + j] * cx; G[3 + j] = H[3 + j] - H[6 + j] * cy; G[6 + j] = H[6 + j]; }
        double hh[3], vv[3], d1[3], d2[3];
        for (int j = 0; j < 3; ++j) { hh[j] = G[j * 3]; vv[j] = G[j * 3 + 1]; d1[j] = (hh[j] + vv[j]) * 0.5; d2[j] = (hh[j] - vv[j]) * 0.5; }
        for (double* t : {hh, vv, d1, d2}) {
            const double nrm = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            for (int j = 0; j < 3; ++j) t[j] /= nrm;
        }
        rows.insert(rows.end(), {hh[0] * vv[0], hh[1] * vv[1], d1[0] * d2[0], d1[1] * d2[1]});
        rhs.insert(rhs.end(), {-hh[2] * vv[2], -d1[2] * d2[2]});
    }
    if (!solve_normal(2, rows, rhs, f)) return false;
    p[0] = sqrt(fabs(1 / f[0]));
    p[1] = sqrt(fabs(1 / f[1]));
    p[2] = cx;
    p[3] = cy;
    for (int v = 0; v < nv; ++v) {   // the pose of each view from its homography
        const double* H = &Hs[(size_t)v * 9];
        double M[9];
        for (int j = 0; j < 3; ++j) { M[j] = H[j] / p[0] - cx / p[0] * H[6 + j]; M[3 + j] = H[3 + j] / p[1] - cy / p[1] * H[6 + j]; M[6 + j] = H[6 + j]; }
        double lam = 1 / sqrt(M[0] * M[0] + M[3] * M[3] + M[6] * M[6]);
        if (M[8] * lam < 0) lam = -lam;
        double r1[3] = {M[0] * lam, M[3] * lam, M[6] * lam}, r2[3] = {M[1] * lam, M[4] * lam, M[7] * lam};
        const double d = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2];
        for (int j = 0; j < 3; ++j) r2[j] -= d * r1[j];
        const double n2 = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
        for (double& t : r2) t /= n2;
        const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
        const double R[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
        rodrigues_inv(R, &p[9 + 6 * v]);
        for (int j = 0; j < 3; ++j) p[12 + 6 * v + j] = M[j * 3 + 2] * lam;
    }
    auto residuals = [&](const std::vector<double>& q, std::vector<double>& r) {
        r.resize((size_t)2 * total);
        for (int v = 0; v < nv; ++v) {
            double R[9];
            rodrigues(&q[9 + 6 * v], R);
            for (int i = off[v]; i < off[v + 1]; ++i) {
                const P2 u = project(obj[i], R, &q[12 + 6 * v], &q[0], &q[4]);
                r[2 * i] = u.x - img[i].x;
                r[2 * i + 1] = u.y - img[i].y;
            }
        }
    };
    auto sumsq = [](const std::vector<double>& r) {
        double s = 0;
        for (double v : r) s += v * v;
        return s;
    };
    std::vector<double> J((size_t)2 * total * np), r, ra, rb, q;
    auto jacobian = [&]() {   // central differences, step kLmStep * max(1, |p_j|)
        for (int j = 0; j < np; ++j) {
            const double h = kLmStep * std::max(1.0, fabs(p[j]));
            q = p; q[j] += h; residuals(q, ra);
            q = p; q[j] -= h; residuals(q, rb);
            for (int i = 0; i < 2 * total; ++i) J[(size_t)i * np + j] = (ra[i] - rb[i]) / (2 * h);
        }
    };
    residuals(p, r);
    double err = sumsq(r), lam = 1e-3;
    jacobian();
    std::vector<double> JtJ((size_t)np * np), g((size_t)np), A, step;
    for (int it = 0; it < kLmIters; ++it) {
        std::fill(JtJ.begin(), JtJ.end(), 0.0);
        std::fill(g.begin(), g.end(), 0.0);
        for (int i = 0; i < 2 * total; ++i) {
            const double* row = &J[(size_t)i * np];
            for (int a = 0; a < np; ++a) {
                if (row[a] == 0.0) continue;
                for (int b = 0; b < np; ++b) JtJ[(size_t)a * np + b] += row[a] * row[b];
                g[a] += row[a] * r[i];
            }
        }
        A = JtJ;
        step.resize((size_t)np);
        for (int a = 0; a < np; ++a) { A[(size_t)a * np + a] += lam * JtJ[(size_t)a * np + a]; step[a] = -g[a]; }
        if (!solve_linear(np, A, step)) { lam *= 10; continue; }
        q = p;
        for (int a = 0; a < np; ++a) q[a] += step[a];
        residuals(q, ra);
        const double e2 = sumsq(ra);
        if (std::isfinite(e2) && e2 < err) {
            double ns = 0, npn = 0;
            for (int a = 0; a < np; ++a) { ns += step[a] * step[a]; npn += p[a] * p[a]; }
            const bool small = sqrt(ns) < DBL_EPSILON * sqrt(npn);
            p = q; r = ra; err = e2; lam = std::max(lam / 10, 1e-16);
            if (small) break;
            jacobian();
        } else {
            lam *= 10;
        }
    }
    const double K[9] = {p[0], 0, p[2], 0, p[1], p[3], 0, 0, 1};
    for (int i = 0; i < 9; ++i) out.K[i] = K[i];
    for (int i = 0; i < 5; ++i) out.dist[i] = p[4 + i];
    out.rvecs.resize((size_t)3 * nv);
    out.tvecs.resize((size_t)3 * nv);
    for (int v = 0; v < nv; ++v)
        for (int j = 0; j < 3; ++j) { out.rvecs[3 * v + j] = p[9 + 6 * v + j]; out.tvecs[3 * v + j] = p[12 + 6 * v + j]; }
    out.rms = sqrt(err / total);
    return std::isfinite(out.rms);
}
}  // namespace calib
