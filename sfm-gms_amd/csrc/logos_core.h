// logos_core.h -- the per-point and per-candidate arithmetic of cv::xfeatures2d::matchLOGOS (LOGOS), restated from the
// reference DLL's machine code and pinned by tests/golden/refdll_logos.npz.
//
// Plain functions of their arguments, so that the SAME source is what logos_kernels.hip runs per lane and what
// tests/cpp/logos_host.cpp compiles with g++ for the CPU tests (a test build). Build with -ffp-contract=off: the DLL rounds every
// float product before the sum. The two elementary functions the DLL takes from the CRT (logf, acosf) are implemented here in
// fp64 from +, -, *, / alone and rounded to float, so that the device and a host build give the same bits; neither ocml nor libm is
// called.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GMS_HD __host__ __device__ __forceinline__
#else
#define GMS_HD inline
#endif

namespace gms {
namespace logos {

// LogosParams of the DLL's Logos::Logos (all 0.1f; NUM1 = NUM2 = 5), and Logos::init: LB = (float)-pi, BINSIZE = 0.1f / 3.0f,
// BINNUMBER = (int)ceil(2 pi / (double)BINSIZE) = 189.
constexpr float kThresh = 0.1f;
constexpr int kNum = 5;
constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 6.283185307179586;
constexpr float kLB = -3.14159274f;
constexpr int kBins = 189;
GMS_HD float bin_size() { return kThresh / 3.0f; }

GMS_HD uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
GMS_HD float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// logf: x = 2^e * m, m in [sqrt(1/2), sqrt(2)); log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| < 0.172; fp64, rounded to float.
GMS_HD float logf_(float xf)
{
    if (xf != xf || xf < 0.0f) return u2f(0x7fc00000u);
    if (xf == 0.0f) return -INFINITY;
    if (xf == INFINITY) return INFINITY;
    uint32_t b = f2u(xf);
    int e = (int)((b >> 23) & 0xffu) - 127;
    double m;
    if (e == -127) {  // subnormal: scale by 2^23 exactly
        b = f2u(xf * 8388608.0f);
        e = (int)((b >> 23) & 0xffu) - 127 - 23;
    }
    m = (double)u2f((b & 0x007fffffu) | 0x3f800000u);
    if (m > 1.4142135623730951) {
        m *= 0.5;
        e += 1;
    }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 23.0;
    for (int k = 21; k >= 1; k -= 2) p = p * z + 1.0 / (double)k;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    return (float)((double)e * ln2_hi + ((double)e * ln2_lo + 2.0 * s * p));
}

// asin(y) for 0 <= y <= 0.5 by its Taylor series (27 terms), fp64
GMS_HD double asin_small(double y)
{
    const double t = y * y;
    double term = y, sum = y, a = 1.0, pw = y;
    for (int n = 0; n < 27; n++) {
        a = a * (double)(2 * n + 1) / (double)(2 * n + 2);
        pw = pw * t;
        term = a * pw / (double)(2 * n + 3);
        sum = sum + term;
    }
    return sum;
}

// sqrt in fp64 from a correctly rounded float seed and two Newton steps (+, *, / only)
GMS_HD double sqrt_nr(double t)
{
    if (t <= 0.0) return 0.0;
    double y = (double)sqrtf((float)t);
    y = 0.5 * (y + t / y);
    y = 0.5 * (y + t / y);
    return y;
}

// acosf: pi/2 - asin x on |x| <= 1/2, 2 asin sqrt((1 - |x|) / 2) beyond; fp64, rounded to float
GMS_HD float acosf_(float xf)
{
    if (xf != xf || xf > 1.0f || xf < -1.0f) return u2f(0x7fc00000u);
    const double x = (double)xf;
    double r;
    if (x <= 0.5 && x >= -0.5) {
        r = kPi * 0.5 - (x < 0.0 ? -asin_small(-x) : asin_small(x));
    } else if (x > 0.0) {
        r = 2.0 * asin_small(sqrt_nr((1.0 - x) * 0.5));
    } else {
        r = kPi - 2.0 * asin_small(sqrt_nr((1.0 + x) * 0.5));
    }
    return (float)r;
}

// Point::Point: orientation = (float)(angle * pi / 180.0) in fp64
GMS_HD float orientation(float angle_deg) { return (float)(((double)angle_deg * kPi) / 180.0); }

// The keypoint domain of every LOGOS entry point (include/gms.h): x, y and angle finite, |angle| <= kMaxAngleDeg. Ten turns is far
// beyond any detector's output (-1, OpenCV's "no orientation", and 360 lie inside), and it is what bounds the loops of rel_ori:
// beyond 2^27 rad a float no longer changes when 2 pi is taken off it, so the DLL's loop -- and this one -- would never end.
// size is not restricted: logf_ is total and a NaN fails every comparison, as in the DLL.
constexpr float kMaxAngleDeg = 3600.0f;
GMS_HD bool kp_ok(float x, float y, float angle)
{
    return x - x == 0.0f && y - y == 0.0f && angle - angle == 0.0f && fabsf(angle) <= kMaxAngleDeg;
}

// PointPair::PointPair: relOri = o1 - o2, brought into [-pi, pi] through fp64 the way the DLL loops. The entry points admit only
// keypoints that pass kp_ok, so |d| <= 2 * 3600 deg = 40 pi (+ rounding) and either loop runs at most 21 times; the inf / NaN test
// only keeps a direct caller (the host build) from looping, it is not reached from the kernels.
GMS_HD float rel_ori(float o1, float o2)
{
    float d = o1 - o2;
    if (!(d - d == 0.0f)) return d;  // inf / NaN: outside the domain; left as they are
    while ((double)d > kPi) d = (float)((double)d - kTwoPi);
    while (-kPi > (double)d) d = (float)((double)d + kTwoPi);
    return d;
}

// min(|2 pi - t|, t), t = |a - b| reduced below 2 pi
GMS_HD float angle_dist(float a, float b)
{
    float t = fabsf(a - b);
    if (!(t - t == 0.0f)) return t;  // inf / NaN (see rel_ori)
    while ((double)t > kTwoPi) t = (float)((double)t - kTwoPi);
    t = fabsf(t);
    const float u = fabsf((float)(kTwoPi - (double)t));
    return u < t ? u : t;
}

struct Pt {
    float x, y, ori, logscale;
};

// One neighbour pair (a in image 1, b in image 2) against the candidate (p, q): all four measures under the thresholds.
// rel_o / rel_s: the candidate's relOri and relScale. NaN (coincident points) fails every comparison, as in the DLL.
GMS_HD bool consistent(const Pt& p, const Pt& q, float rel_o, float rel_s, const Pt& a, const Pt& b)
{
    const float n_rel_o = rel_ori(a.ori, b.ori);
    const float n_rel_s = a.logscale - b.logscale;
    const float intra_o = angle_dist(rel_o, n_rel_o);
    const float intra_s = fabsf(rel_s - n_rel_s);
    const float dx1 = p.x - a.x, dy1 = p.y - a.y;
    const float dx2 = q.x - b.x, dy2 = q.y - b.y;
    const float c1 = dy2 * dx1, c2 = dy1 * dx2;
    const float cross = c1 - c2;
    const float s1a = dy1 * dy1, s1b = dx1 * dx1;
    const float n1 = sqrtf(s1a + s1b);
    const float s2a = dy2 * dy2, s2b = dx2 * dx2;
    const float n2 = sqrtf(s2a + s2b);
    const float d1 = dy2 * dy1, d2 = dx2 * dx1, nn = n2 * n1;
    const float dot = (d1 + d2) / nn;
    float c = -1.0f > dot ? -1.0f : dot;
    if (c > 1.0f) c = 1.0f;
    const float sign = (float)((cross > 0.0f ? 1 : 0) - (0.0f > cross ? 1 : 0));
    const float ang = acosf_(c) * sign;
    const float lsc = logf_(n1) - logf_(n2);
    const float inter_o = angle_dist(rel_o, ang);
    const float inter_s = fabsf(rel_s - lsc);
    return kThresh > intra_o && kThresh > intra_s && kThresh > inter_o && kThresh > inter_s;
}

// The same verdict as consistent(), from the same operations on the same operands, but the cheap intra tests come first and the
// logf / acosf of the inter tests are only evaluated while the verdict is still open (the batched path's support test).
GMS_HD bool consistent_early(const Pt& p, const Pt& q, float rel_o, float rel_s, const Pt& a, const Pt& b)
{
    const float n_rel_o = rel_ori(a.ori, b.ori);
    const float n_rel_s = a.logscale - b.logscale;
    if (!(kThresh > fabsf(rel_s - n_rel_s))) return false;
    if (!(kThresh > angle_dist(rel_o, n_rel_o))) return false;
    const float dx1 = p.x - a.x, dy1 = p.y - a.y;
    const float dx2 = q.x - b.x, dy2 = q.y - b.y;
    const float s1a = dy1 * dy1, s1b = dx1 * dx1;
    const float n1 = sqrtf(s1a + s1b);
    const float s2a = dy2 * dy2, s2b = dx2 * dx2;
    const float n2 = sqrtf(s2a + s2b);
    const float lsc = logf_(n1) - logf_(n2);
    if (!(kThresh > fabsf(rel_s - lsc))) return false;
    const float c1 = dy2 * dx1, c2 = dy1 * dx2;
    const float cross = c1 - c2;
    const float d1 = dy2 * dy1, d2 = dx2 * dx1, nn = n2 * n1;
    const float dot = (d1 + d2) / nn;
    float c = -1.0f > dot ? -1.0f : dot;
    if (c > 1.0f) c = 1.0f;
    const float sign = (float)((cross > 0.0f ? 1 : 0) - (0.0f > cross ? 1 : 0));
    const float ang = acosf_(c) * sign;
    return kThresh > angle_dist(rel_o, ang);
}

// Logos::estimateMatches: histogram bin of a supported candidate's relOri (floor by truncation and correction; out of range ->
// last bin, as the DLL's unsigned compare does)
GMS_HD int bin_of(float rel_o)
{
    const float t = (rel_o - kLB) / bin_size();
    int b = (int)t;
    if ((float)b > t) b -= 1;
    return (b < 0 || b >= kBins) ? kBins - 1 : b;
}

// Logos::calcGlobalOrientation: three-bin circular smoothing, first maximum; returns the peak bin's centre, *peak_bin the bin
GMS_HD float peak_orientation(const int32_t* bins, int* peak_bin)
{
    int best = 0;
    int32_t best_v = bins[kBins - 1] + bins[1] + bins[0];
    for (int b = 1; b < kBins; b++) {
        const int32_t v = b == kBins - 1 ? bins[b - 1] + bins[0] + bins[b] : bins[b + 1] + bins[b - 1] + bins[b];
        if (v > best_v) {
            best_v = v;
            best = b;
        }
    }
    *peak_bin = best;
    const float bs = bin_size();
    const float lo = (float)best * bs + kLB;
    return lo + bs * 0.5f;
}

// the global test: GLOBALORITHRESH > |relOri - peak| in fp64
GMS_HD bool globally_consistent(float rel_o, float peak) { return (double)kThresh > fabs((double)rel_o - (double)peak); }

// squared distance of two points, float, the DLL's order
GMS_HD float dist2(float x0, float y0, float x1, float y1)
{
    const float dx = x0 - x1, dy = y0 - y1;
    const float a = dx * dx, b = dy * dy;
    return a + b;
}

// ---- Point::nearestNeighbours' std::sort (DLL RVA 0x52d60, predicate RVA 0x53540: a.d < b.d on the float alone) ---------------
// MSVC's introsort as the DLL runs it, on records (d[k], ix[k]): ranges of at most 32 by insertion sort, a median of three (of
// nine above 40 elements) and a three-way partition around it, (ideal >> 1) + (ideal >> 2) per level from ideal = n, heap sort
// when that reaches 0. Not stable: among equal distances this order decides which points are the first NUM neighbours. Only the
// ranges reaching into [0, k) are worked on (elements never cross a partition's boundaries), so this costs O(n) on average.
// Matches tests/logos_ref.py msvc_sort_head, which is checked against the DLL's own sort.
constexpr long kIsortMax = 32;

GMS_HD void sort_swap(float* d, int32_t* ix, long a, long b)
{
    const float td = d[a];
    d[a] = d[b];
    d[b] = td;
    const int32_t ti = ix[a];
    ix[a] = ix[b];
    ix[b] = ti;
}

GMS_HD void sort_insertion(float* d, int32_t* ix, long f, long l)
{
    for (long nx = f + 1; nx < l; nx++) {
        const float vd = d[nx];
        const int32_t vi = ix[nx];
        long h = nx;
        if (vd < d[f]) {
            for (; h > f; h--) {
                d[h] = d[h - 1];
                ix[h] = ix[h - 1];
            }
        } else {
            for (; vd < d[h - 1]; h--) {
                d[h] = d[h - 1];
                ix[h] = ix[h - 1];
            }
        }
        d[h] = vd;
        ix[h] = vi;
    }
}

GMS_HD void sort_med3(float* d, int32_t* ix, long f, long m, long l)
{
    if (d[m] < d[f]) sort_swap(d, ix, m, f);
    if (d[l] < d[m]) {
        sort_swap(d, ix, l, m);
        if (d[m] < d[f]) sort_swap(d, ix, m, f);
    }
}

// _Partition_by_median_guess_unchecked: [f, l) -> [f, *pf) < pivot, [*pf, *pl) equal, [*pl, l) greater
GMS_HD void sort_partition(float* d, int32_t* ix, long f, long l, long* out_pf, long* out_pl)
{
    const long m = f + ((l - f) >> 1), last = l - 1, cnt = last - f;
    if (40 < cnt) {
        const long st = (cnt + 1) >> 3, tw = st << 1;
        sort_med3(d, ix, f, f + st, f + tw);
        sort_med3(d, ix, m - st, m, m + st);
        sort_med3(d, ix, last - tw, last - st, last);
        sort_med3(d, ix, f + st, m, last - st);
    } else {
        sort_med3(d, ix, f, m, last);
    }
    long pf = m, pl = m + 1;
    while (f < pf && !(d[pf - 1] < d[pf]) && !(d[pf] < d[pf - 1])) pf--;
    while (pl < l && !(d[pl] < d[pf]) && !(d[pf] < d[pl])) pl++;
    long gf = pl, gl = pf;
    for (;;) {
        for (; gf < l; gf++) {
            if (d[pf] < d[gf]) continue;
            if (d[gf] < d[pf]) break;
            if (pl != gf) sort_swap(d, ix, pl, gf);
            pl++;
        }
        for (; f < gl; gl--) {
            if (d[gl - 1] < d[pf]) continue;
            if (d[pf] < d[gl - 1]) break;
            if (--pf != gl - 1) sort_swap(d, ix, pf, gl - 1);
        }
        if (gl == f && gf == l) break;
        if (gl == f) {
            if (pl != gf) sort_swap(d, ix, pf, pl);
            pl++;
            sort_swap(d, ix, pf, gf);
            pf++;
            gf++;
        } else if (gf == l) {
            if (--gl != --pf) sort_swap(d, ix, gl, pf);
            sort_swap(d, ix, pf, --pl);
        } else {
            sort_swap(d, ix, gf, --gl);
            gf++;
        }
    }
    *out_pf = pf;
    *out_pl = pl;
}

// _Pop_heap_hole_by_index + _Push_heap_by_index on the heap [f, f + bottom) (a max-heap under a.d < b.d)
GMS_HD void sort_sift(float* d, int32_t* ix, long f, long hole, long bottom, float vd, int32_t vi)
{
    const long top = hole, max_non_leaf = (bottom - 1) >> 1;
    long idx = hole;
    while (idx < max_non_leaf) {
        idx = 2 * idx + 2;
        if (d[f + idx] < d[f + idx - 1]) idx--;
        d[f + hole] = d[f + idx];
        ix[f + hole] = ix[f + idx];
        hole = idx;
    }
    if (idx == max_non_leaf && bottom % 2 == 0) {
        d[f + hole] = d[f + bottom - 1];
        ix[f + hole] = ix[f + bottom - 1];
        hole = bottom - 1;
    }
    for (idx = (hole - 1) >> 1; top < hole && d[f + idx] < vd; idx = (hole - 1) >> 1) {
        d[f + hole] = d[f + idx];
        ix[f + hole] = ix[f + idx];
        hole = idx;
    }
    d[f + hole] = vd;
    ix[f + hole] = vi;
}

GMS_HD void sort_heap(float* d, int32_t* ix, long f, long l)
{
    const long n = l - f;
    for (long hole = (n >> 1) - 1; hole >= 0; hole--) sort_sift(d, ix, f, hole, n, d[f + hole], ix[f + hole]);
    for (long last = n - 1; last > 0; last--) {
        const float vd = d[f + last];
        const int32_t vi = ix[f + last];
        d[f + last] = d[f];
        ix[f + last] = ix[f];
        sort_sift(d, ix, f, 0, last, vd, vi);
    }
}

// the first k places (k <= 32) of MSVC std::sort over n records
GMS_HD void msvc_sort_head(float* d, int32_t* ix, long n, long k)
{
    long f = 0, l = n, ideal = n;
    for (;;) {
        if (f >= k) return;
        if (l - f <= kIsortMax) {
            sort_insertion(d, ix, f, l);
            return;
        }
        if (ideal <= 0) {
            sort_heap(d, ix, f, l);
            return;
        }
        long pf, pl;
        sort_partition(d, ix, f, l, &pf, &pl);
        ideal = (ideal >> 1) + (ideal >> 2);
        if (pl < k) {  // both outer parts reach below k: the lower one lies inside [0, k), at most 32 records
            sort_insertion(d, ix, f, pf);
            f = pl;
        } else {
            l = pf;
        }
    }
}

}  // namespace logos
}  // namespace gms
