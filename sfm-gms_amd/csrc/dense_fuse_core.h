// dense_fuse_core.h -- the clouds of several posed pairs fused into one by depth consistency: whether a source (one
// pair's disparity map, valid plane, plan, view and scale) sees a point where its own map says it is, and the rule that keeps a point
// once. The library's own definition. What the kernels (dense_fuse_kernels.hip), the C ABI (capi_dense.cpp) and the host test build
// (tests/cpp/dense_fuse_host.cpp) share; tests/dense_fuse_ref.py states the same in numpy. fp64, only + - * / rint, every sum in the
// order written here, built with -ffp-contract=off: the GPU, the host and numpy agree bit for bit.
#pragma once
#include <stdint.h>

#include "gms.h"
#include "rectify_core.h"

namespace fuse {

constexpr int kMaxNeighbors = 32;
constexpr int kBlockPoints = 1024;  // points per workgroup: 256 lanes x 4 adjacent points
constexpr long long kMaxCap = (long long)rect::kMaxSide * rect::kMaxSide;

enum Look { UNSEEN = 0, CONSISTENT = 1, CONFLICT = 2 };

// the decision bytes of a point: support in the low bits (at most 1 + kMaxNeighbors), kKept when the point is kept
constexpr int kKept = 0x80, kSupportMask = 0x7f;

// what look() needs of a source, by value (the kernel keeps its block's neighbours like this in LDS)
struct View {
    double R1[9], fx, fy, cx, cy, B;
    double GR[9], Gt[3], S;
    const int16_t* disp;
    const uint8_t* valid;
    int32_t width, height, filtered16, min_disp16;
    int32_t lower;  // 1: the source's index is below the looking source's
    int32_t pad;
};
static_assert(sizeof(View) <= 400, "a neighbour record stays under 400 bytes");

RECT_HD bool call_args_ok(long long n_src, long long max_cap, int n_nb, int channels, int tol16, int min_support, long long fused_cap)
{
    return n_src >= 1 && n_src <= 65535 && max_cap >= 1 && max_cap <= kMaxCap && n_src * max_cap <= 2147483647LL && n_nb >= 1 &&
           n_nb <= kMaxNeighbors && (channels == 1 || channels == 3) && tol16 >= 0 && min_support >= 1 && fused_cap >= 0;
}

RECT_HD bool shape_ok(const gms_dense_fuse_src& s, long long max_cap)
{
    return s.width >= 1 && s.width <= rect::kMaxSide && s.height >= 1 && s.height <= rect::kMaxSide && s.cap >= 0 && s.cap <= max_cap;
}

// a source that is not live has no points and sees nothing
RECT_HD bool is_live(const gms_dense_fuse_src& s, long long max_cap)
{
    if (!shape_ok(s, max_cap) || !s.d_plan || !s.d_disp16 || !s.d_valid || !s.d_count) return false;
    if (s.d_plan->status != GMS_OK) return false;
    if (s.d_reg && !(s.d_reg->status == GMS_OK && s.d_reg->S > 0.0)) return false;
    if (s.d_view && s.d_view->registered == 0) return false;
    return true;
}

RECT_HD int n_points(const gms_dense_fuse_src& s, bool live)
{
    if (!live || !s.d_xyz) return 0;
    const int c = *s.d_count;
    return c < 0 ? 0 : c < s.cap ? c : s.cap;
}

// a NULL view is the identity and a NULL registration the scale 1: the arithmetic of look() is the same either way
RECT_HD void make_view(const gms_dense_fuse_src& s, int lower, View& o)
{
    const gms_rectify_plan& P = *s.d_plan;
    for (int i = 0; i < 9; ++i) o.R1[i] = P.R1[i];
    o.fx = P.fx, o.fy = P.fy, o.cx = P.cx, o.cy = P.cy, o.B = P.B;
    for (int i = 0; i < 9; ++i) o.GR[i] = s.d_view ? s.d_view->R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) o.Gt[i] = s.d_view ? s.d_view->t[i] : 0.0;
    o.S = s.d_reg ? s.d_reg->S : 1.0;
    o.disp = s.d_disp16;
    o.valid = s.d_valid;
    o.width = s.width, o.height = s.height, o.filtered16 = s.filtered16, o.min_disp16 = s.min_disp16;
    o.lower = lower;
    o.pad = 0;
}

// Does the source see the point (world frame, float32 widened) where its own map says it is? In two halves, so that a kernel can aim
// several looks, have all their loads in flight together, and then give the verdicts. aim(): the pixel the point falls on, bounds-checked
// before an address is formed; a point that is not in front or falls outside the map aims at pixel 0, which every map has, and is UNSEEN
// whatever it reads there.
struct Aim {
    long long at;  // vi * width + ui, or 0
    double rz;
    int inside;
};
RECT_HD Aim aim(const View& s, const double* P)
{
    double p[3], r[3];
    for (int i = 0; i < 3; ++i) p[i] = ((s.GR[3 * i] * P[0] + s.GR[3 * i + 1] * P[1] + s.GR[3 * i + 2] * P[2]) + s.Gt[i]) / s.S;
    rect::mul3v(s.R1, p, r);
    const double u = s.fx * (r[0] / r[2]) + s.cx, v = s.fy * (r[1] / r[2]) + s.cy;
    const int ui = warp::round_i32(u), vi = warp::round_i32(v);
    Aim a;
    a.rz = r[2];
    a.inside = r[2] > 0.0 && ui >= 0 && ui < s.width && vi >= 0 && vi < s.height;
    a.at = a.inside ? (long long)vi * s.width + ui : 0;
    return a;
}
RECT_HD int verdict(const View& s, const Aim& a, int valid, int d16, int tol16)
{
    if (!a.inside || valid == 0 || d16 == s.filtered16 || d16 < s.min_disp16) return UNSEEN;
    const double e = s.fx * s.B * 16.0 / a.rz;
    return rect::absd((double)d16 - e) <= (double)tol16 ? CONSISTENT : CONFLICT;
}
RECT_HD int look(const View& s, const double* P, int tol16)
{
    const Aim a = aim(s, P);
    return verdict(s, a, s.valid[a.at], s.disp[a.at], tol16);
}

// one look's share of the rule per point, and the point's support byte
RECT_HD void tally(int l, int lower, int& support, int& conflict, int& dup)
{
    support += l == CONSISTENT;
    conflict += l == CONFLICT;
    dup |= (l == CONSISTENT) & lower;
}
RECT_HD int support_byte(int support, int dup, int min_support) { return support | (!dup && support >= min_support ? kKept : 0); }

// the rule per point over the live neighbours in slot order -> its decision bytes
RECT_HD void decide(const View* nb, int n_live, const double* P, int tol16, int min_support, int& sb, int& conflict)
{
    int support = 1, dup = 0;
    conflict = 0;
    for (int j = 0; j < n_live; ++j) tally(look(nb[j], P, tol16), nb[j].lower, support, conflict, dup);
    sb = support_byte(support, dup, min_support);
}

// the live neighbours of source i, in slot order
inline int live_neighbors(const gms_dense_fuse_src* src, int n_src, long long max_cap, const int32_t* nb_row, int n_nb, int i, View* out)
{
    int n = 0;
    for (int q = 0; q < n_nb; ++q) {
        const int j = nb_row[q];
        if (j < 0 || j >= n_src || j == i || !is_live(src[j], max_cap)) continue;
        make_view(src[j], j < i, out[n++]);
    }
    return n;
}

// ---- the definition on host pointers, for the host tests; the kernels restate the loops per block ----------------------------------------
// max_cap: the largest cap a source may have. Outputs as gms_dense_fuse_device's; nothing past min(total, fused_cap) is written.
inline void fuse_host(const gms_dense_fuse_src* src, int n_src, long long max_cap, const int32_t* neighbors, int n_nb, int channels, int tol16,
                      int min_support, long long fused_cap, float* xyz, uint8_t* color, int32_t* source, int32_t* index, uint8_t* support,
                      uint8_t* conflict, int32_t* counts)
{
    long long total = 0;
    for (int i = 0; i < n_src; ++i) {
        View nb[kMaxNeighbors];
        const bool live = is_live(src[i], max_cap);
        const int n = n_points(src[i], live);
        const int n_live = n ? live_neighbors(src, n_src, max_cap, neighbors + (long long)i * n_nb, n_nb, i, nb) : 0;
        int kept = 0;
        for (int k = 0; k < n; ++k) {
            const float* f = src[i].d_xyz + 3LL * k;
            const double P[3] = {(double)f[0], (double)f[1], (double)f[2]};
            int sb, cf;
            decide(nb, n_live, P, tol16, min_support, sb, cf);
            if (!(sb & kKept)) continue;
            if (total < fused_cap) {
                for (int c = 0; c < 3; ++c) xyz[3 * total + c] = f[c];
                if (color)
                    for (int c = 0; c < channels; ++c) color[channels * total + c] = src[i].d_color ? src[i].d_color[(long long)channels * k + c] : 0;
                source[total] = i;
                index[total] = k;
                support[total] = (uint8_t)(sb & kSupportMask);
                conflict[total] = (uint8_t)cf;
            }
            ++total;
            ++kept;
        }
        counts[i] = kept;
    }
    counts[n_src] = (int32_t)total;
}

}  // namespace fuse
