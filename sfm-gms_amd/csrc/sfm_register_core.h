// sfm_register_core.h -- registering many two-view results into one frame: the plan over the pair list, when a
// link between two pairs' points counts and its scale ratio, and the pose and point transforms. What the C ABI (capi_sfm.cpp), the
// kernels (sfm_register_kernels.hip) and the host build (tests/cpp/sfm_register_host.cpp) share; tests/sfm_register_ref.py states the
// same in numpy. This is the library's own definition: the reference stops at one pair (SfMUtil.cpp:4-83).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gms.h"

#if defined(__HIPCC__)
#define SFR_HD __host__ __device__ inline
#else
#define SFR_HD inline
#endif

namespace sfr {

constexpr int32_t kNoSlot = INT32_MAX;

// The plan, from the pair list alone. reg_by: n_frames of scratch (-2: not registered, -1: the root, else the pair that registered
// the frame). Walks the pairs in order: pair i registers frame_b when frame_a is registered and frame_b is not. Its link is the pair
// that registered frame_a (role 1: the shared frame is that pair's frame_b) or, for frame_a = root, the first registering pair out of
// the root (role 0; that pair itself has none). Every other pair is skipped. Returns false on a frame index out of range.
inline bool plan(const gms_pair* pairs, int n_pairs, int n_frames, int root, int32_t* reg_by, gms_sfm_plan_entry* out)
{
    if (root < 0 || root >= n_frames) return false;
    for (int i = 0; i < n_pairs; i++)
        if (pairs[i].frame_a < 0 || pairs[i].frame_a >= n_frames || pairs[i].frame_b < 0 || pairs[i].frame_b >= n_frames) return false;
    for (int f = 0; f < n_frames; f++) reg_by[f] = -2;
    reg_by[root] = -1;
    int first_root = -1;
    for (int i = 0; i < n_pairs; i++) {
        const int a = pairs[i].frame_a, b = pairs[i].frame_b;
        out[i] = gms_sfm_plan_entry{0, -1, 0, 0};
        if (reg_by[a] == -2 || reg_by[b] != -2) continue;
        out[i].registers = 1;
        if (a == root) {
            if (first_root < 0) first_root = i;
            else out[i].link = first_root;
        } else {
            out[i].link = reg_by[a];
            out[i].role = 1;
        }
        if (out[i].link >= 0) out[i].depth = out[out[i].link].depth + 1;
        reg_by[b] = i;
    }
    return true;
}

// Whether a pair's record fits the arrays it indexes: both frame indices in [0, n_frames), m >= 0, a match range inside
// [0, total_m] and both frames' keypoint ranges inside [0, total_kp]. No sum is formed that need not fit 64 bits: match_off is held
// against total_m - m (total_m >= 0 and m >= 0 by then), a frame's end against total_kp. frame_off is read only behind the frame
// indices' check. A pair that does not fit has no matches and does not register. *r: the two frames' ranges, set when it fits.
struct PairRanges {
    int64_t oa, ob, na, nb;
};
SFR_HD bool pair_fits(const gms_pair& pr, const int64_t* frame_off, int n_frames, int64_t total_kp, int64_t total_m, PairRanges* r)
{
    if (pr.frame_a < 0 || pr.frame_a >= n_frames || pr.frame_b < 0 || pr.frame_b >= n_frames || pr.m < 0 || pr.match_off < 0 || total_m < 0 ||
        pr.match_off > total_m - (int64_t)pr.m)
        return false;
    const int64_t oa = frame_off[pr.frame_a], ea = frame_off[pr.frame_a + 1], ob = frame_off[pr.frame_b], eb = frame_off[pr.frame_b + 1];
    if (oa < 0 || ob < 0 || ea < oa || eb < ob || ea > total_kp || eb > total_kp) return false;
    *r = PairRanges{oa, ob, ea - oa, eb - ob};
    return true;
}
// A plan entry of pair i that the walk in pair order can follow: one that registers links to an earlier pair, or to none (-1).
SFR_HD bool plan_entry_fits(const gms_sfm_plan_entry& pl, int i) { return !pl.registers || (pl.link >= -1 && pl.link < i); }

// the matches of a pair that the stage reads: those the two-view stage gathered
SFR_HD int pair_count(const gms_pair& pr, const gms_two_view& t)
{
    if (t.status != GMS_OK) return 0;
    const int n = t.n_points < pr.m ? t.n_points : pr.m;
    return n > 0 ? n : 0;
}
// a pair whose own two-view result can be registered (the plan and the link decide the rest)
SFR_HD bool base_ok(const gms_sfm_plan_entry& pl, const gms_two_view& t) { return pl.registers && t.status == GMS_OK && t.n_triangulated > 0; }

// X of a link: the linked pair's point, for role 1 taken into its second camera: R p + t
SFR_HD void link_point(int role, const double* R, const double* t, const double* p, double* X)
{
    if (role == 0) {
        X[0] = p[0]; X[1] = p[1]; X[2] = p[2];
        return;
    }
    for (int r = 0; r < 3; r++) X[r] = R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2] + t[r];
}
SFR_HD bool link_valid(const double* X, const double* Y)
{
    return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(Y[0]) && isfinite(Y[1]) && isfinite(Y[2]) && X[2] > 0.0 && Y[2] > 0.0;
}
SFR_HD double link_ratio(const double* X, const double* Y)
{
    return sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) / sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
}

// G_b = [R_i G_a.R | R_i G_a.t + S t_i]
SFR_HD void compose_view(const double* Ri, const double* ti, double S, const double* Ra, const double* ta, double* Rb, double* tb)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Rb[3 * r + c] = Ri[3 * r] * Ra[c] + Ri[3 * r + 1] * Ra[3 + c] + Ri[3 * r + 2] * Ra[6 + c];
        tb[r] = Ri[3 * r] * ta[0] + Ri[3 * r + 1] * ta[1] + Ri[3 * r + 2] * ta[2] + S * ti[r];
    }
}
// W = G_a.R^T (S p - G_a.t)
SFR_HD void world_point(const double* Ra, const double* ta, double S, const double* p, double* W)
{
    const double d0 = S * p[0] - ta[0], d1 = S * p[1] - ta[1], d2 = S * p[2] - ta[2];
    for (int c = 0; c < 3; c++) W[c] = d0 * Ra[c] + d1 * Ra[3 + c] + d2 * Ra[6 + c];
}

}  // namespace sfr
