// sfm_pair_pose_core.h -- the two-view and registration records of a frame pair, derived from two views of one view array (DESIGN.md
// §4.10d): the relative pose R_ab, the unit baseline t and its length S, as the dense stage (gms_dense_pairs_device) and the fusion
// (gms_dense_fuse_device) read them from gms_two_view.R/t/status and gms_sfm_pair_reg.S/status. The library's own definition. What the
// kernel (sfm_pair_pose_kernels.hip), the C ABI (capi_sfm.cpp) and the host test build (tests/cpp/sfm_pair_pose_host.cpp) share;
// tests/sfm_pair_pose_ref.py states the same in numpy. fp64, only + - * / sqrt, every sum in index order 0, 1, 2, built with
// -ffp-contract=off: the GPU, the host and numpy agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gms.h"

#if defined(__HIPCC__)
#define PPOSE_HD __host__ __device__ inline
#else
#define PPOSE_HD inline
#endif

namespace ppose {

constexpr int kBlock = 256;         // lanes per workgroup, one pair each
constexpr int kMaxPairs = 1 << 30;  // per call: the grid and a lane's pair index stay far inside 32 bits

static_assert(sizeof(gms_two_view) == 232 && sizeof(gms_sfm_pair_reg) == 40 && sizeof(gms_sfm_view) == 104,
              "the records have no padding: writing every field writes every byte");

PPOSE_HD bool call_args_ok(long long n_frames, long long n_pairs) { return n_pairs >= 0 && n_pairs <= kMaxPairs && n_frames >= 1; }

// finite without a library call: inf - inf and nan - nan are nan
PPOSE_HD bool finite(double v) { return v - v == 0.0; }

PPOSE_HD void zero_records(gms_two_view& tv, gms_sfm_pair_reg& rg, int status)
{
    for (int i = 0; i < 9; ++i) tv.E[i] = tv.R[i] = 0.0;
    for (int i = 0; i < 3; ++i) tv.t[i] = 0.0;
    tv.sum_sq_err1 = tv.sum_sq_err2 = 0.0;
    tv.n_finite = tv.n_behind = 0;
    tv.n_points = tv.n_ransac = tv.ransac_iters = tv.n_pose = tv.pose_which = tv.n_triangulated = 0;
    tv.status = status;
    tv.reserved = 0;
    rg.r = rg.S = 0.0;
    rg.n_links = rg.depth = 0;
    rg.link = -1;
    rg.role = 0;
    rg.status = status;
    rg.reserved = 0;
}

// the pose of camera b against camera a, both views as x_cam = R x_world + t: x_b = R_ab x_a + T. false: not finite, or coincident centres
PPOSE_HD bool relative_pose(const double* Ra, const double* ta, const double* Rb, const double* tb, double* Rab, double* t, double& S)
{
    double T[3];
    bool ok = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Rab[3 * r + c] = Rb[3 * r] * Ra[3 * c] + Rb[3 * r + 1] * Ra[3 * c + 1] + Rb[3 * r + 2] * Ra[3 * c + 2];
            ok = ok && finite(Rab[3 * r + c]);
        }
    for (int r = 0; r < 3; ++r) {
        T[r] = tb[r] - (Rab[3 * r] * ta[0] + Rab[3 * r + 1] * ta[1] + Rab[3 * r + 2] * ta[2]);
        ok = ok && finite(T[r]);
    }
    S = sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]);
    if (!ok || !finite(S) || !(S > 0.0)) return false;
    for (int r = 0; r < 3; ++r) t[r] = T[r] / S;
    return true;
}

// both records of the pair (a, b); the indices are checked before a view's address is formed
PPOSE_HD void pair_records(const gms_sfm_view* views, int n_frames, int a, int b, gms_two_view& tv, gms_sfm_pair_reg& rg)
{
    zero_records(tv, rg, GMS_ERR_NO_MODEL);
    if (a < 0 || a >= n_frames || b < 0 || b >= n_frames || a == b) return;
    const gms_sfm_view &A = views[a], &B = views[b];
    if (A.registered == 0 || B.registered == 0) return;
    double Ra[9], Rb[9], ta[3], tb[3], Rab[9], t[3], S;
    for (int i = 0; i < 9; ++i) Ra[i] = A.R[i], Rb[i] = B.R[i];
    for (int i = 0; i < 3; ++i) ta[i] = A.t[i], tb[i] = B.t[i];
    if (!relative_pose(Ra, ta, Rb, tb, Rab, t, S)) return;
    for (int i = 0; i < 9; ++i) tv.R[i] = Rab[i];
    for (int i = 0; i < 3; ++i) tv.t[i] = t[i];
    rg.S = S;
    tv.status = rg.status = GMS_OK;
}

// ---- the definition on host pointers: the host tests and gms_sfm_pair_poses ---------------------------------------------------------
inline void pair_poses_host(const gms_sfm_view* views, int n_frames, const gms_pair* pairs, int n_pairs, gms_two_view* tv, gms_sfm_pair_reg* rg)
{
    for (int i = 0; i < n_pairs; ++i) pair_records(views, n_frames, pairs[i].frame_a, pairs[i].frame_b, tv[i], rg[i]);
}

}  // namespace ppose
