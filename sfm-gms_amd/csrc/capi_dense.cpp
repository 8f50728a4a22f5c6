// capi_dense.cpp -- the C ABI of the dense stage: the points of disparity maps, the dense clouds of posed pairs (rectify, SGM, speckle
// filter, reproject) and their fusion into one cloud.
#include <vector>

#include "capi_common.h"
#include "dense_fuse_core.h"
#include "gms_kernels.h"
#include "stereo_sgm_core.h"
#include "warp_core.h"

extern "C" {

size_t gms_dense_cloud_workspace_bytes(int width, int height, int n_pairs)
{
    if (n_pairs < 1 || n_pairs > 65535 || !warp::side_ok(width) || !warp::side_ok(height)) return 0;
    return gms::dense_cloud_ws_bytes(n_pairs, width, height);
}

int gms_dense_cloud_device(gms_ctx* c, const int16_t* d_disp16, const uint8_t* d_valid, const uint8_t* d_image, int channels,
                           int image_pitch, int n_pairs, int width, int height, const gms_rectify_plan* d_plans, int filtered16,
                           int min_disp16, const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames,
                           void* d_ws, size_t ws_bytes, int cap, float* d_xyz, uint8_t* d_color, int32_t* d_pixel, int32_t* d_count)
{
    if (!c || n_pairs < 0 || n_pairs > 65535 || !warp::side_ok(width) || !warp::side_ok(height) || min_disp16 < 1 || cap < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_disp16 || !d_valid || !d_plans || !d_ws || !d_count || (cap > 0 && (!d_xyz || !d_pixel)) || !reg_group_ok(d_pairs, d_reg, d_views, n_frames))
        return GMS_ERR_BAD_ARG;
    if (d_image && ((channels != 1 && channels != 3) || (long long)image_pitch < (long long)channels * width)) return GMS_ERR_BAD_ARG;
    if (d_color && !d_image) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::dense_cloud_ws_bytes(n_pairs, width, height)) || misaligned(d_plans, 8) || misaligned(d_disp16, 2) ||
        misaligned(d_xyz, 4) || misaligned(d_pixel, 4) || misaligned(d_count, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_dense_cloud(d_disp16, d_valid, d_image, channels, image_pitch, n_pairs, width, height, d_plans, filtered16, min_disp16,
                                       d_pairs, d_reg, d_views, n_frames, d_ws, cap, d_xyz, d_color, d_pixel, d_count, c->stream);
    });
}

GMS_PARAMS_OR(dense_sgm_params, gms_stereo_sgm_params, GMS_STEREO_SGM_PARAMS_DENSE)

static bool dense_shape_ok(int sw, int sh, int channels, int ow, int oh, int n_pairs, const gms_stereo_sgm_params& p)
{
    return n_pairs >= 1 && n_pairs <= 65535 && (channels == 1 || channels == 3) && warp::side_ok(sw) && warp::side_ok(sh) && warp::side_ok(ow) &&
           warp::side_ok(oh) && sgm::params_ok(p, ow, oh);
}

size_t gms_dense_pairs_workspace_bytes(int sw, int sh, int channels, int ow, int oh, int n_pairs, const gms_stereo_sgm_params* params)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!dense_shape_ok(sw, sh, channels, ow, oh, n_pairs, p)) return 0;
    const size_t sgm_bytes = gms::stereo_sgm_ws_bytes(p, n_pairs, ow, oh);
    return sgm_bytes ? gms::dense_pairs_layout(n_pairs, sw, sh, channels, ow, oh, sgm_bytes).total : 0;
}

// everything behind the plans, in stream order: grey, the three rectified images, the matcher, the cloud
static hipError_t dense_pairs_launch(const gms_camera& cam, const gms_stereo_sgm_params& p, const uint8_t* d_img1, const uint8_t* d_img2, int n,
                                     int sw, int sh, int channels, int ow, int oh, int min_disp16, const gms_pair* d_pairs,
                                     const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                                     const gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color,
                                     int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count,
                                     int speckle_size, int speckle_diff16, int32_t* d_removed, hipStream_t st)
{
    // speckle_size > 0: the workspace is DensePairsFilteredLayout's, whose first regions are DensePairsLayout's
    const gms::DensePairsFilteredLayout F = gms::dense_pairs_filtered_layout(n, sw, sh, channels, ow, oh, gms::stereo_sgm_ws_bytes(p, n, ow, oh));
    const gms::DensePairsLayout& L = F.pairs;
    const uint8_t *g1 = d_img1, *g2 = d_img2;
    hipError_t e;
    if (channels == 3) {
        uint8_t* grey = gms::ws_ptr<uint8_t>(d_ws, L.grey);
        const size_t plane = (size_t)n * (size_t)sw * (size_t)sh;
        if ((e = gms::launch_bgr_to_gray(d_img1, n, sw, sh, grey, st)) != hipSuccess) return e;
        if ((e = gms::launch_bgr_to_gray(d_img2, n, sw, sh, grey + plane, st)) != hipSuccess) return e;
        g1 = grey;
        g2 = grey + plane;
        if ((e = gms::launch_rectify(cam, d_img1, n, sw, sh, 3, 3 * sw, d_plans, n, 1, d_color, ow, oh, 3 * ow, nullptr, st)) != hipSuccess) return e;
    }
    if ((e = gms::launch_rectify(cam, g1, n, sw, sh, 1, sw, d_plans, n, 1, d_rect1, ow, oh, ow, d_valid, st)) != hipSuccess) return e;
    if ((e = gms::launch_rectify(cam, g2, n, sw, sh, 1, sw, d_plans, n, 2, d_rect2, ow, oh, ow, nullptr, st)) != hipSuccess) return e;
    if ((e = gms::launch_stereo_sgm(p, d_rect1, d_rect2, n, ow, oh, ow, gms::ws_ptr<void>(d_ws, L.sgm), d_disp16, nullptr, st)) != hipSuccess) return e;
    if (speckle_size > 0)
        e = gms::launch_filter_speckles(d_disp16, n, ow, oh, (p.bm.min_disparity - 1) * 16, speckle_size, speckle_diff16,
                                        gms::ws_ptr<void>(d_ws, F.speckle), d_removed, st);
    else if (d_removed)
        e = hipMemsetAsync(d_removed, 0, sizeof(int32_t) * (size_t)n, st);
    if (e != hipSuccess) return e;
    return gms::launch_dense_cloud(d_disp16, d_valid, channels == 3 ? d_color : d_rect1, channels, channels * ow, n, ow, oh, d_plans,
                                   (p.bm.min_disparity - 1) * 16, min_disp16, d_pairs, d_reg, d_views, n_frames, gms::ws_ptr<void>(d_ws, L.cloud), cap,
                                   d_xyz, d_cloud_color, d_pixel, d_count, st);
}

size_t gms_dense_pairs_filtered_workspace_bytes(int sw, int sh, int channels, int ow, int oh, int n_pairs, const gms_stereo_sgm_params* params)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!dense_shape_ok(sw, sh, channels, ow, oh, n_pairs, p)) return 0;
    const size_t sgm_bytes = gms::stereo_sgm_ws_bytes(p, n_pairs, ow, oh);
    return sgm_bytes ? gms::dense_pairs_filtered_layout(n_pairs, sw, sh, channels, ow, oh, sgm_bytes).total : 0;
}

// filtered: the workspace also holds the filter's region (also with speckle_size 0, so that one size serves every call)
static int dense_pairs_device(gms_ctx* c, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1, const uint8_t* d_img2,
                              int n_pairs, int sw, int sh, int channels, const gms_two_view* d_tv, int ow, int oh, int min_disp16,
                              const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                              size_t ws_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color,
                              int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count, bool filtered,
                              int speckle_size, int speckle_diff16, int32_t* d_removed)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!c || !camera || !dense_shape_ok(sw, sh, channels, ow, oh, n_pairs, p) || min_disp16 < 1 || cap < 0) return GMS_ERR_BAD_ARG;
    if (speckle_size < 0 || speckle_diff16 < 0 || misaligned(d_removed, 4)) return GMS_ERR_BAD_ARG;
    if (!d_img1 || !d_img2 || !d_tv || !d_ws || !d_plans || !d_rect1 || !d_rect2 || !d_valid || (channels == 3 && !d_color) || !d_disp16 ||
        !d_count || (cap > 0 && (!d_xyz || !d_pixel)) || !reg_group_ok(d_pairs, d_reg, d_views, n_frames))
        return GMS_ERR_BAD_ARG;
    const size_t need = filtered ? gms_dense_pairs_filtered_workspace_bytes(sw, sh, channels, ow, oh, n_pairs, &p)
                                 : gms_dense_pairs_workspace_bytes(sw, sh, channels, ow, oh, n_pairs, &p);
    if (!ws_ok(d_ws, ws_bytes, need) || misaligned(d_plans, 8) || misaligned(d_disp16, 2) || misaligned(d_xyz, 4) || misaligned(d_pixel, 4) ||
        misaligned(d_count, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        const hipError_t e = gms::launch_rectify_plan(*camera, d_tv, n_pairs, sw, sh, ow, oh, d_plans, c->stream);
        if (e != hipSuccess) return e;
        return dense_pairs_launch(*camera, p, d_img1, d_img2, n_pairs, sw, sh, channels, ow, oh, min_disp16, d_pairs, d_reg, d_views, n_frames, d_ws,
                                  d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color, d_pixel, d_count, speckle_size,
                                  speckle_diff16, d_removed, c->stream);
    });
}

int gms_dense_pairs_device(gms_ctx* c, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1, const uint8_t* d_img2,
                           int n_pairs, int sw, int sh, int channels, const gms_two_view* d_tv, int ow, int oh, int min_disp16,
                           const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                           size_t ws_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color,
                           int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count)
{
    return dense_pairs_device(c, camera, params, d_img1, d_img2, n_pairs, sw, sh, channels, d_tv, ow, oh, min_disp16, d_pairs, d_reg, d_views, n_frames,
                              d_ws, ws_bytes, d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color, d_pixel, d_count, false,
                              0, 0, nullptr);
}

int gms_dense_pairs_filtered_device(gms_ctx* c, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1,
                                    const uint8_t* d_img2, int n_pairs, int sw, int sh, int channels, const gms_two_view* d_tv, int ow, int oh,
                                    int min_disp16, const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames,
                                    void* d_ws, size_t ws_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid,
                                    uint8_t* d_color, int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel,
                                    int32_t* d_count, int speckle_size, int speckle_diff16, int32_t* d_removed)
{
    return dense_pairs_device(c, camera, params, d_img1, d_img2, n_pairs, sw, sh, channels, d_tv, ow, oh, min_disp16, d_pairs, d_reg, d_views, n_frames,
                              d_ws, ws_bytes, d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color, d_pixel, d_count, true,
                              speckle_size, speckle_diff16, d_removed);
}

int gms_dense_pair_filtered(const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* img1, const uint8_t* img2, int width,
                            int height, int channels, const double* R, const double* t, int out_w, int out_h, int min_disp16, gms_rectify_plan* plan,
                            uint8_t* rect1, uint8_t* rect2, uint8_t* valid, uint8_t* color, int16_t* disp16, int cap, float* xyz,
                            uint8_t* cloud_color, int32_t* pixel, int32_t* count, int speckle_size, int speckle_diff16, int32_t* removed)
{
    const gms_stereo_sgm_params& p = dense_sgm_params(params);
    if (!camera || !img1 || !img2 || !R || !t || !plan || !count || min_disp16 < 1 || cap < 0 || (cap > 0 && (!xyz || !pixel))) return GMS_ERR_BAD_ARG;
    if (speckle_size < 0 || speckle_diff16 < 0) return GMS_ERR_BAD_ARG;
    const int rc = gms_rectify_plan_host(camera, R, t, width, height, out_w, out_h, plan);
    if (rc != GMS_OK) return rc;
    if (plan->status != GMS_OK) return GMS_ERR_NO_MODEL;
    const int ow = plan->out_w, oh = plan->out_h;
    const size_t ws = speckle_size > 0 ? gms_dense_pairs_filtered_workspace_bytes(width, height, channels, ow, oh, 1, &p)
                                       : gms_dense_pairs_workspace_bytes(width, height, channels, ow, oh, 1, &p);
    if (ws == 0) return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)width * (size_t)height * (size_t)channels, px = (size_t)ow * (size_t)oh, ucap = (size_t)cap;
    gms::BlockLayout lay;
    const size_t o_1 = lay.add(s_bytes), o_2 = lay.add(s_bytes), o_plan = lay.add(sizeof(gms_rectify_plan)), o_ws = lay.add(ws), o_r1 = lay.add(px),
                 o_r2 = lay.add(px), o_v = lay.add(px), o_c = lay.add(3 * px), o_d = lay.add(2 * px), o_xyz = lay.add(12 * ucap + 4),
                 o_cc = lay.add(3 * ucap + 4), o_pix = lay.add(4 * ucap + 4), o_n = lay.add(4), o_rm = lay.add(4);
    DevBlock blk(lay, nullptr);
    blk.in(o_1, img1, s_bytes);
    blk.in(o_2, img2, s_bytes);
    blk.in(o_plan, plan, sizeof(gms_rectify_plan));
    blk.run([&](hipStream_t st) {
        return dense_pairs_launch(*camera, p, blk.at<uint8_t>(o_1), blk.at<uint8_t>(o_2), 1, width, height, channels, ow, oh, min_disp16, nullptr, nullptr,
                                  nullptr, 0, blk.at(o_ws), blk.at<gms_rectify_plan>(o_plan), blk.at<uint8_t>(o_r1), blk.at<uint8_t>(o_r2),
                                  blk.at<uint8_t>(o_v), blk.at<uint8_t>(o_c), blk.at<int16_t>(o_d), cap, blk.at<float>(o_xyz),
                                  cloud_color ? blk.at<uint8_t>(o_cc) : nullptr, blk.at<int32_t>(o_pix), blk.at<int32_t>(o_n), speckle_size,
                                  speckle_diff16, removed ? blk.at<int32_t>(o_rm) : nullptr, st);
    });
    int32_t n = 0;
    blk.out_now(&n, o_n, 4);
    *count = n;
    if (removed) blk.out(removed, o_rm, 4);
    const size_t k = (size_t)(n < cap ? n : cap);
    if (rect1) blk.out(rect1, o_r1, px);
    if (rect2) blk.out(rect2, o_r2, px);
    if (valid) blk.out(valid, o_v, px);
    if (color && channels == 3) blk.out(color, o_c, 3 * px);
    if (disp16) blk.out(disp16, o_d, 2 * px);
    if (k && blk.ok()) {
        blk.out(xyz, o_xyz, 12 * k);
        blk.out(pixel, o_pix, 4 * k);
        if (cloud_color) blk.out(cloud_color, o_cc, (size_t)channels * k);
    }
    return blk.finish();
}

int gms_dense_pair(const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* img1, const uint8_t* img2, int width, int height,
                   int channels, const double* R, const double* t, int out_w, int out_h, int min_disp16, gms_rectify_plan* plan, uint8_t* rect1,
                   uint8_t* rect2, uint8_t* valid, uint8_t* color, int16_t* disp16, int cap, float* xyz, uint8_t* cloud_color, int32_t* pixel,
                   int32_t* count)
{
    return gms_dense_pair_filtered(camera, params, img1, img2, width, height, channels, R, t, out_w, out_h, min_disp16, plan, rect1, rect2, valid, color,
                                   disp16, cap, xyz, cloud_color, pixel, count, 0, 0, nullptr);
}

// ---- the clouds of several pairs fused into one (dense_fuse_kernels.hip, dense_fuse_core.h) ----------------------
static_assert(sizeof(gms_dense_fuse_src) == 88, "gms_dense_fuse_src: eight pointers and six 32-bit words");

size_t gms_dense_fuse_workspace_bytes(int n_src, int max_cap)
{
    if (!fuse::call_args_ok(n_src, max_cap, 1, 1, 0, 1, 0)) return 0;
    return gms::dense_fuse_ws_bytes(n_src, max_cap);
}

int gms_dense_fuse_device(gms_ctx* c, const gms_dense_fuse_src* d_src, int n_src, int max_cap, const int32_t* d_neighbors, int n_nb, int channels,
                          int tol16, int min_support, void* d_ws, size_t ws_bytes, int fused_cap, float* d_xyz, uint8_t* d_color, int32_t* d_source,
                          int32_t* d_index, uint8_t* d_support, uint8_t* d_conflict, int32_t* d_counts)
{
    if (!c || !fuse::call_args_ok(n_src, max_cap, n_nb, channels, tol16, min_support, fused_cap)) return GMS_ERR_BAD_ARG;
    if (!d_src || !d_neighbors || !d_ws || !d_counts || (fused_cap > 0 && (!d_xyz || !d_source || !d_index || !d_support || !d_conflict)))
        return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::dense_fuse_ws_bytes(n_src, max_cap)) || misaligned(d_src, 8) || misaligned(d_neighbors, 4) ||
        misaligned(d_xyz, 4) || misaligned(d_source, 4) || misaligned(d_index, 4) || misaligned(d_counts, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_dense_fuse(d_src, n_src, max_cap, d_neighbors, n_nb, channels, tol16, min_support, d_ws, fused_cap, d_xyz, d_color, d_source,
                                      d_index, d_support, d_conflict, d_counts, c->stream);
    });
}

int gms_dense_fuse(const gms_dense_fuse_src* src, int n_src, const int32_t* neighbors, int n_nb, int channels, int tol16, int min_support,
                   int fused_cap, float* xyz, uint8_t* color, int32_t* source, int32_t* index, uint8_t* support, uint8_t* conflict, int32_t* counts)
{
    if (!src || n_src < 1 || n_src > 65535 || !neighbors || !counts || (fused_cap > 0 && (!xyz || !source || !index || !support || !conflict)))
        return GMS_ERR_BAD_ARG;
    long long max_cap = 1;
    for (int i = 0; i < n_src; ++i) {
        const gms_dense_fuse_src& s = src[i];
        if (!fuse::shape_ok(s, fuse::kMaxCap) || !s.d_disp16 || !s.d_valid || !s.d_plan || !s.d_count || (s.cap > 0 && !s.d_xyz)) return GMS_ERR_BAD_ARG;
        if (s.cap > max_cap) max_cap = s.cap;
    }
    if (!fuse::call_args_ok(n_src, max_cap, n_nb, channels, tol16, min_support, fused_cap)) return GMS_ERR_BAD_ARG;
    const size_t ws = gms::dense_fuse_ws_bytes(n_src, (int)max_cap), ucap = (size_t)fused_cap, un = (size_t)n_src;
    // one block: the table, the neighbours, the workspace, the outputs, then every source's arrays
    struct Off { size_t disp, valid, plan, xyz, color, count, view, reg; };
    std::vector<Off> off(un);
    gms::BlockLayout lay;
    const size_t o_tab = lay.add(sizeof(gms_dense_fuse_src) * un), o_nb = lay.add(4 * un * (size_t)n_nb), o_ws = lay.add(ws), o_xyz = lay.add(12 * ucap + 4),
                 o_col = lay.add(3 * ucap + 4), o_src = lay.add(4 * ucap + 4), o_idx = lay.add(4 * ucap + 4), o_sup = lay.add(ucap + 4),
                 o_con = lay.add(ucap + 4), o_cnt = lay.add(4 * (un + 1));
    for (size_t i = 0; i < un; ++i) {
        const gms_dense_fuse_src& s = src[i];
        const size_t px = (size_t)s.width * (size_t)s.height, cap = (size_t)s.cap;
        off[i] = {lay.add(2 * px), lay.add(px), lay.add(sizeof(gms_rectify_plan)), lay.add(12 * cap + 4), lay.add(s.d_color ? channels * cap + 4 : 4),
                  lay.add(4), lay.add(sizeof(gms_sfm_view)), lay.add(sizeof(gms_sfm_pair_reg))};
    }
    DevBlock blk(lay, nullptr);
    std::vector<gms_dense_fuse_src> tab(src, src + n_src);
    for (size_t i = 0; i < un; ++i) {
        const gms_dense_fuse_src& s = src[i];
        const size_t px = (size_t)s.width * (size_t)s.height, cap = (size_t)s.cap;
        blk.in(off[i].disp, s.d_disp16, 2 * px);
        blk.in(off[i].valid, s.d_valid, px);
        blk.in(off[i].plan, s.d_plan, sizeof(gms_rectify_plan));
        blk.in(off[i].count, s.d_count, 4);
        if (cap) blk.in(off[i].xyz, s.d_xyz, 12 * cap);
        if (cap && s.d_color) blk.in(off[i].color, s.d_color, channels * cap);
        if (s.d_view) blk.in(off[i].view, s.d_view, sizeof(gms_sfm_view));
        if (s.d_reg) blk.in(off[i].reg, s.d_reg, sizeof(gms_sfm_pair_reg));
        tab[i].d_disp16 = blk.at<int16_t>(off[i].disp);
        tab[i].d_valid = blk.at<uint8_t>(off[i].valid);
        tab[i].d_plan = blk.at<gms_rectify_plan>(off[i].plan);
        tab[i].d_xyz = blk.at<float>(off[i].xyz);
        tab[i].d_color = s.d_color ? blk.at<uint8_t>(off[i].color) : nullptr;
        tab[i].d_count = blk.at<int32_t>(off[i].count);
        tab[i].d_view = s.d_view ? blk.at<gms_sfm_view>(off[i].view) : nullptr;
        tab[i].d_reg = s.d_reg ? blk.at<gms_sfm_pair_reg>(off[i].reg) : nullptr;
    }
    blk.in(o_tab, tab.data(), sizeof(gms_dense_fuse_src) * un);
    blk.in(o_nb, neighbors, 4 * un * (size_t)n_nb);
    blk.run([&](hipStream_t st) {
        return gms::launch_dense_fuse(blk.at<gms_dense_fuse_src>(o_tab), n_src, (int)max_cap, blk.at<int32_t>(o_nb), n_nb, channels, tol16, min_support,
                                      blk.at(o_ws), fused_cap, blk.at<float>(o_xyz), color ? blk.at<uint8_t>(o_col) : nullptr, blk.at<int32_t>(o_src),
                                      blk.at<int32_t>(o_idx), blk.at<uint8_t>(o_sup), blk.at<uint8_t>(o_con), blk.at<int32_t>(o_cnt), st);
    });
    blk.out_now(counts, o_cnt, 4 * (un + 1));  // (also waits for the copies in: `tab` is read until then)
    const size_t k = blk.ok() ? (size_t)(counts[n_src] < fused_cap ? counts[n_src] : fused_cap) : 0;
    if (k) {
        blk.out(xyz, o_xyz, 12 * k);
        if (color) blk.out(color, o_col, (size_t)channels * k);
        blk.out(source, o_src, 4 * k);
        blk.out(index, o_idx, 4 * k);
        blk.out(support, o_sup, k);
        blk.out(conflict, o_con, k);
    }
    return blk.finish();
}

}  // extern "C"
