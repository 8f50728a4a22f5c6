// capi_image.cpp -- the C ABI of the image operations: portrait mode and the median blur, resize / warpAffine / img_rotate, and
// rectification (the plan, the remap, undistort).
#include "capi_common.h"
#include "gms_kernels.h"
#include "portrait_core.h"
#include "rectify_core.h"
#include "warp_core.h"

extern "C" {

// ---- portrait mode (portrait_kernels.hip) --------------------------------------------------------------------------
GMS_PARAMS_OR(pm_params, gms_portrait_params, GMS_PORTRAIT_PARAMS_REFERENCE)

size_t gms_portrait_workspace_bytes(int width, int height, int n, const gms_portrait_params* params)
{
    if (n < 1 || n > 65535 || !pm::params_ok(pm_params(params), width, height)) return 0;
    return gms::portrait_ws_bytes(n, width, height);
}

int gms_portrait_device(gms_ctx* c, const gms_portrait_params* params, const uint8_t* d_bgr, const uint8_t* d_disparity, int n, int width,
                        int height, int pitch_bgr, int pitch_disp, void* d_ws, size_t ws_bytes, uint8_t* d_out_bgr, uint8_t* d_mask,
                        uint8_t* d_selected, uint8_t* d_blurred)
{
    const gms_portrait_params& p = pm_params(params);
    if (!c || n < 1 || n > 65535 || !pm::params_ok(p, width, height) || pitch_bgr < 3 * width || pitch_disp < width) return GMS_ERR_BAD_ARG;
    if (!d_bgr || !d_disparity || !d_ws || !d_out_bgr || !ws_ok(d_ws, ws_bytes, gms::portrait_ws_bytes(n, width, height))) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_portrait(p, d_bgr, d_disparity, n, width, height, pitch_bgr, pitch_disp, d_ws, d_out_bgr, d_mask, d_selected, d_blurred,
                                    c->stream);
    });
}

int gms_portrait_profile_device(gms_ctx* c, const gms_portrait_params* params, const uint8_t* d_bgr, const uint8_t* d_disparity, int n,
                                int width, int height, int pitch_bgr, int pitch_disp, void* d_ws, size_t ws_bytes, uint8_t* d_out_bgr,
                                uint8_t* d_mask, uint8_t* d_selected, uint8_t* d_blurred, float* stage_ms)
{
    const gms_portrait_params& p = pm_params(params);
    if (!c || !stage_ms || n < 1 || n > 65535 || !pm::params_ok(p, width, height) || pitch_bgr < 3 * width || pitch_disp < width)
        return GMS_ERR_BAD_ARG;
    if (!d_bgr || !d_disparity || !d_ws || !d_out_bgr || !ws_ok(d_ws, ws_bytes, gms::portrait_ws_bytes(n, width, height))) return GMS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    hipEvent_t ev[GMS_PORTRAIT_STAGES + 1] = {};
    hipError_t e = hipSuccess;
    for (int i = 0; i <= GMS_PORTRAIT_STAGES && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    if (e == hipSuccess)
        e = gms::launch_portrait(p, d_bgr, d_disparity, n, width, height, pitch_bgr, pitch_disp, d_ws, d_out_bgr, d_mask, d_selected,
                                 d_blurred, c->stream, ev);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    for (int i = 0; i < GMS_PORTRAIT_STAGES && e == hipSuccess; i++) e = hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]);
    for (int i = 0; i <= GMS_PORTRAIT_STAGES; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    GMS_HIP(e);
    return GMS_OK;
}

int gms_median_blur_device(gms_ctx* c, const uint8_t* d_src, int n, int width, int height, int channels, int pitch, int ksize,
                           uint8_t* d_dst)
{
    if (!c || n < 1 || n > 65535 || !pm::median_ok(width, height, channels, ksize) || pitch < channels * width || !d_src || !d_dst)
        return GMS_ERR_BAD_ARG;
    const uintptr_t span = (uintptr_t)n * (uintptr_t)height * (uintptr_t)pitch;
    if (ranges_overlap(d_src, span, d_dst, span)) return GMS_ERR_BAD_ARG;  // the destination may not overlap the source
    return on_ctx(c, [&] { return gms::launch_median_blur(d_src, n, width, height, channels, pitch, ksize, d_dst, c->stream); });
}

int gms_median_blur(const uint8_t* src, int width, int height, int channels, int ksize, uint8_t* dst)
{
    if (!pm::median_ok(width, height, channels, ksize) || !src || !dst) return GMS_ERR_BAD_ARG;
    const size_t bytes = (size_t)width * (size_t)height * (size_t)channels;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(bytes), o_dst = lay.add(bytes);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, bytes);
    blk.run([&](hipStream_t st) {
        return gms::launch_median_blur(blk.at<uint8_t>(o_src), 1, width, height, channels, width * channels, ksize, blk.at<uint8_t>(o_dst), st);
    });
    blk.out(dst, o_dst, bytes);
    return blk.finish();
}

int gms_portrait(const gms_portrait_params* params, const uint8_t* bgr, const uint8_t* disparity, int width, int height, uint8_t* out_bgr,
                 uint8_t* mask, uint8_t* selected, uint8_t* blurred)
{
    const gms_portrait_params& p = pm_params(params);
    if (!pm::params_ok(p, width, height) || !bgr || !disparity || !out_bgr) return GMS_ERR_BAD_ARG;
    const size_t px = (size_t)width * (size_t)height;
    gms::BlockLayout lay;
    const size_t o_img = lay.add(3 * px), o_d = lay.add(px), o_ws = lay.add(gms::portrait_ws_bytes(1, width, height)), o_out = lay.add(3 * px);
    const size_t o_m = lay.add(px), o_s = lay.add(px), o_b = lay.add(3 * px);
    DevBlock blk(lay, nullptr);
    blk.in(o_img, bgr, 3 * px);
    blk.in(o_d, disparity, px);
    blk.run([&](hipStream_t st) {
        return gms::launch_portrait(p, blk.at<uint8_t>(o_img), blk.at<uint8_t>(o_d), 1, width, height, 3 * width, width, blk.at(o_ws),
                                    blk.at<uint8_t>(o_out), mask ? blk.at<uint8_t>(o_m) : nullptr, selected ? blk.at<uint8_t>(o_s) : nullptr,
                                    blurred ? blk.at<uint8_t>(o_b) : nullptr, st);
    });
    blk.out(out_bgr, o_out, 3 * px);
    if (mask) blk.out(mask, o_m, px);
    if (selected) blk.out(selected, o_s, px);
    if (blurred) blk.out(blurred, o_b, 3 * px);
    return blk.finish();
}

// ---- resize and warpAffine (warp_kernels.hip) ----------------------------------------------------------------------
static bool warp_ranges_ok(const uint8_t* d_src, int n, int sh, int src_pitch, const uint8_t* d_dst, int dh, int dst_pitch)
{
    if (!d_src || !d_dst) return false;
    const uintptr_t s_span = (uintptr_t)n * (uintptr_t)sh * (uintptr_t)src_pitch, d_span = (uintptr_t)n * (uintptr_t)dh * (uintptr_t)dst_pitch;
    return !ranges_overlap(d_src, s_span, d_dst, d_span);  // the destination may not overlap the source
}

int gms_resize_device(gms_ctx* c, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, uint8_t* d_dst, int dw, int dh,
                      int dst_pitch)
{
    if (!c || !warp::args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) || !warp_ranges_ok(d_src, n, sh, src_pitch, d_dst, dh, dst_pitch))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_resize(d_src, n, sw, sh, channels, src_pitch, d_dst, dw, dh, dst_pitch, c->stream); });
}

int gms_warp_affine_device(gms_ctx* c, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, const double* d_M,
                           int n_matrices, uint8_t* d_dst, int dw, int dh, int dst_pitch)
{
    if (!c || !d_M || (n_matrices != 1 && n_matrices != n) || !warp::args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) ||
        !warp_ranges_ok(d_src, n, sh, src_pitch, d_dst, dh, dst_pitch))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_warp_affine(d_src, n, sw, sh, channels, src_pitch, d_M, n_matrices, d_dst, dw, dh, dst_pitch, c->stream);
    });
}

int gms_rotation_matrix_2d(double center_x, double center_y, double angle, double scale, double* M)
{
    if (!M) return GMS_ERR_BAD_ARG;
    warp::rotation_matrix_2d(center_x, center_y, angle, scale, M);
    return GMS_OK;
}

int gms_resize(const uint8_t* src, int sw, int sh, int channels, uint8_t* dst, int dw, int dh)
{
    if (!src || !dst || !warp::args_ok(1, sw, sh, channels, (long long)channels * sw, dw, dh, (long long)channels * dw)) return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)sw * (size_t)sh * (size_t)channels, d_bytes = (size_t)dw * (size_t)dh * (size_t)channels;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(s_bytes), o_dst = lay.add(d_bytes);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, s_bytes);
    blk.run([&](hipStream_t st) {
        return gms::launch_resize(blk.at<uint8_t>(o_src), 1, sw, sh, channels, sw * channels, blk.at<uint8_t>(o_dst), dw, dh, dw * channels, st);
    });
    blk.out(dst, o_dst, d_bytes);
    return blk.finish();
}

int gms_warp_affine(const uint8_t* src, int sw, int sh, int channels, const double* M, uint8_t* dst, int dw, int dh)
{
    if (!src || !dst || !M || !warp::args_ok(1, sw, sh, channels, (long long)channels * sw, dw, dh, (long long)channels * dw))
        return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)sw * (size_t)sh * (size_t)channels, d_bytes = (size_t)dw * (size_t)dh * (size_t)channels;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(s_bytes), o_M = lay.add(6 * sizeof(double)), o_dst = lay.add(d_bytes);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, s_bytes);
    blk.in(o_M, M, 6 * sizeof(double));
    blk.run([&](hipStream_t st) {
        return gms::launch_warp_affine(blk.at<uint8_t>(o_src), 1, sw, sh, channels, sw * channels, blk.at<double>(o_M), 1, blk.at<uint8_t>(o_dst),
                                       dw, dh, dw * channels, st);
    });
    blk.out(dst, o_dst, d_bytes);
    return blk.finish();
}

int gms_img_rotate(const uint8_t* src, int width, int height, int channels, double angle, uint8_t* dst)
{
    double M[6];
    warp::rotation_matrix_2d(width / 2., height / 2., angle, 1.0, M);
    return gms_warp_affine(src, width, height, channels, M, dst, width, height);
}

// ---- a dense cloud from a posed pair (rectify_kernels.hip, rectify_core.h): the plan and the remap; the cloud itself is capi_dense.cpp
static_assert(sizeof(gms_rectify_plan) == 200, "gms_rectify_plan: 23 doubles and four 32-bit words");

int gms_rectify_plan_host(const gms_camera* camera, const double* R, const double* t, int width, int height, int out_w, int out_h,
                          gms_rectify_plan* plan)
{
    if (!camera || !R || !t || !plan || !warp::side_ok(width) || !warp::side_ok(height) || out_w > warp::kMaxSide || out_h > warp::kMaxSide)
        return GMS_ERR_BAD_ARG;
    rect::make_plan(rect::camera_of(*camera), R, t, width, height, out_w, out_h, *plan);
    return GMS_OK;
}

int gms_rectify_plan_device(gms_ctx* c, const gms_camera* camera, const gms_two_view* d_tv, int n_pairs, int width, int height, int out_w,
                            int out_h, gms_rectify_plan* d_plans)
{
    if (!c || !camera || n_pairs < 0 || n_pairs > 65535 || !warp::side_ok(width) || !warp::side_ok(height) || out_w > warp::kMaxSide ||
        out_h > warp::kMaxSide)
        return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_tv || !d_plans) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_rectify_plan(*camera, d_tv, n_pairs, width, height, out_w, out_h, d_plans, c->stream); });
}

int gms_rectify_q(const gms_rectify_plan* plan, double* Q)
{
    if (!plan || !Q) return GMS_ERR_BAD_ARG;
    rect::plan_q(*plan, Q);
    return GMS_OK;
}

int gms_rectify_device(gms_ctx* c, const gms_camera* camera, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch,
                       const gms_rectify_plan* d_plans, int n_plans, int which, uint8_t* d_dst, int dw, int dh, int dst_pitch,
                       uint8_t* d_valid)
{
    if (!c || !camera || !d_plans || misaligned(d_plans, 8) || (n_plans != 1 && n_plans != n) || (which != 1 && which != 2) ||
        !rect::image_args_ok(n, sw, sh, channels, src_pitch, dw, dh, dst_pitch) || !warp_ranges_ok(d_src, n, sh, src_pitch, d_dst, dh, dst_pitch))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_rectify(*camera, d_src, n, sw, sh, channels, src_pitch, d_plans, n_plans, which, d_dst, dw, dh, dst_pitch, d_valid,
                                   c->stream);
    });
}

int gms_rectify(const gms_camera* camera, const gms_rectify_plan* plan, int which, const uint8_t* src, int sw, int sh, int channels,
                uint8_t* dst, uint8_t* valid)
{
    if (!camera || !plan || !src || !dst || (which != 1 && which != 2)) return GMS_ERR_BAD_ARG;
    const int dw = plan->out_w, dh = plan->out_h;
    if (!rect::image_args_ok(1, sw, sh, channels, (long long)channels * sw, dw, dh, (long long)channels * dw)) return GMS_ERR_BAD_ARG;
    const size_t s_bytes = (size_t)sw * (size_t)sh * (size_t)channels, d_px = (size_t)dw * (size_t)dh;
    gms::BlockLayout lay;
    const size_t o_src = lay.add(s_bytes), o_plan = lay.add(sizeof(gms_rectify_plan)), o_dst = lay.add(d_px * channels), o_valid = lay.add(d_px);
    DevBlock blk(lay, nullptr);
    blk.in(o_src, src, s_bytes);
    blk.in(o_plan, plan, sizeof(gms_rectify_plan));
    blk.run([&](hipStream_t st) {
        return gms::launch_rectify(*camera, blk.at<uint8_t>(o_src), 1, sw, sh, channels, sw * channels, blk.at<gms_rectify_plan>(o_plan), 1, which,
                                   blk.at<uint8_t>(o_dst), dw, dh, dw * channels, valid ? blk.at<uint8_t>(o_valid) : nullptr, st);
    });
    blk.out(dst, o_dst, d_px * channels);
    if (valid) blk.out(valid, o_valid, d_px);
    return blk.finish();
}

int gms_undistort(const gms_camera* camera, const uint8_t* src, int width, int height, int channels, uint8_t* dst)
{
    if (!camera || !warp::side_ok(width) || !warp::side_ok(height)) return GMS_ERR_BAD_ARG;
    gms_rectify_plan plan;
    rect::identity_plan(rect::camera_of(*camera), width, height, plan);
    return gms_rectify(camera, &plan, 1, src, width, height, channels, dst, nullptr);
}

}  // extern "C"
