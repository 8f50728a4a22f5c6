// capi_twoview.cpp -- the C ABI of the matches' consumers (consumer_kernels.hip, twoview_kernels.hip): the disparity map, the points,
// the essential matrix, the pose and the triangulation of one pair or of a batch of pairs, and the two device self-tests.
#include "capi_common.h"
#include "gms_kernels.h"
#include "twoview_core.h"

static_assert(sizeof(gms_two_view) == 232 && sizeof(gms_camera) == 72, "two-view records");

// The scratch of gms_recover_pose_device (vote bytes + counters): grown like the filter's workspaces -- never inside a stream
// capture, and only after everything that may still use the old block has finished.
int gms::grow_pose_ws(gms_ctx* c, size_t bytes, hipStream_t st)
{
    if (bytes <= c->pose_ws.cap) return GMS_OK;
    if (stream_is_capturing(st)) return GMS_ERR_NOT_RESERVED;
    GMS_HIP(hipStreamSynchronize(st));
    GMS_HIP(hipDeviceSynchronize());  // (an earlier call may have run on another stream of the caller's)
    GMS_HIP(c->pose_ws.reserve(bytes));
    return GMS_OK;
}

extern "C" {

int gms_disparity_device(gms_ctx* c, const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2,
                         const gms_dmatch* d_matches, const int32_t* d_n_matches, int max_matches, int width, int height,
                         const uint8_t* d_gt, int disp_ratio, uint8_t* d_disparity, uint32_t* d_work, gms_disparity_stats* d_stats)
{
    if (!c || n1 < 0 || n2 < 0 || max_matches < 0 || width <= 0 || height <= 0) return GMS_ERR_BAD_ARG;
    if (!d_n_matches || !d_disparity || !d_work || !d_stats || (d_gt && disp_ratio == 0)) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_kp1 || !d_kp2 || !d_matches)) return GMS_ERR_BAD_ARG;
    if (max_matches >= (1 << 24)) return GMS_ERR_CAPACITY;  // the scatter key keeps the match index in 24 bits
    return on_ctx(c, [&] {
        return gms::launch_disparity(d_kp1, n1, d_kp2, n2, d_matches, d_n_matches, max_matches, width, height, d_gt, disp_ratio, d_disparity, d_work,
                                     d_stats, c->stream);
    });
}

int gms_gather_points_device(gms_ctx* c, const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2,
                             const gms_dmatch* d_matches, const int32_t* d_n_matches, int max_matches,
                             float* d_coords1, float* d_coords2, int32_t* d_status)
{
    if (!c || n1 < 0 || n2 < 0 || max_matches < 0 || !d_n_matches || !d_status) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_kp1 || !d_kp2 || !d_matches || !d_coords1 || !d_coords2)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_gather_points(d_kp1, n1, d_kp2, n2, d_matches, d_n_matches, max_matches, d_coords1, d_coords2, d_status, c->stream);
    });
}

int gms_triangulate_device(gms_ctx* c, const double camera[4], const double dist[5], const double P1[12], const double P2[12],
                           const float* d_coords1, const float* d_coords2, const int32_t* d_n_matches, int max_matches,
                           double* d_points3d, gms_triangulation_stats* d_stats)
{
    if (!c || !camera || !P1 || !P2 || !d_n_matches || !d_stats || max_matches < 0) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_coords1 || !d_coords2 || !d_points3d)) return GMS_ERR_BAD_ARG;
    if (camera[0] == 0.0 || camera[1] == 0.0) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_triangulate(camera, dist, P1, P2, d_coords1, d_coords2, d_n_matches, max_matches, d_points3d, d_stats, c->stream);
    });
}

int gms_recover_pose_device(gms_ctx* c, const double E[9], const double camera[4], const float* d_coords1, const float* d_coords2,
                            const int32_t* d_n_matches, int max_matches, const uint8_t* d_in_mask, gms_pose* d_pose, uint8_t* d_out_mask)
{
    if (!c || !E || !camera || !d_n_matches || !d_pose || max_matches < 0) return GMS_ERR_BAD_ARG;
    if (max_matches > 0 && (!d_coords1 || !d_coords2)) return GMS_ERR_BAD_ARG;
    if (camera[0] == 0.0 || camera[1] == 0.0) return GMS_ERR_BAD_ARG;
    double R1[9], R2[9], t[3];
    if (!gms::tv::decompose_essential(E, R1, R2, t)) return GMS_ERR_BAD_ARG;  // cv::decomposeEssentialMat (twoview_core.h)
    double P[4][12];
    for (int h = 0; h < 4; ++h) {
        const double* R = (h & 1) ? R2 : R1;
        const double sg = h < 2 ? 1.0 : -1.0;
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) P[h][4 * r + k] = R[3 * r + k];
            P[h][4 * r + 3] = sg * t[r];
        }
    }
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    GMS_TRY(gms::grow_pose_ws(c, (size_t)max_matches + 48, c->stream));
    GMS_HIP(gms::launch_recover_pose(camera, P, 50.0, d_coords1, d_coords2, d_n_matches, max_matches, d_in_mask, d_pose, d_out_mask,
                                     c->pose_ws.p, c->stream));
    return GMS_OK;
}

// ---- the batched consumers (twoview_kernels.hip): nothing but launches on the context's stream --------------------------------
static bool camera_ok(const gms_camera* cam) { return cam && cam->fx != 0.0 && cam->fy != 0.0; }

int gms_gather_points_batch_device(gms_ctx* c, const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs,
                                   int n_pairs, int max_m, const gms_dmatch* d_filtered, const gms_pair_result* d_results, float* d_coords1,
                                   float* d_coords2, gms_two_view* d_tv)
{
    if (!c || n_frames < 0 || n_pairs < 0 || max_m < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_frame_off || !d_pairs || !d_results || !d_tv) return GMS_ERR_BAD_ARG;
    if (max_m > 0 && (!d_kp || !d_filtered || !d_coords1 || !d_coords2)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_gather_batch(d_kp, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_coords1, d_coords2, d_tv,
                                        c->stream);
    });
}

int gms_find_essential_batch_device(gms_ctx* c, const gms_camera* camera, double prob, double threshold, int max_iters, const gms_pair* d_pairs,
                                    int n_pairs, const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv)
{
    if (!c || n_pairs < 0 || !camera_ok(camera)) return GMS_ERR_BAD_ARG;
    if (!(prob > 0.0 && prob < 1.0) || !(threshold > 0.0) || max_iters < 1) return GMS_ERR_BAD_ARG;  // (CV_Assert(confidence > 0 && confidence < 1))
    if (n_pairs == 0) return GMS_OK;
    if (!d_pairs || !d_coords1 || !d_coords2 || !d_mask || !d_tv) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_find_essential_batch(*camera, prob, threshold, max_iters, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv, c->stream);
    });
}

int gms_recover_pose_batch_device(gms_ctx* c, const gms_camera* camera, int use_in_mask, const gms_pair* d_pairs, int n_pairs,
                                  const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv)
{
    if (!c || n_pairs < 0 || !camera_ok(camera)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_pairs || !d_coords1 || !d_coords2 || !d_mask || !d_tv) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_recover_pose_batch(*camera, 50.0, use_in_mask ? 1 : 0, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv, c->stream);
    });
}

int gms_triangulate_batch_device(gms_ctx* c, const gms_camera* camera, const gms_pair* d_pairs, int n_pairs, const float* d_coords1,
                                 const float* d_coords2, const uint8_t* d_mask, double* d_points3d, gms_two_view* d_tv)
{
    if (!c || n_pairs < 0 || !camera_ok(camera)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_pairs || !d_coords1 || !d_coords2 || !d_points3d || !d_tv) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_triangulate_batch(*camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_points3d, d_tv, c->stream);
    });
}

int gms_two_view_batch_device(gms_ctx* c, const gms_camera* camera, double prob, double threshold, int max_iters, const gms_keypoint* d_kp,
                              const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_m,
                              const gms_dmatch* d_filtered, const gms_pair_result* d_results, float* d_coords1, float* d_coords2,
                              uint8_t* d_mask, double* d_points3d, gms_two_view* d_tv)
{
    GMS_TRY(gms_gather_points_batch_device(c, d_kp, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_coords1, d_coords2, d_tv));
    GMS_TRY(gms_find_essential_batch_device(c, camera, prob, threshold, max_iters, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv));
    GMS_TRY(gms_recover_pose_batch_device(c, camera, 1, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv));
    return gms_triangulate_batch_device(c, camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_points3d, d_tv);
}

int gms_disparity_batch_device(gms_ctx* c, const gms_keypoint* d_kp, const int64_t* d_frame_off, const int32_t* d_wh, int n_frames,
                               const gms_pair* d_pairs, int n_pairs, int max_m, const gms_dmatch* d_filtered, const gms_pair_result* d_results,
                               const uint8_t* d_gt, int64_t gt_stride, int disp_ratio, uint8_t* d_disparity, int64_t map_stride, uint32_t* d_work,
                               gms_disparity_stats* d_stats)
{
    if (!c || n_frames < 0 || n_pairs < 0 || max_m < 0 || map_stride <= 0 || gt_stride < 0) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_frame_off || !d_wh || !d_pairs || !d_results || !d_disparity || !d_work || !d_stats || (d_gt && disp_ratio == 0)) return GMS_ERR_BAD_ARG;
    if (max_m > 0 && (!d_kp || !d_filtered)) return GMS_ERR_BAD_ARG;
    if (max_m >= (1 << 24)) return GMS_ERR_CAPACITY;  // the scatter key keeps the match index in 24 bits
    return on_ctx(c, [&] {
        return gms::launch_disparity_batch(d_kp, d_frame_off, d_wh, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_gt, gt_stride,
                                           disp_ratio, d_disparity, map_stride, d_work, d_stats, c->stream);
    });
}

int gms_selftest_five_point(gms_ctx* c, const double* pts, int n_samples, double* models, int32_t* counts)
{
    if (!c || n_samples < 0 || (n_samples > 0 && (!pts || !models || !counts))) return GMS_ERR_BAD_ARG;
    if (n_samples == 0) return GMS_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    const size_t b_pts = (size_t)n_samples * 20 * 8, b_models = (size_t)n_samples * 90 * 8, b_counts = (size_t)n_samples * 4;
    GMS_HIP(hipStreamSynchronize(c->stream));
    GMS_HIP(c->aux.reserve(b_pts + b_models + b_counts));
    double* d_pts = (double*)c->aux.p;
    double* d_models = d_pts + (size_t)n_samples * 20;
    int* d_counts = (int*)(d_models + (size_t)n_samples * 90);
    GMS_HIP(hipMemcpyAsync(d_pts, pts, b_pts, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(gms::launch_five_point_selftest(d_pts, n_samples, d_models, d_counts, c->stream));
    GMS_HIP(hipMemcpyAsync(models, d_models, b_models, hipMemcpyDeviceToHost, c->stream));
    GMS_HIP(hipMemcpyAsync(counts, d_counts, b_counts, hipMemcpyDeviceToHost, c->stream));
    GMS_HIP(hipStreamSynchronize(c->stream));
    return GMS_OK;
}

int gms_selftest_threshold(gms_ctx* c, const int32_t* T, const int32_t* n, const int32_t* score, double factor,
                           int count, uint8_t* out)
{
    if (!c || count < 0 || (count > 0 && (!T || !n || !score || !out))) return GMS_ERR_BAD_ARG;
    if (count == 0) return GMS_OK;
    std::lock_guard<std::mutex> lock(c->mu);
    GMS_HIP(hipSetDevice(c->device));
    const size_t nb = (size_t)count * 4;
    GMS_HIP(c->aux.reserve(3 * nb + (size_t)count));
    int32_t* dT = (int32_t*)c->aux.p;
    int32_t* dn = dT + count;
    int32_t* ds = dn + count;
    uint8_t* dout = (uint8_t*)(ds + count);
    GMS_HIP(hipMemcpyAsync(dT, T, nb, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(hipMemcpyAsync(dn, n, nb, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(hipMemcpyAsync(ds, score, nb, hipMemcpyHostToDevice, c->stream));
    GMS_HIP(gms::launch_threshold(dT, dn, ds, factor, count, dout, c->stream));
    GMS_HIP(hipMemcpyAsync(out, dout, (size_t)count, hipMemcpyDeviceToHost, c->stream));
    GMS_HIP(hipStreamSynchronize(c->stream));
    return GMS_OK;
}

}  // extern "C"
