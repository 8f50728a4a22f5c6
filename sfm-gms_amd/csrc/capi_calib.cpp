// capi_calib.cpp -- the C ABI of camera calibration: chessboard corner candidates, sub-pixel corners, calibrateCamera.
#include <algorithm>
#include <vector>

#include "calib_core.h"
#include "capi_common.h"
#include "gms_kernels.h"

extern "C" {

// ---- camera calibration from chessboard photographs (calib_kernels.hip, calib_core.h) -----------------------------
static_assert(sizeof(gms_chess_candidate) == 12 && sizeof(calib::Candidate) == 12, "candidate records are three 32-bit words");
static_assert(GMS_CHESS_MAX_CANDIDATES == calib::kMaxCandidates && GMS_WARP_MAX_SIDE == calib::kMaxSide && GMS_DETECT_BORDER == calib::kBorder,
              "gms.h and calib_core.h state the same limits");

size_t gms_chess_candidates_workspace_bytes(int width, int height, int n_images)
{
    if (!calib::batch_ok(n_images, width, height, 1)) return 0;
    return gms::chess_candidates_ws_bytes(n_images, width, height);
}

int gms_chess_candidates_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, int max_candidates, void* d_ws,
                                size_t ws_bytes, gms_chess_candidate* d_out, int32_t* d_counts)
{
    if (!c || !calib::batch_ok(n_images, width, height, max_candidates) || !d_images || !d_ws || !d_out || !d_counts) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::chess_candidates_ws_bytes(n_images, width, height)) || misaligned(d_out, 4) || misaligned(d_counts, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_chess_candidates(d_images, n_images, width, height, max_candidates, d_ws, d_out, d_counts, c->stream); });
}

int gms_corner_subpix_device(gms_ctx* c, const uint8_t* d_images, int n_images, int width, int height, const int32_t* d_image_of,
                             double* d_corners, int n_corners, int win, int max_iter, double eps, int32_t* d_status)
{
    if (!c || n_images < 1 || n_images > 65535 || n_corners < 0 || !calib::subpix_args_ok(width, height, win, max_iter, eps)) return GMS_ERR_BAD_ARG;
    if (n_corners == 0) return GMS_OK;
    if (!d_images || !d_corners || misaligned(d_corners, 8) || misaligned(d_image_of, 4) || misaligned(d_status, 4)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_corner_subpix(d_images, n_images, width, height, d_image_of, d_corners, n_corners, max_iter, eps, d_status, c->stream);
    });
}

int gms_find_chessboard_corners(const uint8_t* image, int width, int height, int nx, int ny, int* found, float* corners)
{
    if (!image || !found || !corners || nx < 2 || ny < 2 || nx == ny || (long long)nx * ny > calib::kMaxCandidates ||
        !calib::batch_ok(1, width, height, nx * ny))
        return GMS_ERR_BAD_ARG;
    *found = 0;
    const int n = nx * ny;
    const size_t px = (size_t)width * (size_t)height;
    gms::BlockLayout lay;
    const size_t o_img = lay.add(px), o_ws = lay.add(gms::chess_candidates_ws_bytes(1, width, height)), o_out = lay.add((size_t)n * sizeof(gms_chess_candidate)),
                 o_cnt = lay.add(sizeof(int32_t));
    std::vector<gms_chess_candidate> cand((size_t)n);
    int32_t count = 0;
    DevBlock blk(lay, nullptr);
    blk.in(o_img, image, px);
    blk.run([&](hipStream_t st) {
        return gms::launch_chess_candidates(blk.at<uint8_t>(o_img), 1, width, height, n, blk.at(o_ws), blk.at<gms_chess_candidate>(o_out),
                                            blk.at<int32_t>(o_cnt), st);
    });
    blk.out(&count, o_cnt, sizeof(int32_t));
    blk.out(cand.data(), o_out, (size_t)n * sizeof(gms_chess_candidate));
    const int rc = blk.finish();
    if (rc != GMS_OK || count < n) return rc;
    std::vector<calib::P2> p((size_t)n), ordered;
    for (int i = 0; i < n; ++i) p[i] = {(double)cand[i].x, (double)cand[i].y};
    if (!calib::order_board(p, nx, ny, ordered)) return GMS_OK;
    for (int i = 0; i < n; ++i) {
        corners[2 * i] = (float)ordered[i].x;
        corners[2 * i + 1] = (float)ordered[i].y;
    }
    *found = 1;
    return GMS_OK;
}

int gms_order_chessboard(const double* points, int nx, int ny, int* found, double* ordered)
{
    if (!points || !found || !ordered || nx < 2 || ny < 2 || nx == ny || (long long)nx * ny > calib::kMaxCandidates) return GMS_ERR_BAD_ARG;
    const int n = nx * ny;
    std::vector<calib::P2> p((size_t)n), o;
    for (int i = 0; i < n; ++i) p[i] = {points[2 * i], points[2 * i + 1]};
    *found = calib::order_board(p, nx, ny, o) ? 1 : 0;
    if (*found)
        for (int i = 0; i < n; ++i) {
            ordered[2 * i] = o[i].x;
            ordered[2 * i + 1] = o[i].y;
        }
    return GMS_OK;
}

int gms_corner_subpix(const uint8_t* image, int width, int height, double* corners, int n_corners, int win, int max_iter, double eps,
                      int32_t* status)
{
    if (!image || n_corners < 0 || (n_corners > 0 && !corners) || !calib::subpix_args_ok(width, height, win, max_iter, eps)) return GMS_ERR_BAD_ARG;
    for (int i = 0; i < n_corners; ++i)
        if (!calib::subpix_window_ok(width, height, corners[2 * i], corners[2 * i + 1])) return GMS_ERR_BAD_ARG;
    if (n_corners == 0) return GMS_OK;
    const size_t px = (size_t)width * (size_t)height, cb = (size_t)n_corners * 2 * sizeof(double), sb = (size_t)n_corners * sizeof(int32_t);
    gms::BlockLayout lay;
    const size_t o_img = lay.add(px), o_c = lay.add(cb), o_s = lay.add(sb);
    DevBlock blk(lay, nullptr);
    blk.in(o_img, image, px);
    blk.in(o_c, corners, cb);
    blk.run([&](hipStream_t st) {
        return gms::launch_corner_subpix(blk.at<uint8_t>(o_img), 1, width, height, nullptr, blk.at<double>(o_c), n_corners, max_iter, eps,
                                         blk.at<int32_t>(o_s), st);
    });
    blk.out(corners, o_c, cb);
    if (status) blk.out(status, o_s, sb);
    return blk.finish();
}

int gms_calibrate_camera(const double* object_points, const double* image_points, const int32_t* counts, int n_views, int width, int height,
                         double* K, double* dist, double* rvecs, double* tvecs, double* rms)
{
    if (!object_points || !image_points || !counts || n_views < 1 || n_views > 4096 || width < 1 || height < 1 || !K || !dist || !rvecs ||
        !tvecs || !rms)
        return GMS_ERR_BAD_ARG;
    std::vector<int> off(1, 0);
    for (int v = 0; v < n_views; ++v) {
        if (counts[v] < 4 || counts[v] > (1 << 20)) return GMS_ERR_BAD_ARG;
        off.push_back(off.back() + counts[v]);
    }
    const size_t total = (size_t)off.back();
    std::vector<calib::P3> obj(total);
    std::vector<calib::P2> img(total);
    for (size_t i = 0; i < total; ++i) {
        obj[i] = {object_points[3 * i], object_points[3 * i + 1], object_points[3 * i + 2]};
        img[i] = {image_points[2 * i], image_points[2 * i + 1]};
    }
    calib::Calibration cal;
    if (!calib::calibrate_camera(obj, img, off, width, height, cal)) return GMS_ERR_DOMAIN;
    std::copy(cal.K, cal.K + 9, K);
    std::copy(cal.dist, cal.dist + 5, dist);
    std::copy(cal.rvecs.begin(), cal.rvecs.end(), rvecs);
    std::copy(cal.tvecs.begin(), cal.tvecs.end(), tvecs);
    *rms = cal.rms;
    return GMS_OK;
}

}  // extern "C"
