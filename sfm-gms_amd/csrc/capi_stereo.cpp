// capi_stereo.cpp -- the C ABI of the disparity matchers (StereoBM, semi-global matching) and of the speckle filter behind them.
#include "capi_common.h"
#include "gms_kernels.h"
#include "speckle_core.h"
#include "stereo_bm_core.h"
#include "stereo_sgm_core.h"

extern "C" {

// ---- StereoBM (stereo_bm_kernels.hip) ----------------------------------------------------------------------------
GMS_PARAMS_OR(sbm_params, gms_stereo_bm_params, GMS_STEREO_BM_PARAMS_REFERENCE)

size_t gms_stereo_bm_workspace_bytes(int width, int height, int n_pairs, const gms_stereo_bm_params* params)
{
    if (n_pairs < 0 || n_pairs > 65535 || !sbm::params_ok(sbm_params(params), width, height)) return 0;
    return gms::stereo_bm_ws_bytes(n_pairs, width, height);
}

int gms_stereo_bm_device(gms_ctx* c, const gms_stereo_bm_params* params, const uint8_t* d_left, const uint8_t* d_right, int n_pairs,
                         int width, int height, int pitch, void* d_ws, size_t ws_bytes, int16_t* d_disp16, int32_t* d_cost)
{
    const gms_stereo_bm_params& p = sbm_params(params);
    if (!c || n_pairs < 0 || n_pairs > 65535 || !sbm::params_ok(p, width, height) || pitch < width) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_left || !d_right || !d_ws || !d_disp16) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::stereo_bm_ws_bytes(n_pairs, width, height)) || misaligned(d_disp16, 2) || misaligned(d_cost, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_stereo_bm(p, d_left, d_right, n_pairs, width, height, pitch, d_ws, d_disp16, d_cost, c->stream); });
}

int gms_stereo_bm_normalize_device(gms_ctx* c, const int16_t* d_disp16, int n, int width, int height, uint8_t* d_out8)
{
    if (!c || n < 0 || width <= 0 || height <= 0) return GMS_ERR_BAD_ARG;
    if (n == 0) return GMS_OK;
    if (!d_disp16 || !d_out8 || misaligned(d_disp16, 2)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_stereo_bm_normalize(d_disp16, n, width, height, d_out8, c->stream); });
}

int gms_stereo_bm(const gms_stereo_bm_params* params, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                  int16_t* disp16, int32_t* cost, uint8_t* disp8)
{
    const gms_stereo_bm_params& p = sbm_params(params);
    if (!sbm::params_ok(p, width, height) || pitch < width || !left || !right) return GMS_ERR_BAD_ARG;
    const size_t px = (size_t)width * (size_t)height, img = (size_t)pitch * (size_t)(height - 1) + (size_t)width;
    gms::BlockLayout lay;  // the images keep the caller's pitch
    const size_t o_l = lay.add(img), o_r = lay.add(img), o_ws = lay.add(gms::stereo_bm_ws_bytes(1, width, height));
    const size_t o_d = lay.add(2 * px), o_c = lay.add(4 * px), o_8 = lay.add(px);
    DevBlock blk(lay, nullptr);
    blk.in(o_l, left, img);
    blk.in(o_r, right, img);
    blk.run([&](hipStream_t st) {
        return gms::launch_stereo_bm(p, blk.at<uint8_t>(o_l), blk.at<uint8_t>(o_r), 1, width, height, pitch, blk.at(o_ws), blk.at<int16_t>(o_d),
                                     cost ? blk.at<int32_t>(o_c) : nullptr, st);
    });
    if (disp8) blk.run([&](hipStream_t st) { return gms::launch_stereo_bm_normalize(blk.at<int16_t>(o_d), 1, width, height, blk.at<uint8_t>(o_8), st); });
    if (disp16) blk.out(disp16, o_d, 2 * px);
    if (cost) blk.out(cost, o_c, 4 * px);
    if (disp8) blk.out(disp8, o_8, px);
    return blk.finish();
}

// ---- semi-global matching (stereo_sgm_kernels.hip) ------------------------------------------------------------------
GMS_PARAMS_OR(sgm_params, gms_stereo_sgm_params, GMS_STEREO_SGM_PARAMS_REFERENCE)

size_t gms_stereo_sgm_workspace_bytes(int width, int height, int n_pairs, const gms_stereo_sgm_params* params)
{
    if (n_pairs < 0 || n_pairs > 65535 || !sgm::params_ok(sgm_params(params), width, height)) return 0;
    return gms::stereo_sgm_ws_bytes(sgm_params(params), n_pairs, width, height);
}

int gms_stereo_sgm_device(gms_ctx* c, const gms_stereo_sgm_params* params, const uint8_t* d_left, const uint8_t* d_right, int n_pairs,
                          int width, int height, int pitch, void* d_ws, size_t ws_bytes, int16_t* d_disp16, int32_t* d_cost)
{
    const gms_stereo_sgm_params& p = sgm_params(params);
    if (!c || n_pairs < 0 || n_pairs > 65535 || !sgm::params_ok(p, width, height) || pitch < width) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_left || !d_right || !d_ws || !d_disp16) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::stereo_sgm_ws_bytes(p, n_pairs, width, height)) || misaligned(d_disp16, 2) || misaligned(d_cost, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_stereo_sgm(p, d_left, d_right, n_pairs, width, height, pitch, d_ws, d_disp16, d_cost, c->stream); });
}

int gms_stereo_sgm(const gms_stereo_sgm_params* params, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                   int16_t* disp16, int32_t* cost, uint8_t* disp8)
{
    const gms_stereo_sgm_params& p = sgm_params(params);
    if (!sgm::params_ok(p, width, height) || pitch < width || !left || !right) return GMS_ERR_BAD_ARG;
    const size_t ws = gms::stereo_sgm_ws_bytes(p, 1, width, height);
    if (ws == 0) return GMS_ERR_BAD_ARG;
    const size_t px = (size_t)width * (size_t)height, img = (size_t)pitch * (size_t)(height - 1) + (size_t)width;
    gms::BlockLayout lay;  // the images keep the caller's pitch
    const size_t o_l = lay.add(img), o_r = lay.add(img), o_ws = lay.add(ws);
    const size_t o_d = lay.add(2 * px), o_c = lay.add(4 * px), o_8 = lay.add(px);
    DevBlock blk(lay, nullptr);
    blk.in(o_l, left, img);
    blk.in(o_r, right, img);
    blk.run([&](hipStream_t st) {
        return gms::launch_stereo_sgm(p, blk.at<uint8_t>(o_l), blk.at<uint8_t>(o_r), 1, width, height, pitch, blk.at(o_ws), blk.at<int16_t>(o_d),
                                      cost ? blk.at<int32_t>(o_c) : nullptr, st);
    });
    if (disp8) blk.run([&](hipStream_t st) { return gms::launch_stereo_bm_normalize(blk.at<int16_t>(o_d), 1, width, height, blk.at<uint8_t>(o_8), st); });
    if (disp16) blk.out(disp16, o_d, 2 * px);
    if (cost) blk.out(cost, o_c, 4 * px);
    if (disp8) blk.out(disp8, o_8, px);
    return blk.finish();
}

// ---- the speckle filter (speckle_kernels.hip, speckle_core.h) ------------------------------------------------------
size_t gms_filter_speckles_workspace_bytes(int width, int height, int n)
{
    if (!spk::args_ok(width, height, n, 0, 0, 0)) return 0;
    return gms::speckle_ws_bytes(n, width, height);
}

int gms_filter_speckles_device(gms_ctx* c, int16_t* d_disp16, int n, int width, int height, int new_val, int max_speckle_size, int max_diff,
                               void* d_ws, size_t ws_bytes, int32_t* d_removed)
{
    if (!c || !spk::args_ok(width, height, n, new_val, max_speckle_size, max_diff) || !d_disp16 || !d_ws) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::speckle_ws_bytes(n, width, height)) || misaligned(d_disp16, 2) || misaligned(d_removed, 4))
        return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_filter_speckles(d_disp16, n, width, height, new_val, max_speckle_size, max_diff, d_ws, d_removed, c->stream);
    });
}

int gms_filter_speckles(int16_t* disp16, int width, int height, int new_val, int max_speckle_size, int max_diff, int32_t* removed)
{
    if (!spk::args_ok(width, height, 1, new_val, max_speckle_size, max_diff) || !disp16) return GMS_ERR_BAD_ARG;
    const size_t bytes = 2 * (size_t)width * (size_t)height;
    gms::BlockLayout lay;
    const size_t o_d = lay.add(bytes), o_ws = lay.add(gms::speckle_ws_bytes(1, width, height)), o_rm = lay.add(4);
    DevBlock blk(lay, nullptr);
    blk.in(o_d, disp16, bytes);
    blk.run([&](hipStream_t st) {
        return gms::launch_filter_speckles(blk.at<int16_t>(o_d), 1, width, height, new_val, max_speckle_size, max_diff, blk.at(o_ws),
                                           blk.at<int32_t>(o_rm), st);
    });
    blk.out(disp16, o_d, bytes);
    if (removed) blk.out(removed, o_rm, 4);
    return blk.finish();
}

}  // extern "C"
