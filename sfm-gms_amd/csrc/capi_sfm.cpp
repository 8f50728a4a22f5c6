// capi_sfm.cpp -- the C ABI of the many-view stage: the registration plan, registering the views into one frame, one-to-one matches
// for its tracks, bundle adjustment, and pair records from a view array.
#include <vector>

#include "capi_common.h"
#include "gms_kernels.h"
#include "sfm_ba_core.h"
#include "sfm_pair_pose_core.h"
#include "sfm_register_core.h"

extern "C" {

// ---- many views into one frame (sfm_register_kernels.hip; the plan and the arithmetic are sfm_register_core.h) ----------------------
int gms_sfm_plan(const gms_pair* pairs, int n_pairs, int n_frames, int root, gms_sfm_plan_entry* plan)
{
    if (n_pairs < 0 || n_frames < 1 || (n_pairs > 0 && (!pairs || !plan))) return GMS_ERR_BAD_ARG;
    std::vector<int32_t> reg_by((size_t)n_frames);
    return sfr::plan(pairs, n_pairs, n_frames, root, reg_by.data(), plan) ? GMS_OK : GMS_ERR_BAD_ARG;
}

static bool sfm_register_sizes_ok(int n_frames, int n_pairs, int64_t total_kp, int64_t total_matches)
{
    return n_frames >= 1 && n_pairs >= 0 && total_kp >= 0 && total_kp < INT32_MAX && total_matches >= 0 && total_matches < ((int64_t)1 << 40);
}

size_t gms_sfm_register_workspace_bytes(int n_frames, int n_pairs, int64_t total_kp, int64_t total_matches)
{
    if (!sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_matches)) return 0;
    return gms::sfm_register_ws_bytes(n_pairs, total_kp, total_matches);
}

int gms_sfm_register_keep_device(gms_ctx* c, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                            const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_matches, const gms_dmatch* d_filtered,
                            const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links, void* d_ws,
                            size_t ws_bytes, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_points_world, int32_t* d_track,
                            int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs, int32_t* d_cloud_est,
                            double* d_cloud_spread, gms_sfm_summary* d_summary, const uint8_t* d_keep)
{
    if (!c || !sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_matches) || max_m < 0 || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (root < 0 || root >= n_frames || min_links < 1 || cloud_cap < 0) return GMS_ERR_BAD_ARG;
    if (!d_frame_off || !d_ws || !d_views || !d_summary) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!d_pairs || !d_plan || !d_tv || !d_reg)) return GMS_ERR_BAD_ARG;
    if (total_matches > 0 && (!d_filtered || !d_mask || !d_points3d || !d_points_world || !d_track)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!d_cloud || !d_cloud_id || !d_cloud_obs || !d_cloud_est || !d_cloud_spread)) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::sfm_register_ws_bytes(n_pairs, total_kp, total_matches))) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_sfm_register(d_frame_off, n_frames, total_kp, d_pairs, d_plan, n_pairs, max_m, total_matches, d_filtered, d_mask,
                                        d_points3d, d_tv, root, min_links, d_ws, d_views, d_reg, d_points_world, d_track, cloud_cap, d_cloud,
                                        d_cloud_id, d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary, c->stream, d_keep);
    });
}

int gms_sfm_register_keep(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const double* points3d, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                     gms_sfm_pair_reg* reg, double* points_world, int32_t* track, int64_t cloud_cap, double* cloud, int32_t* cloud_id,
                     int32_t* cloud_obs, int32_t* cloud_est, double* cloud_spread, gms_sfm_summary* summary, const uint8_t* keep)
{
    if (n_frames < 1 || n_pairs < 0 || !frame_off || !views || !summary || root < 0 || root >= n_frames || min_links < 1 || cloud_cap < 0)
        return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!pairs || !tv || !reg)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!cloud || !cloud_id || !cloud_obs || !cloud_est || !cloud_spread)) return GMS_ERR_BAD_ARG;
    if (!frame_offsets_ok(frame_off, n_frames)) return GMS_ERR_BAD_ARG;
    std::vector<gms_sfm_plan_entry> plan((size_t)n_pairs);
    GMS_TRY(gms_sfm_plan(pairs, n_pairs, n_frames, root, plan.data()));
    const PairRanges ranges = pair_ranges(pairs, n_pairs, n_frames, false);
    if (!ranges.ok) return GMS_ERR_BAD_ARG;
    const int64_t total_m = ranges.total_m;
    const int max_m = ranges.max_m;
    const int64_t total_kp = frame_off[n_frames];
    if (!sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_m) || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (total_m > 0 && (!filtered || !mask || !points3d || !points_world || !track)) return GMS_ERR_BAD_ARG;
    const size_t M = (size_t)total_m, P = (size_t)n_pairs, Cc = (size_t)cloud_cap;
    gms::BlockLayout lay;
    const size_t o_off = lay.add(8 * ((size_t)n_frames + 1)), o_pairs = lay.add(sizeof(gms_pair) * P), o_plan = lay.add(sizeof(gms_sfm_plan_entry) * P);
    const size_t o_m = lay.add(sizeof(gms_dmatch) * M), o_mask = lay.add(M), o_pts = lay.add(24 * M), o_tv = lay.add(sizeof(gms_two_view) * P);
    const size_t o_ws = lay.add(gms::sfm_register_ws_bytes(n_pairs, total_kp, total_m)), o_keep = lay.add(keep ? M : 0);
    // the outputs, back to back: cleared as one span
    const size_t o_views = lay.add(sizeof(gms_sfm_view) * (size_t)n_frames), o_reg = lay.add(sizeof(gms_sfm_pair_reg) * P), o_world = lay.add(24 * M);
    const size_t o_track = lay.add(4 * M), o_cloud = lay.add(24 * Cc), o_id = lay.add(4 * Cc), o_obs = lay.add(4 * Cc), o_est = lay.add(4 * Cc);
    const size_t o_spread = lay.add(8 * Cc), o_sum = lay.add(sizeof(gms_sfm_summary));
    DevBlock blk(lay, nullptr);
    blk.in(o_off, frame_off, 8 * ((size_t)n_frames + 1));
    if (P) {
        blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
        blk.in(o_plan, plan.data(), sizeof(gms_sfm_plan_entry) * P);
        blk.in(o_tv, tv, sizeof(gms_two_view) * P);
    }
    if (M) {
        blk.in(o_m, filtered, sizeof(gms_dmatch) * M);
        blk.in(o_mask, mask, M);
        blk.in(o_pts, points3d, 24 * M);
        if (keep) blk.in(o_keep, keep, M);
    }
    blk.run([&](hipStream_t st) { return hipMemsetAsync(blk.at(o_views), 0, lay.total() - o_views, st); });
    blk.run([&](hipStream_t st) {
        return gms::launch_sfm_register(blk.at<int64_t>(o_off), n_frames, total_kp, blk.at<gms_pair>(o_pairs), blk.at<gms_sfm_plan_entry>(o_plan),
                                        n_pairs, max_m, total_m, blk.at<gms_dmatch>(o_m), blk.at<uint8_t>(o_mask), blk.at<double>(o_pts),
                                        blk.at<gms_two_view>(o_tv), root, min_links, blk.at(o_ws), blk.at<gms_sfm_view>(o_views),
                                        blk.at<gms_sfm_pair_reg>(o_reg), blk.at<double>(o_world), blk.at<int32_t>(o_track), cloud_cap,
                                        blk.at<double>(o_cloud), blk.at<int32_t>(o_id), blk.at<int32_t>(o_obs), blk.at<int32_t>(o_est),
                                        blk.at<double>(o_spread), blk.at<gms_sfm_summary>(o_sum), st, keep && M ? blk.at<uint8_t>(o_keep) : nullptr);
    });
    blk.out(views, o_views, sizeof(gms_sfm_view) * (size_t)n_frames);
    if (P) blk.out(reg, o_reg, sizeof(gms_sfm_pair_reg) * P);
    if (M) {
        blk.out(points_world, o_world, 24 * M);
        blk.out(track, o_track, 4 * M);
    }
    if (Cc) {
        blk.out(cloud, o_cloud, 24 * Cc);
        blk.out(cloud_id, o_id, 4 * Cc);
        blk.out(cloud_obs, o_obs, 4 * Cc);
        blk.out(cloud_est, o_est, 4 * Cc);
        blk.out(cloud_spread, o_spread, 8 * Cc);
    }
    blk.out(summary, o_sum, sizeof(gms_sfm_summary));
    return blk.finish();
}

// the calls without a keep plane: the same launches with a null plane
int gms_sfm_register_device(gms_ctx* c, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                            const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_matches, const gms_dmatch* d_filtered,
                            const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links, void* d_ws,
                            size_t ws_bytes, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_points_world, int32_t* d_track,
                            int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs, int32_t* d_cloud_est,
                            double* d_cloud_spread, gms_sfm_summary* d_summary)
{
    return gms_sfm_register_keep_device(c, d_frame_off, n_frames, total_kp, d_pairs, d_plan, n_pairs, max_m, total_matches, d_filtered, d_mask,
                                        d_points3d, d_tv, root, min_links, d_ws, ws_bytes, d_views, d_reg, d_points_world, d_track, cloud_cap,
                                        d_cloud, d_cloud_id, d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary, nullptr);
}

int gms_sfm_register(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const double* points3d, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                     gms_sfm_pair_reg* reg, double* points_world, int32_t* track, int64_t cloud_cap, double* cloud, int32_t* cloud_id,
                     int32_t* cloud_obs, int32_t* cloud_est, double* cloud_spread, gms_sfm_summary* summary)
{
    return gms_sfm_register_keep(frame_off, n_frames, pairs, n_pairs, filtered, mask, points3d, tv, root, min_links, views, reg, points_world,
                                 track, cloud_cap, cloud, cloud_id, cloud_obs, cloud_est, cloud_spread, summary, nullptr);
}

// ---- one-to-one matches per pair (match_unique_kernels.hip; the rule is match_unique_core.h) ----------------------------------------
size_t gms_match_unique_workspace_bytes(int n_pairs, int64_t total_kp, int64_t total_matches)
{
    if (!sfm_register_sizes_ok(1, n_pairs, total_kp, total_matches)) return 0;
    return gms::match_unique_ws_bytes(total_matches);
}

int gms_match_unique_device(gms_ctx* c, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs,
                            int max_m, int64_t total_matches, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_two_view* d_tv,
                            void* d_ws, size_t ws_bytes, uint8_t* d_keep, int32_t* d_counts)
{
    if (!c || !sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_matches) || max_m < 0 || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (!d_frame_off || !d_ws) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!d_pairs || !d_counts)) return GMS_ERR_BAD_ARG;
    if (total_matches > 0 && (!d_filtered || !d_keep)) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::match_unique_ws_bytes(total_matches))) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_match_unique(d_frame_off, n_frames, total_kp, d_pairs, n_pairs, max_m, total_matches, d_filtered, d_mask, d_tv, d_ws,
                                        d_keep, d_counts, c->stream);
    });
}

int gms_match_unique(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const gms_two_view* tv, uint8_t* keep, int32_t* counts)
{
    if (n_frames < 1 || n_pairs < 0 || !frame_off) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!pairs || !counts)) return GMS_ERR_BAD_ARG;
    if (!frame_offsets_ok(frame_off, n_frames)) return GMS_ERR_BAD_ARG;
    const PairRanges ranges = pair_ranges(pairs, n_pairs, n_frames, true);
    if (!ranges.ok) return GMS_ERR_BAD_ARG;
    const int64_t total_m = ranges.total_m;
    const int max_m = ranges.max_m;
    const int64_t total_kp = frame_off[n_frames];
    if (!sfm_register_sizes_ok(n_frames, n_pairs, total_kp, total_m) || max_m >= (1 << 24)) return GMS_ERR_BAD_ARG;
    if (total_m > 0 && (!filtered || !keep)) return GMS_ERR_BAD_ARG;
    const size_t M = (size_t)total_m, P = (size_t)n_pairs;
    gms::BlockLayout lay;
    const size_t o_off = lay.add(8 * ((size_t)n_frames + 1)), o_pairs = lay.add(sizeof(gms_pair) * P), o_m = lay.add(sizeof(gms_dmatch) * M);
    const size_t o_mask = lay.add(mask ? M : 0), o_tv = lay.add(tv ? sizeof(gms_two_view) * P : 0), o_ws = lay.add(gms::match_unique_ws_bytes(total_m));
    const size_t o_keep = lay.add(M), o_counts = lay.add(8 * P);  // the outputs, back to back: cleared as one span
    DevBlock blk(lay, nullptr);
    blk.in(o_off, frame_off, 8 * ((size_t)n_frames + 1));
    if (P) {
        blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
        if (tv) blk.in(o_tv, tv, sizeof(gms_two_view) * P);
    }
    if (M) {
        blk.in(o_m, filtered, sizeof(gms_dmatch) * M);
        if (mask) blk.in(o_mask, mask, M);
    }
    if (lay.total() > o_keep) blk.run([&](hipStream_t st) { return hipMemsetAsync(blk.at(o_keep), 0, lay.total() - o_keep, st); });
    blk.run([&](hipStream_t st) {
        return gms::launch_match_unique(blk.at<int64_t>(o_off), n_frames, total_kp, blk.at<gms_pair>(o_pairs), n_pairs, max_m, total_m,
                                        blk.at<gms_dmatch>(o_m), mask && M ? blk.at<uint8_t>(o_mask) : nullptr,
                                        tv && P ? blk.at<gms_two_view>(o_tv) : nullptr, blk.at(o_ws), blk.at<uint8_t>(o_keep),
                                        blk.at<int32_t>(o_counts), st);
    });
    if (M) blk.out(keep, o_keep, M);
    if (P) blk.out(counts, o_counts, 8 * P);
    return blk.finish();
}

// ---- bundle adjustment behind the registration (sfm_ba_kernels.hip; the arithmetic is sfm_ba_core.h) --------------------------------
static bool sfm_ba_sizes_ok(int n_frames, int n_pairs, int64_t total_kp, int64_t cloud_cap)
{
    return n_frames >= 1 && n_frames <= (1 << 24) && n_pairs >= 0 && total_kp >= 0 && total_kp < INT32_MAX && cloud_cap >= 0 && cloud_cap < INT32_MAX;
}

size_t gms_sfm_ba_workspace_bytes(int n_frames, int n_pairs, int64_t total_kp, int64_t cloud_cap)
{
    if (!sfm_ba_sizes_ok(n_frames, n_pairs, total_kp, cloud_cap)) return 0;
    return gms::sfm_ba_ws_bytes(n_frames, total_kp, cloud_cap);
}

int gms_sfm_ba_device(gms_ctx* c, const gms_camera* camera, const gms_sfm_ba_params* params, const gms_keypoint* d_kp,
                      const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs,
                      int64_t total_matches, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_sfm_view* d_views,
                      const gms_sfm_pair_reg* d_reg, const int32_t* d_track, int64_t cloud_cap, const double* d_cloud,
                      const int32_t* d_cloud_id, const gms_sfm_summary* d_reg_summary, void* d_ws, size_t ws_bytes,
                      gms_sfm_view* d_views_out, double* d_cloud_out, int32_t* d_track_status, gms_sfm_ba_summary* d_summary)
{
    if (!c || !camera || !params || !sfm_ba_sizes_ok(n_frames, n_pairs, total_kp, cloud_cap) || !sba::params_ok(*params)) return GMS_ERR_BAD_ARG;
    if (total_matches < 0 || total_matches >= ((int64_t)1 << 40)) return GMS_ERR_BAD_ARG;
    if (!d_frame_off || !d_views || !d_reg_summary || !d_ws || !d_views_out || !d_summary) return GMS_ERR_BAD_ARG;
    if (total_kp > 0 && !d_kp) return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!d_pairs || !d_reg)) return GMS_ERR_BAD_ARG;
    if (total_matches > 0 && (!d_filtered || !d_mask || !d_track)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!d_cloud || !d_cloud_id || !d_cloud_out || !d_track_status)) return GMS_ERR_BAD_ARG;
    if (!ws_ok(d_ws, ws_bytes, gms::sfm_ba_ws_bytes(n_frames, total_kp, cloud_cap))) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] {
        return gms::launch_sfm_ba(*camera, *params, d_kp, d_frame_off, n_frames, total_kp, d_pairs, n_pairs, total_matches, d_filtered, d_mask,
                                  d_views, d_reg, d_track, cloud_cap, d_cloud, d_cloud_id, d_reg_summary, d_ws, d_views_out, d_cloud_out,
                                  d_track_status, d_summary, c->stream);
    });
}

int gms_sfm_ba(const gms_camera* camera, const gms_sfm_ba_params* params, const gms_keypoint* kp, const int64_t* frame_off, int n_frames,
               const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered, const uint8_t* mask, const gms_sfm_view* views,
               const gms_sfm_pair_reg* reg, const int32_t* track, int64_t cloud_cap, const double* cloud, const int32_t* cloud_id,
               int64_t n_tracks, gms_sfm_view* views_out, double* cloud_out, int32_t* track_status, gms_sfm_ba_summary* summary)
{
    if (!camera || !params || n_frames < 1 || n_pairs < 0 || !frame_off || !views || !views_out || !summary || cloud_cap < 0 || n_tracks < 0 ||
        !sba::params_ok(*params))
        return GMS_ERR_BAD_ARG;
    if (n_pairs > 0 && (!pairs || !reg)) return GMS_ERR_BAD_ARG;
    if (cloud_cap > 0 && (!cloud || !cloud_id || !cloud_out || !track_status)) return GMS_ERR_BAD_ARG;
    if (!frame_offsets_ok(frame_off, n_frames)) return GMS_ERR_BAD_ARG;
    const PairRanges ranges = pair_ranges(pairs, n_pairs, n_frames, false);
    if (!ranges.ok) return GMS_ERR_BAD_ARG;
    const int64_t total_m = ranges.total_m;
    const int64_t total_kp = frame_off[n_frames];
    if (!sfm_ba_sizes_ok(n_frames, n_pairs, total_kp, cloud_cap) || total_m >= ((int64_t)1 << 40)) return GMS_ERR_BAD_ARG;
    if (total_kp > 0 && !kp) return GMS_ERR_BAD_ARG;
    if (total_m > 0 && (!filtered || !mask || !track)) return GMS_ERR_BAD_ARG;
    const size_t M = (size_t)total_m, P = (size_t)n_pairs, Cc = (size_t)cloud_cap, K = (size_t)total_kp, F = (size_t)n_frames;
    gms_sfm_summary rs = {};
    rs.n_tracks = n_tracks;
    gms::BlockLayout lay;
    const size_t o_kp = lay.add(sizeof(gms_keypoint) * K), o_off = lay.add(8 * (F + 1)), o_pairs = lay.add(sizeof(gms_pair) * P);
    const size_t o_m = lay.add(sizeof(gms_dmatch) * M), o_mask = lay.add(M), o_views = lay.add(sizeof(gms_sfm_view) * F);
    const size_t o_reg = lay.add(sizeof(gms_sfm_pair_reg) * P), o_track = lay.add(4 * M), o_cloud = lay.add(24 * Cc), o_id = lay.add(4 * Cc);
    const size_t o_rs = lay.add(sizeof(gms_sfm_summary)), o_ws = lay.add(gms::sfm_ba_ws_bytes(n_frames, total_kp, cloud_cap));
    const size_t o_vout = lay.add(sizeof(gms_sfm_view) * F), o_cout = lay.add(24 * Cc), o_st = lay.add(4 * Cc), o_sum = lay.add(sizeof(gms_sfm_ba_summary));
    DevBlock blk(lay, nullptr);
    blk.in(o_off, frame_off, 8 * (F + 1));
    blk.in(o_views, views, sizeof(gms_sfm_view) * F);
    blk.in(o_rs, &rs, sizeof(rs));
    if (K) blk.in(o_kp, kp, sizeof(gms_keypoint) * K);
    if (P) {
        blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
        blk.in(o_reg, reg, sizeof(gms_sfm_pair_reg) * P);
    }
    if (M) {
        blk.in(o_m, filtered, sizeof(gms_dmatch) * M);
        blk.in(o_mask, mask, M);
        blk.in(o_track, track, 4 * M);
    }
    if (Cc) {
        blk.in(o_cloud, cloud, 24 * Cc);
        blk.in(o_id, cloud_id, 4 * Cc);
    }
    blk.run([&](hipStream_t st) {
        return gms::launch_sfm_ba(*camera, *params, blk.at<gms_keypoint>(o_kp), blk.at<int64_t>(o_off), n_frames, total_kp,
                                  blk.at<gms_pair>(o_pairs), n_pairs, total_m, blk.at<gms_dmatch>(o_m), blk.at<uint8_t>(o_mask),
                                  blk.at<gms_sfm_view>(o_views), blk.at<gms_sfm_pair_reg>(o_reg), blk.at<int32_t>(o_track), cloud_cap,
                                  blk.at<double>(o_cloud), blk.at<int32_t>(o_id), blk.at<gms_sfm_summary>(o_rs), blk.at(o_ws),
                                  blk.at<gms_sfm_view>(o_vout), blk.at<double>(o_cout), blk.at<int32_t>(o_st), blk.at<gms_sfm_ba_summary>(o_sum), st);
    });
    blk.out(views_out, o_vout, sizeof(gms_sfm_view) * F);
    if (Cc) {
        blk.out(cloud_out, o_cout, 24 * Cc);
        blk.out(track_status, o_st, 4 * Cc);
    }
    blk.out(summary, o_sum, sizeof(gms_sfm_ba_summary));
    return blk.finish();
}

// ---- pair records from a view array (sfm_pair_pose_kernels.hip; the arithmetic is sfm_pair_pose_core.h) -------------
int gms_sfm_pair_poses_device(gms_ctx* c, const gms_sfm_view* d_views, int n_frames, const gms_pair* d_pairs, int n_pairs, gms_two_view* d_tv_out,
                              gms_sfm_pair_reg* d_reg_out)
{
    if (!c || !ppose::call_args_ok(n_frames, n_pairs)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!d_views || !d_pairs || !d_tv_out || !d_reg_out) return GMS_ERR_BAD_ARG;
    if (misaligned(d_views, 8) || misaligned(d_pairs, 8) || misaligned(d_tv_out, 8) || misaligned(d_reg_out, 8)) return GMS_ERR_BAD_ARG;
    return on_ctx(c, [&] { return gms::launch_sfm_pair_poses(d_views, n_frames, d_pairs, n_pairs, d_tv_out, d_reg_out, c->stream); });
}

int gms_sfm_pair_poses(const gms_sfm_view* views, int n_frames, const gms_pair* pairs, int n_pairs, gms_two_view* tv_out, gms_sfm_pair_reg* reg_out)
{
    if (!ppose::call_args_ok(n_frames, n_pairs)) return GMS_ERR_BAD_ARG;
    if (n_pairs == 0) return GMS_OK;
    if (!views || !pairs || !tv_out || !reg_out) return GMS_ERR_BAD_ARG;
    const size_t F = (size_t)n_frames, P = (size_t)n_pairs;
    gms::BlockLayout lay;
    const size_t o_views = lay.add(sizeof(gms_sfm_view) * F), o_pairs = lay.add(sizeof(gms_pair) * P), o_tv = lay.add(sizeof(gms_two_view) * P),
                 o_reg = lay.add(sizeof(gms_sfm_pair_reg) * P);
    DevBlock blk(lay, nullptr);
    blk.in(o_views, views, sizeof(gms_sfm_view) * F);
    blk.in(o_pairs, pairs, sizeof(gms_pair) * P);
    blk.run([&](hipStream_t st) {
        return gms::launch_sfm_pair_poses(blk.at<gms_sfm_view>(o_views), n_frames, blk.at<gms_pair>(o_pairs), n_pairs, blk.at<gms_two_view>(o_tv),
                                          blk.at<gms_sfm_pair_reg>(o_reg), st);
    });
    blk.out(tv_out, o_tv, sizeof(gms_two_view) * P);
    blk.out(reg_out, o_reg, sizeof(gms_sfm_pair_reg) * P);
    return blk.finish();
}

}  // extern "C"
