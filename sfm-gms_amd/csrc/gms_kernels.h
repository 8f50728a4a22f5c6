// gms_kernels.h -- internal interface between the C-ABI host code and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gms.h"
#include "logos_dict_core.h"
#include "ws_layout.h"

namespace gms {

constexpr int kThreads = 1024;                         // one 16-wave workgroup per image pair
constexpr size_t kLdsBytes = 160 * 1024;               // gfx950 LDS per CU (and per workgroup)
// record handed from filter_kernel_dense_scales to filter_kernel: state, best count, best scale, best rotation, then one
// inlier bit per match of the best hypothesis so far (16 x 1024 matches at most)
constexpr uint32_t kPartialHeaderDw = 4;
constexpr uint32_t kPartialStrideDw = kPartialHeaderDw + 16 * 1024 / 32;

// The frame table (gms_frame_table_bytes) starts with a 16-byte header -- magic, then the number of keypoints it was built
// for -- so that the kernels find the code arrays behind the points by themselves, whatever n_frames / frame_off a filter call
// passes (a prefix or a subset of the table's frames is fine). A block without the header is filtered from its points alone.
constexpr uint32_t kTableMagic0 = 0x46534D47u, kTableMagic1 = 0x31424154u;  // "GMSF" "TAB1"
constexpr int kTableHeaderBytes = 16;

// Per-frame side records: what the byte-matrix kernel's identity-query path (dense_pair_plain<..., IDENT>) needs of frame A and
// what does not depend on the pair -- the half-cell histogram of ALL the frame's keypoints and two flags. They live in a buffer
// of the CONTEXT that built the table (side_records_kernel behind normalize_kernel), not in the table: its public size and
// layout stay what they were. Table and records are tied by a stamp: a 64-bit digest of what the records were built from (every
// frame's left codes, offset and count: table_stamp_kernel), never 0, which the build writes into the table's 16 spare bytes behind
// the code arrays (which no kernel interprets) and into every record. Equal tables carry equal bytes whoever built them; a table
// rebuilt from other keypoints -- by any context, at any address -- no longer matches the records of the build before. The kernel
// takes the identity path for a pair only when the two stamps agree and the record's (off, n) is the pair's frame A as this
// call's frame_off describes it.
struct SideRecord {
    int64_t off;              // the frame's first keypoint and ...
    int32_t n;                // ... number of keypoints when the records were built
    uint32_t flags;           // kSideBadLeft | kSideSpill
    uint64_t stamp;
    uint32_t pad[2];
    uint32_t hist[400];       // the half-cell histogram exactly as dense_pair_plain builds it in LDS: a dword per cell of grid type 1, a byte per half cell
};
static_assert(sizeof(SideRecord) == 1632 && sizeof(SideRecord) % 16 == 0, "side records are read in uint4s");
constexpr uint32_t kSideBadLeft = 1u;   // some left code is kLCellBad (a keypoint outside the parity domain)
constexpr uint32_t kSideSpill = 2u;     // some half cell holds more than 255 keypoints (a byte of hist has wrapped: hist is void)
constexpr size_t kSideMaxBytes = (size_t)64 << 20;  // a table of more frames than fit this gets no records (and no identity path)

struct FilterParams {
    const float2* pts;          // normalised keypoints of all frames (the table's points: kTableHeaderBytes behind its start)
    const int64_t* frame_off;   // n_frames + 1
    int n_frames;
    const gms_pair* pairs;
    int n_pairs;
    int stagger_ticks;          // first-round workgroups start spread over this many 100 MHz wall-clock ticks (0 = off)
    int stagger_blocks;         // how many leading workgroups count as the first round
    const gms_dmatch* matches;
    gms_dmatch* out;
    gms_pair_result* results;
    uint8_t* mask;              // optional
    uint32_t table_slots;       // multiple of 4: data + header buckets of all 400 regions
    int region_shift;           // region slots per match = 1 + 2^-shift
    int with_rotation, with_scale;
    uint32_t* partial;          // scale hypotheses: per-pair records of the byte-matrix kernel (scales 0..3), or null
    const uint32_t* pair_flags; // large-pair kernel only: when set, it filters just the pairs whose flag word has bit 1 set
    int dealt;                  // byte-matrix kernel: deal the matches to the lanes (inputs in spatial order; see dense_pair_rot in gms_kernel_dense.hip)
    int probe_scales;           // scale hypotheses: bit s set = bound scale s's inlier count first and skip the scale when it cannot win
    int probe_nibble;           // scale hypotheses: bit 3 / bit 4 = bound the 28 x 28 / 40 x 40 grid with four-bit entries first (half the bands of the byte probe)
    uint32_t* probe_stats;      // optional device counters: [0] scales probed, [1] scales the probe let skip
    uint32_t* overflow_events;  // streamed byte-matrix kernels: a word (pinned host memory) that counts the pairs they had to hand on because an entry left its byte
    int prefetch_type, prefetch_ahead;  // byte-matrix kernel: before grid type prefetch_type a workgroup touches the records of pair + prefetch_ahead (0 = off)
    int dense;                  // try the byte-matrix path first (no scale hypotheses only); the general path is the fallback
    int ident;                  // byte-matrix kernel, default flags: the identity-query instantiation (side != nullptr, side_frames >= 1, stamp != 0)
    int side_frames;            // records behind side
    const SideRecord* side;     // the context's per-frame side records, or nullptr
    uint64_t side_stamp;        // non-zero: the context's latest table build left side records (the stamp itself is on the device)
    uint32_t* ident_misses;     // a word (pinned host memory) that counts the pairs the identity instantiation had to filter with the generic body
    double threshold_factor;
    int right_w[5], right_h[5]; // setScale (DLL@0x180048c10): cvRound(20 * ratio[s])
#ifdef GMS_PHASE_TIMING
    unsigned long long* diag;   // diagnostic build only: [n_pairs][12] cycle sums
#endif
};

hipError_t init_filter_kernels();        // once per context, before the first launch: dynamic-LDS limits of every kernel
hipError_t init_band_kernels();
hipError_t init_big_kernels();
int        filter_pick_kpt(int max_m);   // matches per thread (template variant) for max_m, 0 = too large
uint32_t   filter_table_slots(int kpt);
int        filter_region_shift(int kpt);
size_t     filter_lds_bytes(int kpt, uint32_t table_slots);
// kp_stride_bytes: 28 = cv::KeyPoint records, 8 = packed (pt.x, pt.y) pairs
// d_side: n_frames side records to fill behind the table (stamp != 0), or nullptr (stamp 0: the table is marked as having none)
hipError_t launch_normalize(const void* d_kp, int kp_stride_bytes, const int64_t* d_frame_off, const int32_t* d_wh,
                            int n_frames, int64_t total_kp, float* d_pts, SideRecord* d_side, uint64_t stamp, hipStream_t stream);
hipError_t launch_filter(const FilterParams& p, int kpt, int n_pairs, hipStream_t stream);
// what launch_filter and init_filter_kernels dispatch to: the hashed kernel (gms_kernel_hash.hip), the byte-matrix kernel that
// falls back to it per pair (gms_kernel_dense.hip), and the limits of launch_filter_scales' first kernel (gms_kernel_scales.hip)
hipError_t launch_filter_hash(const FilterParams& p, int kpt, int n_pairs, size_t lds_bytes, hipStream_t stream);
hipError_t launch_filter_dense(const FilterParams& p, int kpt, int n_pairs, size_t lds_bytes, hipStream_t stream);
hipError_t init_hash_kernels();
hipError_t init_dense_kernels();
hipError_t init_scales_kernels();
hipError_t launch_order_probe(const FilterParams& p, uint32_t* flag, uint32_t* ident_flag, hipStream_t stream);  // *flag, *ident_flag: pinned host words
hipError_t launch_probe_verdict(uint32_t* stats, uint32_t* flag, hipStream_t stream);      // FilterParams::probe_stats -> pinned host word
// pair-table validation: ranges [match_off, match_off + m) must be disjoint; offenders get GMS_ERR_BAD_ARG in d_results (d_flag: a device word)
hipError_t launch_check_pairs(const gms_pair* d_pairs, int n_pairs, gms_pair_result* d_results, uint32_t* d_flag, hipStream_t stream);
hipError_t launch_filter_scales(const FilterParams& p, int kpt, int n_pairs, hipStream_t stream);
// gms_filter_host_batch: pair i's n_inliers survivors (at d_out + match_off) packed back to back into d_packed, the total into *d_total
hipError_t launch_compact_survivors(const gms_pair* d_pairs, const gms_pair_result* d_results, int n_pairs, const gms_dmatch* d_out,
                                    gms_dmatch* d_packed, int64_t* d_total, hipStream_t stream);
// large pairs (gms_kernel_big.hip): code words and table in a per-workgroup HBM slab
constexpr int kBigMaxMatches = 1 << 22;       // per pair: 4 194 304 (a 2594 x 1131 one-keypoint-per-pixel frame of DisparityUtil.cpp:299 has 2.93 M)
constexpr int kBigLdsMaskMatches = 262144;   // up to here the slab kernel keeps the winner's bit mask in LDS
int        big_mcap(int max_m);
size_t     big_ws_stride_dwords(int mcap);
hipError_t launch_filter_big(const FilterParams& p, int mcap, int n_workgroups, uint32_t* ws, hipStream_t stream);
// large pairs under the default flags (gms_kernel_band.hip): three-band 16-bit matrix in LDS; *flags_out marks the pairs
// left to launch_filter_big (bit 1)
size_t     band_ws_bytes_per_pair(int mcap, bool need_mask);
hipError_t launch_filter_band(const FilterParams& p, int mcap, void* ws, const uint32_t** flags_out, hipStream_t stream);
// large pairs with rotation / scale hypotheses (gms_kernel_band.hip): tiled 16-bit matrix, three launches per scale
size_t     tile_ws_bytes_per_pair(const FilterParams& p, int mcap, bool need_mask);
hipError_t launch_filter_tiles(const FilterParams& p, int mcap, void* ws, const uint32_t** flags_out, hipStream_t stream);
// pairs of 16 385 .. 65 536 matches, every flag combination (gms_kernel_stream.hip): the byte matrix with the matches streamed from a
// row-sorted workspace array, one workgroup per (pair, scale hypothesis); *flags_out marks the pairs left to launch_filter_big (bit 1)
hipError_t init_stream_kernels();
int        stream_max_matches();
size_t     stream_ws_bytes_per_pair(const FilterParams& p, int mcap, bool need_mask);
hipError_t launch_filter_stream(const FilterParams& p, int mcap, void* ws, const uint32_t** flags_out, hipStream_t stream);
// the same size class without scale hypotheses (gms_kernel_stream.hip; the default flags: gms_kernel_stream_plain.hip): one workgroup per pair, the byte matrix of gms_kernel_dense.hip with the code words streamed from an L2-resident array
size_t     stream_dense_ws_bytes_per_pair(int mcap);
hipError_t launch_filter_stream_dense(const FilterParams& p, int mcap, void* ws, const uint32_t** flags_out, hipStream_t stream);
// brute-force descriptor matcher (bf_kernels.hip)
size_t     bf_prepared_bytes(int kind, int64_t total, int n_frames);
hipError_t launch_bf_prepare(int kind, const void* d_desc, const int64_t* d_frame_off, int n_frames, int64_t total, void* d_prep,
                             hipStream_t stream);
hipError_t launch_bf_match(int kind, const void* d_desc, const void* d_prep, int64_t total, const int64_t* d_frame_off, int n_frames,
                           const gms_pair* d_pairs, int n_pairs, int max_query, gms_dmatch* d_matches, hipStream_t stream);
// bruteForceMatch: cross-check merge, ratio prune and MSVC sort prefix behind the matcher (bf_select_kernels.hip)
size_t     bf_select_ws_bytes(int n_pairs, int64_t max_rows, int64_t total_back);
hipError_t launch_bf_select(int kind, const void* d_desc, const void* d_prep, int64_t total, const int64_t* d_frame_off, int n_frames,
                            const gms_pair* d_pairs, int n_pairs, int max_rows, int64_t total_back, int cross, double coef, int max_size,
                            void* d_ws, gms_dmatch* d_out, gms_bf_result* d_res, gms_pair_result* d_pres, hipStream_t stream);
// consumers of the filtered matches (consumer_kernels.hip)
hipError_t launch_disparity(const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2, const gms_dmatch* d_matches,
                            const int32_t* d_n_matches, int max_matches, int w, int h, const uint8_t* d_gt, int disp_ratio,
                            uint8_t* d_disparity, uint32_t* d_work, gms_disparity_stats* d_stats, hipStream_t stream);
hipError_t launch_gather_points(const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2, const gms_dmatch* d_matches,
                                const int32_t* d_n_matches, int max_matches, float* d_coords1, float* d_coords2, int32_t* d_status,
                                hipStream_t stream);
hipError_t launch_triangulate(const double* camera, const double* dist, const double* P1, const double* P2, const float* d_coords1,
                              const float* d_coords2, const int32_t* d_n_matches, int max_matches, double* d_points3d,
                              gms_triangulation_stats* d_stats, hipStream_t stream);
hipError_t launch_recover_pose(const double* camera, const double P[4][12], double dist_thresh, const float* d_coords1, const float* d_coords2,
                               const int32_t* d_n_matches, int max_matches, const uint8_t* d_in_mask, gms_pose* d_pose, uint8_t* d_out_mask,
                               void* d_work, hipStream_t stream);
// batched consumers (twoview_kernels.hip)
hipError_t launch_gather_batch(const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_m,
                               const gms_dmatch* d_filtered, const gms_pair_result* d_results, float* d_coords1, float* d_coords2,
                               gms_two_view* d_tv, hipStream_t stream);
hipError_t launch_find_essential_batch(const gms_camera& cam, double prob, double threshold, int max_iters, const gms_pair* d_pairs, int n_pairs,
                                       const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv, hipStream_t stream);
hipError_t launch_five_point_selftest(const double* d_pts, int n_samples, double* d_models, int* d_counts, hipStream_t stream);
hipError_t launch_recover_pose_batch(const gms_camera& cam, double dist_thresh, int use_in_mask, const gms_pair* d_pairs, int n_pairs,
                                     const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv, hipStream_t stream);
hipError_t launch_triangulate_batch(const gms_camera& cam, const gms_pair* d_pairs, int n_pairs, const float* d_coords1, const float* d_coords2,
                                    const uint8_t* d_mask, double* d_points3d, gms_two_view* d_tv, hipStream_t stream);
hipError_t launch_disparity_batch(const gms_keypoint* d_kp, const int64_t* d_frame_off, const int32_t* d_wh, int n_frames, const gms_pair* d_pairs,
                                  int n_pairs, int max_m, const gms_dmatch* d_filtered, const gms_pair_result* d_results, const uint8_t* d_gt,
                                  int64_t gt_stride, int disp_ratio, uint8_t* d_disparity, int64_t map_stride, uint32_t* d_work,
                                  gms_disparity_stats* d_stats, hipStream_t stream);
// keypoint source (detect_kernels.hip)
size_t     detect_workspace_bytes(int w, int h, int n_images, int max_keypoints);
hipError_t launch_detect(const uint8_t* d_images, int n_images, int w, int h, int threshold, int max_keypoints, void* d_ws,
                         gms_keypoint* d_kp, uint8_t* d_desc, int32_t* d_counts, hipStream_t stream);
hipError_t launch_describe(const uint8_t* d_image, int w, int h, gms_keypoint* d_kp, int n, void* d_ws, uint8_t* d_desc, int32_t* d_status,
                           hipStream_t stream);
// pyramid keypoint source (detect_kernels.hip): the same detector on every level of an image pyramid (level sizes: ws_layout.h)
void       pyramid_quotas(const int* widths, const int* heights, int n, int max_keypoints, int* quotas);
// what a pyramid run does: the detector, its strength (the FAST threshold or the DoG contrast: dog_kernels.hip) and
// whether the records are refined to 1/16 pixel and 1/16 layer (DoG only; the workspace then ends with the plane of refinement codes)
struct PyramidRun {
    enum Detector { kFast, kDog } detector;
    int strength;
    bool refined;
};
size_t     detect_pyramid_workspace_bytes(int w, int h, int n_images, int max_keypoints, int n_levels, bool refined);
hipError_t launch_pyramid_build(const uint8_t* d_images, int n_images, int w, int h, int n_levels, uint8_t* d_levels, hipStream_t stream);
// d_rows128: the gradient descriptor's rows as well, or nullptr
hipError_t launch_detect_pyramid(const PyramidRun& run, const uint8_t* d_images, int n_images, int w, int h, int max_keypoints, int n_levels, void* d_ws,
                                 gms_keypoint* d_kp, uint8_t* d_desc, float* d_rows128, int32_t* d_counts, int32_t* d_level_counts, hipStream_t stream);
hipError_t launch_detect_maps(const uint8_t* d_images, int n_images, int w, int h, void* d_ws, hipStream_t stream);
// gradient descriptor (grad_desc_kernels.hip; arithmetic in grad_desc_core.h): 128-float rows at the detector's keypoints
hipError_t launch_grad_level(int n_images, int w, int h, int quota, void* d_det_ws, const int32_t* d_level_counts, int level, int out_stride,
                             gms_keypoint* d_kp, float* d_rows128, hipStream_t stream);
hipError_t launch_describe_grad(const uint8_t* d_image, int w, int h, gms_keypoint* d_kp, int n, void* d_ws, float* d_rows128, int32_t* d_status,
                                hipStream_t stream);
// difference-of-Gaussians detector (dog_kernels.hip; arithmetic in dog_core.h): the candidate plane, box sums and score histogram
// (d_box and d_hist may be nullptr) that a level's selection and describe kernels read. d_codes != nullptr: dog_core.h's refinement
// codes (uint16) as well, where d_cand is non-zero; then d_cand == nullptr: on every pixel (0: no candidate), no candidate plane
hipError_t launch_dog_maps(const uint8_t* d_images, int n_images, int w, int h, int contrast, uint8_t* d_cand, uint16_t* d_box, uint32_t* d_hist,
                           uint16_t* d_codes, hipStream_t stream);
// from photographs to the tables (ingest_kernels.hip): BGR -> grey planes; the detector's blocks -> frames back to back
hipError_t launch_bgr_to_gray(const uint8_t* d_bgr, int n, int w, int h, uint8_t* d_gray, hipStream_t stream);
hipError_t launch_detect_pack(const gms_keypoint* d_kp_blocks, const uint8_t* d_rows32_blocks, const float* d_rows128_blocks, const int32_t* d_counts,
                              int n, int max_keypoints, gms_keypoint* d_kp, uint8_t* d_rows32, float* d_rows128, int64_t* d_frame_off,
                              hipStream_t stream);
// batched LOGOS (logos_batch_kernels.hip; layouts in logos_batch.h)
hipError_t launch_logos_prepare(const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const int32_t* d_words,
                                int n_words, void* d_ws, size_t ws_bytes, void* d_table, int n_cus, hipStream_t stream);
hipError_t launch_logos_filter(const void* d_table, const gms_pair* d_pairs, int n_pairs, void* d_ws, size_t ws_bytes, gms_dmatch* d_out,
                               gms_logos_result* d_lres, gms_pair_result* d_pres, int n_cus, hipStream_t stream);
hipError_t launch_logos_words(int kind, const void* d_desc, int64_t total, const void* d_dict, int n_words, int32_t* d_words, int n_cus,
                              hipStream_t stream);
// LOGOS dictionary training (logos_dict_kernels.hip; shared parts and the workspace layout in logos_dict_core.h)
size_t     logos_dict_ws_bytes(const logos_dict::Params& p);
hipError_t launch_logos_dict_train(const logos_dict::Params& p, const void* d_desc, const int64_t* d_set_off, void* d_ws, void* d_dict,
                                   gms_logos_dict_result* d_results, int32_t* d_labels, hipStream_t stream);
// StereoBM block matching (stereo_bm_kernels.hip; shared arithmetic in stereo_bm_core.h)
size_t     stereo_bm_ws_bytes(int n, int W, int H);
hipError_t launch_stereo_bm(const gms_stereo_bm_params& p, const uint8_t* d_left, const uint8_t* d_right, int n, int W, int H, int pitch,
                            void* d_ws, int16_t* d_disp, int32_t* d_cost, hipStream_t stream);
hipError_t launch_stereo_bm_normalize(const int16_t* d_disp, int n, int W, int H, uint8_t* d_out, hipStream_t stream);
hipError_t launch_stereo_bm_prefilter(const gms_stereo_bm_params& p, const uint8_t* d_left, const uint8_t* d_right, int n, int W, int H,
                                      int pitch, uint8_t* pre, hipStream_t stream);
hipError_t launch_stereo_bm_validate(const gms_stereo_bm_params& p, int n, int W, int H, int16_t* d_disp, const int32_t* wcost,
                                     int32_t* d_cost, hipStream_t stream);
// many two-view results into one frame (sfm_register_kernels.hip; shared arithmetic in sfm_register_core.h)
size_t     sfm_register_ws_bytes(int n_pairs, int64_t total_kp, int64_t total_m);
hipError_t launch_sfm_register(const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                               const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_m, const gms_dmatch* d_filtered,
                               const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links,
                               void* d_ws, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_world, int32_t* d_track,
                               int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs, int32_t* d_cloud_est,
                               double* d_cloud_spread, gms_sfm_summary* d_summary, hipStream_t stream, const uint8_t* d_keep = nullptr);
// one-to-one matches per pair (match_unique_kernels.hip; the rule is match_unique_core.h); d_mask, d_tv: null for every slot live
size_t     match_unique_ws_bytes(int64_t total_m);
hipError_t launch_match_unique(const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs, int max_m,
                               int64_t total_m, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_two_view* d_tv, void* d_ws,
                               uint8_t* d_keep, int32_t* d_counts, hipStream_t stream);
// bundle adjustment behind the registration (sfm_ba_kernels.hip; shared arithmetic in sfm_ba_core.h)
size_t     sfm_ba_ws_bytes(int n_frames, int64_t total_kp, int64_t cloud_cap);
hipError_t launch_sfm_ba(const gms_camera& camera, const gms_sfm_ba_params& prm, const gms_keypoint* d_kp, const int64_t* d_frame_off,
                         int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs, int64_t total_m, const gms_dmatch* d_filtered,
                         const uint8_t* d_mask, const gms_sfm_view* d_views, const gms_sfm_pair_reg* d_reg, const int32_t* d_track,
                         int64_t cloud_cap, const double* d_cloud, const int32_t* d_cloud_id, const gms_sfm_summary* d_reg_summary, void* d_ws,
                         gms_sfm_view* d_views_out, double* d_cloud_out, int32_t* d_track_status, gms_sfm_ba_summary* d_summary,
                         hipStream_t stream);
// two-view and registration records of frame pairs from a view array (sfm_pair_pose_kernels.hip; arithmetic in sfm_pair_pose_core.h)
hipError_t launch_sfm_pair_poses(const gms_sfm_view* d_views, int n_frames, const gms_pair* d_pairs, int n_pairs, gms_two_view* d_tv,
                                 gms_sfm_pair_reg* d_reg, hipStream_t stream);
// semi-global matching on StereoBM's costs (stereo_sgm_kernels.hip; shared arithmetic in stereo_sgm_core.h); 0 bytes: beyond size_t
size_t     stereo_sgm_ws_bytes(const gms_stereo_sgm_params& p, int n, int W, int H);
hipError_t launch_stereo_sgm(const gms_stereo_sgm_params& p, const uint8_t* d_left, const uint8_t* d_right, int n, int W, int H, int pitch,
                             void* d_ws, int16_t* d_disp, int32_t* d_cost, hipStream_t stream);
// portrait mode (portrait_kernels.hip; shared parts in portrait_core.h)
size_t     portrait_ws_bytes(int n, int W, int H);
hipError_t launch_portrait(const gms_portrait_params& p, const uint8_t* d_bgr, const uint8_t* d_disp, int n, int W, int H, int pitch_bgr,
                           int pitch_disp, void* d_ws, uint8_t* d_out, uint8_t* d_mask, uint8_t* d_selected, uint8_t* d_blurred,
                           hipStream_t stream, hipEvent_t* stage_events = nullptr);
hipError_t launch_median_blur(const uint8_t* d_src, int n, int W, int H, int channels, int pitch, int ksize, uint8_t* d_dst,
                              hipStream_t stream);
// resize and warpAffine (warp_kernels.hip; arithmetic in warp_core.h): no workspace
hipError_t launch_resize(const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, uint8_t* d_dst, int dw, int dh,
                         int dst_pitch, hipStream_t stream);
hipError_t launch_warp_affine(const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch, const double* d_M, int n_matrices,
                              uint8_t* d_dst, int dw, int dh, int dst_pitch, hipStream_t stream);
// a dense cloud from a posed pair (rectify_kernels.hip; arithmetic in rectify_core.h; workspace: ws_layout.h DenseCloudLayout)
hipError_t launch_rectify_plan(const gms_camera& camera, const gms_two_view* d_tv, int n_pairs, int W, int H, int out_w, int out_h,
                               gms_rectify_plan* d_plans, hipStream_t stream);
hipError_t launch_rectify(const gms_camera& camera, const uint8_t* d_src, int n, int sw, int sh, int channels, int src_pitch,
                          const gms_rectify_plan* d_plans, int n_plans, int which, uint8_t* d_dst, int dw, int dh, int dst_pitch,
                          uint8_t* d_valid, hipStream_t stream);
size_t     dense_cloud_ws_bytes(int n_pairs, int W, int H);
hipError_t launch_dense_cloud(const int16_t* d_disp16, const uint8_t* d_valid, const uint8_t* d_image, int channels, int image_pitch,
                              int n_pairs, int W, int H, const gms_rectify_plan* d_plans, int filtered16, int min_disp16,
                              const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_ws,
                              int cap, float* d_xyz, uint8_t* d_color, int32_t* d_pixel, int32_t* d_count, hipStream_t stream);
// the clouds of several pairs fused into one (dense_fuse_kernels.hip; arithmetic in dense_fuse_core.h; workspace: ws_layout.h DenseFuseLayout)
size_t     dense_fuse_ws_bytes(int n_src, int max_cap);
hipError_t launch_dense_fuse(const gms_dense_fuse_src* d_src, int n_src, int max_cap, const int32_t* d_neighbors, int n_nb, int channels, int tol16,
                             int min_support, void* d_ws, int fused_cap, float* d_xyz, uint8_t* d_color, int32_t* d_source, int32_t* d_index,
                             uint8_t* d_support, uint8_t* d_conflict, int32_t* d_counts, hipStream_t stream);
// the speckle filter on int16 maps, in place (speckle_kernels.hip; shared parts in speckle_core.h; workspace: ws_layout.h SpeckleLayout)
size_t     speckle_ws_bytes(int n, int W, int H);
hipError_t launch_filter_speckles(int16_t* d_disp16, int n, int W, int H, int new_val, int max_speckle_size, int max_diff, void* d_ws,
                                  int32_t* d_removed, hipStream_t stream);
// chessboard corner candidates and cornerSubPix (calib_kernels.hip; arithmetic in calib_core.h; workspace: ws_layout.h ChessLayout)
size_t     chess_candidates_ws_bytes(int n, int w, int h);
hipError_t launch_chess_candidates(const uint8_t* d_images, int n, int w, int h, int max_candidates, void* d_ws,
                                   gms_chess_candidate* d_out, int32_t* d_counts, hipStream_t stream);
hipError_t launch_corner_subpix(const uint8_t* d_images, int n_images, int w, int h, const int32_t* d_image_of, double* d_corners,
                                int n_corners, int max_iter, double eps, int32_t* d_status, hipStream_t stream);
hipError_t launch_threshold(const int32_t* d_T, const int32_t* d_n, const int32_t* d_score, double factor,
                            int count, uint8_t* d_out, hipStream_t stream);

}  // namespace gms
