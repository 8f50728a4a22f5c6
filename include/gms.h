/*
 * gms.h -- C ABI of the MI355X-native GMS (Grid-based Motion Statistics) match filter.
 *
 * Drop-in boundary for ONE reference call:
 *
 *   cv::xfeatures2d::matchGMS(size1, size2, keypoints1, keypoints2, matches1to2, matchesGMS,
 *                             withRotation=false, withScale=false, thresholdFactor=6.0)
 *
 * as called by the reference at
 *   SfM-GMS/SfM-GMS/FeatureMatchUtil.cpp:69      (withRotation=true, withScale=true, 6.0)
 *   SfM-GMS/SfM-GMS/DisparityUtil.cpp:149, :299  (defaults: false, false, 6.0)
 * and implemented (binary only) in SfM-GMS/bin/opencv_xfeatures2d452.dll, export ordinal 884,
 * RVA 0x48280 (opencv_contrib xfeatures2d 4.5.2, class GMSMatcher).
 *
 * Everything here is plain C: pointers, sizes, PODs. No torch, no OpenCV, no C++ types.
 * The work behind every entry point is done by hand-written HIP kernels for gfx950; there is no
 * CPU fallback in this library (a missing/failed GPU is an error code, never a silent detour).
 */
#ifndef MI355_GMS_H
#define MI355_GMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (the reference signals nothing: void return, UB on bad input) ------------- */
#define GMS_OK             0
#define GMS_ERR_BAD_ARG   (-1) /* null pointer / negative size / zero image dimension            */
#define GMS_ERR_DOMAIN    (-2) /* input outside the domain on which the reference is defined     */
#define GMS_ERR_HIP       (-3) /* a HIP runtime call failed (gms_last_hip_error() has the code)  */
#define GMS_ERR_NO_DEVICE (-4) /* no usable gfx950 device                                        */
#define GMS_ERR_CAPACITY  (-5) /* m exceeds what this build supports (see gms_max_matches())     */
#define GMS_ERR_IO        (-7) /* gms_dataset_read / _write: cannot open, short file, or not a GMSFRM01 file             */
#define GMS_ERR_NO_MODEL  (-8) /* two-view stage: fewer than five correspondences, or no essential matrix / pose could be estimated */
#define GMS_ERR_NOT_RESERVED (-6) /* a workspace would have to grow while the stream is being captured: call
                                     gms_ctx_reserve() for this shape first                          */

/* ---- PODs, bit-compatible with the reference's element types ------------------------------- */

/* cv::KeyPoint: 28 bytes, stride 0x1c at DLL@0x1800485d4; only pt.x (+0) and pt.y (+4) are read. */
typedef struct gms_keypoint {
    float x, y;      /* pt                                                      */
    float size;      /* ignored by GMS                                          */
    float angle;     /* ignored                                                 */
    float response;  /* ignored                                                 */
    int32_t octave;  /* ignored                                                 */
    int32_t class_id;/* ignored                                                 */
} gms_keypoint;

/* cv::DMatch: 16 bytes, stride 0x10; queryIdx (+0) and trainIdx (+4) are read (DLL@0x180046aa3),
 * the whole struct is copied verbatim to the output (DLL@0x18004836a). */
typedef struct gms_dmatch {
    int32_t queryIdx;
    int32_t trainIdx;
    int32_t imgIdx;   /* opaque payload, carried through */
    float   distance; /* opaque payload, carried through */
} gms_dmatch;

/* One image pair of a batch: which two resident frames, and where its putative matches live. */
typedef struct gms_pair {
    int32_t frame_a;    /* index of the query ("left") frame  -> keypoints1 / size1 */
    int32_t frame_b;    /* index of the train ("right") frame -> keypoints2 / size2 */
    int32_t m;          /* number of putative matches of this pair                  */
    int32_t reserved;   /* must be 0                                                */
    int64_t match_off;  /* element offset of the pair's first gms_dmatch in the match (and out) array */
} gms_pair;

/* Per-pair result record. */
typedef struct gms_pair_result {
    int32_t n_inliers;  /* number of gms_dmatch written for this pair                           */
    int32_t best_scale; /* 0..4 index into {1, 1/2, 1/sqrt2, sqrt2, 2}; -1 if no hypothesis won  */
    int32_t best_rot;   /* 1..8 rotation pattern; -1 if no hypothesis won                        */
    int32_t status;     /* GMS_OK, GMS_ERR_DOMAIN (input outside the reference's domain) or GMS_ERR_BAD_ARG (the pair's match range overlaps another pair's) */
} gms_pair_result;

typedef struct gms_ctx gms_ctx;

/* ---- one-shot drop-in ------------------------------------------------------------------------
 * Same contract as the reference call: inputs borrowed, `out` must have room
 * for m entries, receives the surviving matches verbatim and in input order, *n_out their number.
 * Host pointers. Uses a lazily created process-wide context on device 0.
 * Replaces: cv::xfeatures2d::matchGMS (FeatureMatchUtil.cpp:69; DisparityUtil.cpp:149,299). */
int gms_match(const gms_keypoint* kp1, int n1, int w1, int h1,
              const gms_keypoint* kp2, int n2, int w2, int h2,
              const gms_dmatch* matches, int m,
              int with_rotation, int with_scale, double threshold_factor,
              gms_dmatch* out, int* n_out);

/* Same, on an explicit context; additionally reports the winning hypothesis (may be NULL). */
int gms_match_ctx(gms_ctx* ctx,
                  const gms_keypoint* kp1, int n1, int w1, int h1,
                  const gms_keypoint* kp2, int n2, int w2, int h2,
                  const gms_dmatch* matches, int m,
                  int with_rotation, int with_scale, double threshold_factor,
                  gms_dmatch* out, int* n_out, gms_pair_result* result);

/* ---- context --------------------------------------------------------------------------------
 * One context per (process, device). Every entry point that takes a context serialises on it (a context may be
 * shared by host threads); work is ordered on the context's current stream. If the stream is changed while earlier
 * launches are still running, later launches that reuse the context's internal workspaces wait for them (an event). */
int  gms_ctx_create(int device, gms_ctx** out_ctx);
int  gms_ctx_destroy(gms_ctx* ctx);
/* Launch on a caller-owned hipStream_t (pass it as void*); NULL selects the context's own stream. */
int  gms_ctx_set_stream(gms_ctx* ctx, void* hip_stream);
int  gms_ctx_synchronize(gms_ctx* ctx);
/* Sizes the internal workspaces for gms_filter_device calls of up to n_pairs pairs of up to max_m matches under the
 * given flags. After it, such calls neither allocate nor synchronise -- they are pure stream-ordered launches and can
 * be captured into a hipGraph. May allocate and synchronise itself. */
int  gms_ctx_reserve(gms_ctx* ctx, int n_pairs, int max_m, int with_rotation, int with_scale);
/* What the context's most recent gms_filter_device launch ran with, for reports (bench.py prints them beside its numbers). The
 * library picks between bit-identical kernel variants from what earlier launches of the context saw: a probe kernel behind
 * every sixteenth launch writes a verdict, and the first later launch that finds that kernel complete adopts it. */
#define GMS_QUERY_LAST_DEALT        1 /* 1: the byte-matrix kernel dealt the matches to its lanes (inputs in spatial order) */
#define GMS_QUERY_LAST_SCALE_PROBE  2 /* bit s set: scale hypothesis s was bounded by a probe before being evaluated; bit 8 + s: with four-bit entries first */
#define GMS_QUERY_LAST_KPT          3 /* matches per thread of the workgroup kernel (0: the large-pair kernels ran)        */
#define GMS_QUERY_LAUNCHES          4 /* filter launches of the context so far                                             */
#define GMS_QUERY_CUS               5 /* compute units of the context's device                                             */
#define GMS_QUERY_PREFETCH_TYPE     6 /* byte-matrix kernel: grid type (0..3) before which a workgroup touches the match records of
                                         the pair its CU's next workgroup will filter, so that they wait in L2 (-1: never)        */
#define GMS_QUERY_PREFETCH_AHEAD    7 /* ... how many pairs ahead that pair is (the number of CUs unless GMS_PREFETCH says otherwise) */
#define GMS_QUERY_STAGGER_TICKS     8 /* first-round start spread of the most recent launch, in 10 ns ticks (0: none)             */
#define GMS_QUERY_LAST_IDENT        9 /* 1: the byte-matrix kernel ran its identity-query instantiation (match k of a pair is query k, one
                                         match per keypoint of frame A: what gms_bfmatch_device and cv::BFMatcher::match return)      */
#define GMS_QUERY_IDENT_MISSES     10 /* pairs that instantiation has had to filter with the generic body so far (a device counter, read
                                         without waiting: complete for the launches the caller has synchronised with)              */
int  gms_ctx_query(gms_ctx* ctx, int what, int64_t* value);
/* Forces one of those choices for the context's later launches (value 0 / 1), or hands it back to the library (-1, the default).
 * Speed only: every variant produces the same bytes. The environment switches GMS_DEAL / GMS_SCALE_PROBE / GMS_IDENT do the same process-wide. */
#define GMS_OPTION_DEAL         1
#define GMS_OPTION_SCALE_PROBE  2
#define GMS_OPTION_IDENT        3 /* (GMS_IDENT): identity-query pairs under the default flags. Forced on, every pair is still checked and a
                                     pair that is not one -- or whose table this context did not build last -- takes the generic body */
int  gms_ctx_set_option(gms_ctx* ctx, int option, int value);

/* ---- device-resident batch path (throughput API) ---------------------------------------------
 * All d_* pointers are device pointers on the context's device; calls are stream-ordered on the
 * context's stream. gms_normalize_device does not synchronise (but see the side records below). gms_filter_device does not synchronise or allocate
 * once the shape has been reserved (gms_ctx_reserve); without a reservation it grows its workspaces on first
 * use of a larger shape (one hipStreamSynchronize + hipMalloc then), and returns GMS_ERR_NOT_RESERVED instead
 * if that would have to happen inside a stream capture. Batches of pairs up to 16 384 matches under the
 * default flags need no workspace at all.
 *
 * gms_normalize_device: GMSMatcher::normalizePoints (DLL@0x180048420) for every keypoint of every
 * frame: d_pts[2*i] = kp[i].x / (float)w[frame], d_pts[2*i+1] = kp[i].y / (float)h[frame]
 * (IEEE fp32 divide). d_frame_off has n_frames+1 entries (keypoint offsets), d_wh 2*n_frames ints.
 * d_pts is the frame table the filter works from and needs gms_frame_table_bytes(total_kp) bytes (16 per keypoint + 32):
 * a 16-byte header (GMS_FRAME_TABLE_HEADER_BYTES: a magic word and total_kp, so that the table describes itself), the
 * normalised points (8 bytes each, point i at float index 4 + 2 i), then 8 bytes of cell codes per keypoint -- everything
 * about a keypoint that does not depend on the pair it is matched in (its cells on the left grid's four half-cell shifted
 * types and on the right grids of setScale) is worked out once per frame here, not once per pair. Opaque beyond the points;
 * always pass the block back whole (16-byte aligned). gms_filter_device may be given any n_frames / d_frame_off whose frames lie
 * inside the table (a prefix of the frames, say): where the code arrays are is read from the header, not derived from the call. */
#define GMS_FRAME_TABLE_HEADER_BYTES 16
int64_t gms_frame_table_bytes(int64_t total_kp);
int gms_normalize_device(gms_ctx* ctx, const gms_keypoint* d_kp, const int64_t* d_frame_off,
                         const int32_t* d_wh, int n_frames, int64_t total_kp, float* d_pts);
/* Beside the table a build fills per-frame side records in a buffer of the CONTEXT (the half-cell histogram of each frame's keypoints
 * as left points, GMS_SIDE_RECORD_BYTES each): what the filter's identity-query instantiation needs of a pair's frame A. They describe
 * the context's LATEST build only; table and records carry a stamp (a 64-bit digest of what the records were built from, in the
 * table's spare bytes: equal tables stay byte-identical), and a table whose stamp is not the records' -- built from other keypoints
 * by this or another context, at the same address or not -- is filtered by the generic code. The buffer holds 2048 frames from the start; a build of more frames grows it, which
 * synchronises the device once (a build inside a stream capture that would have to grow it leaves no records instead), and a table of
 * more than 64 MiB of records gets none.
 * gms_ctx_read_side_records: diagnostic. Waits for the context's stream and copies the records of the latest build to host memory:
 * per frame int64 first keypoint, int32 keypoint count, uint32 flags (1: a keypoint outside the parity domain, 2: a half cell above 255
 * keypoints), uint64 stamp, 8 spare bytes, then 400 dwords -- cell c of the 20 x 20 grid, byte (hx & 1) + 2 (hy & 1) of it the
 * count of its half cell. *n_frames: how many records there are (0: the latest build left none); at most dst_bytes are written. */
#define GMS_SIDE_RECORD_BYTES 1632
int gms_ctx_read_side_records(gms_ctx* ctx, void* dst, size_t dst_bytes, int* n_frames);

/* gms_filter_device: the GMS filter proper (GMSMatcher ctor..getInlierMask..copy-out, DLL@0x180046900,
 * 0x180047dc0, 0x180048630, 0x180048d10, 0x180048340) for n_pairs independent pairs.
 *   d_pts/d_frame_off  normalised keypoint table from gms_normalize_device
 *   d_pairs            n_pairs descriptors; max_m >= every d_pairs[i].m (host-known upper bound)
 *   d_matches          putative matches, pair i at [match_off, match_off+m). The ranges of a batch's pairs must be DISJOINT
 *                      (empty pairs aside): pair i's survivors are written over the head of the same range of d_out, so
 *                      overlapping ranges would make pairs overwrite each other. Validated on the device BEHIND the first launch
 *                      of a context and every sixteenth (every launch with GMS_CHECK_PAIRS=1; never inside a stream capture or a
 *                      graph replay): every pair whose range overlaps another's gets status GMS_ERR_BAD_ARG in d_results. The check
 *                      reports, it does not prevent: d_out of the flagged pairs AND of whatever their ranges touch has already been
 *                      written by then and is invalid, and a launch that is not checked returns GMS_OK on such a table. A caller
 *                      that cannot vouch for its table validates it once itself (gms_filter_host_batch does: every call, on the
 *                      host, GMS_ERR_BAD_ARG before anything is launched).
 *   d_out              same offsets/capacity; pair i's survivors are written at d_out[match_off ...]
 *   d_results          n_pairs result records
 *   d_mask             optional (may be NULL): per-match inlier byte (0/1) at the match's offset */
int gms_filter_device(gms_ctx* ctx, const float* d_pts, const int64_t* d_frame_off, int n_frames,
                      const gms_pair* d_pairs, int n_pairs, int max_m,
                      const gms_dmatch* d_matches,
                      int with_rotation, int with_scale, double threshold_factor,
                      gms_dmatch* d_out, gms_pair_result* d_results, uint8_t* d_mask);

/* ---- host-pointer batch path -------------------------------------------------------------------
 * The throughput entry for callers that hold everything in host memory (a C++ caller of the reference looping over
 * image pairs: FeatureMatchUtil.cpp:66-69 once per pair): the frames' keypoints are uploaded and normalised once,
 * then the pair list is cut into chunks (at most 2^21 matches or 8192 pairs each; a larger pair is a chunk of its own) that
 * travel through pinned staging buffers on three lanes, each with a stream of its own; chunk k rides lane k % 3, so that
 * chunk k+1 is uploaded while chunk k is filtered and chunk k-1 comes back. Synchronous: returns when out/results are complete.
 *   kp/frame_off/wh   keypoints of all frames back to back, n_frames+1 offsets, (w, h) per frame. frame_off[0] must be 0 and the
 *                     offsets must never decrease (GMS_ERR_BAD_ARG before anything is copied or launched otherwise); kp must hold
 *                     at least frame_off[n_frames] records -- the library cannot check that, it reads that many
 *   pairs/matches     as gms_filter_device, host memory; match_off indexes `matches` and `out` alike
 *   out               pair i's survivors verbatim at out[match_off .. match_off + results[i].n_inliers)
 * Only those records of out are written: the rest of each pair's range, and whatever lies outside every pair's range, keep what
 * they held; so do results[n_pairs ..]. Returns GMS_OK, or the first error; pairs outside the parity domain are reported per
 * pair in results[i].status. */
int gms_filter_host_batch(gms_ctx* ctx, const gms_keypoint* kp, const int64_t* frame_off, const int32_t* wh,
                          int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* matches,
                          int with_rotation, int with_scale, double threshold_factor,
                          gms_dmatch* out, gms_pair_result* results);

/* ---- brute-force descriptor matcher: the producer of the match array ------------------------------------
 * Replaces, for a batch of pairs on the resident frame table, what the reference runs in front of matchGMS
 * (FeatureMatchUtil.cpp:66-68; DisparityUtil.cpp:104-109,143):
 *     BFMatcher::create(normType)->match(descriptors1, descriptors2, matches)          (no cross-check)
 * Descriptor i of a frame belongs to keypoint i (same d_frame_off as the keypoint table). Pair p gets
 * one match per query row -- {queryIdx = i, trainIdx = first minimum over the train rows, imgIdx = 0, distance} for
 * i < min(d_pairs[p].m, n(frame_a)) -- written at d_matches[match_off + i]: the array gms_filter_device reads next.
 *   GMS_DESC_HAMMING256    rows of 32 bytes (ORB), NORM_HAMMING, distance = popcount as float. With a prepared block the
 *                          cross term runs on the matrix cores (the bits as FP4 elements, exact); with d_prepared = NULL on
 *                          the vector ALUs straight from the raw rows. Same results.
 *   GMS_DESC_L2_F32X128    rows of 128 floats (SIFT), NORM_L2, distance = sqrtf(sum of squared differences in fp32); needs
 *                          the prepared block. Frames whose values are all integers 0..255 (what SIFT emits) run on the
 *                          matrix cores (as int8, exact arithmetic); any other frame is matched by the reference's fp32 loop.
 * gms_bf_prepare_device builds the per-frame tables (gms_bf_prepared_bytes bytes, caller-allocated) once per frame table.
 * Stream-ordered on the context's stream, no allocation, no synchronisation. A frame may hold at most 2^22 rows. */
#define GMS_DESC_NONE      (-1)
#define GMS_DESC_HAMMING256  0
#define GMS_DESC_L2_F32X128  1
int64_t gms_bf_prepared_bytes(int desc_kind, int64_t total_desc, int n_frames);
int gms_bf_prepare_device(gms_ctx* ctx, int desc_kind, const void* d_desc, const int64_t* d_frame_off, int n_frames,
                          int64_t total_desc, void* d_prepared);
int gms_bfmatch_device(gms_ctx* ctx, int desc_kind, const void* d_desc, const void* d_prepared, int64_t total_desc,
                       const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_query,
                       gms_dmatch* d_matches);

/* ---- bruteForceMatch: cross-check, sort and ratio prune (FeatureMatchUtil.cpp:20-31) --------------------------
 * What the reference's DEFAULT_SIFT method and its SIFT_matchBF baseline run:
 *     BFMatcher(normType, crossCheck = true).match(desc1, desc2, matches); std::sort(matches);
 *     while (front.distance * coef < back.distance) pop_back;  while (size > max_size) pop_back;     (coef 4.0, max_size 500)
 * for n_pairs pairs of the resident descriptor table of gms_bfmatch_device (same d_desc / d_prepared / d_frame_off / desc_kind).
 * Cross-check is OpenCV's one-sided rule, not a mutual-nearest test: every row i of frame_b takes its first nearest row tidx[i] of
 * frame_a, and query row q keeps, among the i with tidx[i] == q, the one of smallest distance (lowest i on ties). The candidates,
 * (q, t = that i, imgIdx = 0, distance) in ascending q, are sorted by distance in the order MSVC's std::sort leaves them (unstable;
 * restated in bf_select_core.h) and the first K = min(max_size, #{d : !((double)d_min * coef < (double)d)}) are the survivors.
 * cross_check = 0: the candidates are the plain forward matches of gms_bfmatch_device (the reference's match() helper, :38-50).
 * imgIdx is 0 (the matcher's convention; OpenCV's split of trainIdx above 2^18 train rows is not reproduced).
 *
 * gms_bf_select_device: for a gms_pair here, m is the pair's OUTPUT CAPACITY and match_off where its survivors start in d_out (ranges
 *   disjoint). max_rows bounds both frames of every pair (a pair with a larger frame gets GMS_ERR_BAD_ARG); the matcher's grid is
 *   sized by it. d_bf_results gets one record per pair. K > m: nothing of the pair is written, status GMS_ERR_CAPACITY, n_out = K.
 *   An empty frame: no survivors, GMS_ERR_DOMAIN (the reference calls front() on an empty vector). A frame index out of range,
 *   m < 0, or more matcher rows than total_backward_rows over the pairs before it: GMS_ERR_BAD_ARG. d_pair_results (optional)
 *   gets {n_inliers = survivors written, -1, -1, status} for gms_two_view_batch_device / gms_disparity_batch_device.
 *   coef < 1 or not finite, max_size < 0, a bad kind or pointer, or too small a workspace: GMS_ERR_BAD_ARG for the call, nothing run.
 *   Stream-ordered on the context's stream; no allocation, no synchronisation (graph-capturable).
 * gms_bf_select_workspace_bytes(n_pairs, max_rows, total_backward_rows): the workspace (256-byte aligned pointer), where
 *   total_backward_rows >= the sum over pairs of n(frame_b) with cross-check, of n(frame_a) without.
 * gms_bf_match_select: the same for ONE pair on host rows (desc1: n1 query rows, desc2: n2 train rows), synchronous, on the current
 *   HIP device; out_cap: room in out; *n_out: K, also when it exceeds out_cap (GMS_ERR_CAPACITY, nothing written). Byte-identical to
 *   the batched call for that pair. result may be NULL. */
typedef struct gms_bf_result {
    int64_t n_candidates; /* cross-check survivors (forward matches without cross-check)         */
    int64_t n_ratio;      /* candidates with !(d_min * coef < d)                                 */
    int64_t n_out;        /* K = min(max_size, n_ratio): survivors (the needed count on overflow) */
    float   d_min;        /* smallest candidate distance; 0 when there is none                   */
    int32_t status;       /* GMS_OK, _DOMAIN, _CAPACITY or _BAD_ARG                               */
} gms_bf_result;

size_t gms_bf_select_workspace_bytes(int n_pairs, int max_rows, int64_t total_backward_rows);
int gms_bf_select_device(gms_ctx* ctx, int desc_kind, const void* d_desc, const void* d_prepared, int64_t total_desc,
                         const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs, int max_rows, int cross_check,
                         double distance_coef, int max_size, void* d_ws, size_t ws_bytes, gms_dmatch* d_out, gms_bf_result* d_bf_results,
                         gms_pair_result* d_pair_results);
int gms_bf_match_select(int desc_kind, const void* desc1, int n1, const void* desc2, int n2, int cross_check, double distance_coef,
                        int max_size, gms_dmatch* out, int64_t out_cap, int64_t* n_out, gms_bf_result* result);
/* gms_bf_select_host_batch: prepare + select on host arrays, synchronous (the C++ shim's batch form): desc holds frame_off[n_frames]
 * rows; pairs / out / results as for gms_bf_select_device, in host memory. */
int gms_bf_select_host_batch(gms_ctx* ctx, int desc_kind, const void* desc, const int64_t* frame_off, int n_frames, const gms_pair* pairs,
                             int n_pairs, int cross_check, double distance_coef, int max_size, gms_dmatch* out, gms_bf_result* results);

/* ---- consumers of the filtered matches --------------------------------------------------------------------
 * Both read the survivors of ONE pair where gms_filter_device left them (d_matches = d_out + match_off, *d_n_matches =
 * d_results[i].n_inliers, max_matches >= that count, e.g. the pair's m) and the two frames' ORIGINAL keypoints (pixel
 * coordinates, cv::KeyPoint records). Stream-ordered, no allocation, no synchronisation.
 *
 * gms_disparity_device: DisparityUtil.cpp:179-201. d_disparity (w*h bytes, row-major) receives the disparity map (255 = no
 * match; a later match overwrites an earlier one on the same pixel); with a ground-truth image d_gt (w*h bytes, may be NULL)
 * d_stats receives count / sum of squares / maximum of |map - gt / disp_ratio| over the matched pixels, from which
 * rms = sqrt(sum_sq / count) (DisparityUtil.cpp:201). d_work: w*h uint32 of scratch. status: GMS_ERR_DOMAIN when a match
 * indexes outside the keypoints or lands outside the image (undefined behaviour in the reference). */
typedef struct gms_disparity_stats {
    int64_t count;    /* matched pixels (map != 255) */
    int64_t sum_sq;   /* sum of a^2, a = |map - gt / disp_ratio| */
    int32_t max_abs;  /* max a */
    int32_t status;   /* GMS_OK or GMS_ERR_DOMAIN */
} gms_disparity_stats;
int gms_disparity_device(gms_ctx* ctx, const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2,
                         const gms_dmatch* d_matches, const int32_t* d_n_matches, int max_matches, int width, int height,
                         const uint8_t* d_gt, int disp_ratio, uint8_t* d_disparity, uint32_t* d_work,
                         gms_disparity_stats* d_stats);
/* gms_gather_points_device: SfMUtil.cpp:25-35. coords1[i] = keypoints1[queryIdx].pt, coords2[i] = keypoints2[trainIdx].pt
 * (two floats each) for i < *d_n_matches: the arrays findEssentialMat / recoverPose / undistortPoints take (SfMUtil.cpp:39,
 * 45,78-79). *d_status: GMS_OK or GMS_ERR_DOMAIN. */
int gms_gather_points_device(gms_ctx* ctx, const gms_keypoint* d_kp1, int n1, const gms_keypoint* d_kp2, int n2,
                             const gms_dmatch* d_matches, const int32_t* d_n_matches, int max_matches,
                             float* d_coords1, float* d_coords2, int32_t* d_status);

/* gms_triangulate_device: SfMUtil.cpp:76-82 and 128-143 for the gathered points -- cv::undistortPoints (camera = fx, fy, cx, cy;
 * dist = k1, k2, p1, p2, k3 or NULL), cv::triangulatePoints with the 3 x 4 row-major projection matrices P1, P2 (the reference
 * uses [I|0] and [R|t] from recoverPose), division by the fourth coordinate. d_points3d receives 3 doubles per match;
 * d_stats the sums of squared reprojection errors in both views (normalised image coordinates), the number of finite points
 * and how many of them lie behind a camera. fp64; agrees with OpenCV's SVD-based routine to rounding, not bit for bit.
 * camera / dist / P1 / P2 are HOST pointers (they travel as kernel arguments). */
typedef struct gms_triangulation_stats {
    double  sum_sq_err1, sum_sq_err2;
    int64_t count, behind;
} gms_triangulation_stats;
int gms_triangulate_device(gms_ctx* ctx, const double camera[4], const double dist[5], const double P1[12], const double P2[12],
                           const float* d_coords1, const float* d_coords2, const int32_t* d_n_matches, int max_matches,
                           double* d_points3d, gms_triangulation_stats* d_stats);

/* gms_recover_pose_device: cv::recoverPose(E, points1, points2, cameraMatrix, R, t, mask) as SfMUtil.cpp:45 calls it (OpenCV 4.5.2:
 * distance threshold 50) for the gathered points: the four (R, t) the essential matrix decomposes into, each tried on every
 * correspondence by triangulation in normalised coordinates (positive depth below the threshold in both cameras); the first of
 * (R1, t), (R2, t), (R1, -t), (R2, -t) with the most such points wins. E (3 x 3 row-major) and camera = (fx, fy, cx, cy) are HOST
 * pointers; d_in_mask (optional: findEssentialMat's inlier mask, non-zero = use) and everything else device pointers.
 * *d_pose receives R, t, the winner's point count and its index; d_out_mask (optional) per correspondence what the reference's
 * bitwise_and leaves: the input mask's byte where the point passes (255 without an input mask), 0 elsewhere.
 * Stream-ordered; the context keeps max_matches + 48 bytes of scratch, which grows (one stream synchronisation) on first use of a
 * larger max_matches -- GMS_ERR_NOT_RESERVED instead when the stream is being captured; gms_ctx_reserve(ctx, 1, max_matches, ...) sizes it. fp64, agrees with OpenCV to rounding (R1 / R2 and the
 * sign of t may be numbered differently than by another SVD: `which` is informational). */
typedef struct gms_pose {
    double  R[9], t[3];
    int32_t n_good, which;
} gms_pose;
int gms_recover_pose_device(gms_ctx* ctx, const double E[9], const double camera[4], const float* d_coords1, const float* d_coords2,
                            const int32_t* d_n_matches, int max_matches, const uint8_t* d_in_mask, gms_pose* d_pose,
                            uint8_t* d_out_mask);

/* ---- the same consumers for a whole batch ---------------------------------------------------------------------------
 * What structureFromMotion does with the survivors of ONE pair (SfMUtil.cpp:25-82) and matchBasedDispCalculate with its map
 * (DisparityUtil.cpp:170-201), for every pair of a batch per launch: same pair table, same offsets as gms_filter_device. Every
 * per-match array (coords, mask, 3-D points) holds pair i's entries at its match_off (coords: 2 floats per match, points: 3 doubles),
 * d_tv holds one record per pair. Stream-ordered on the context's stream, no allocation, no synchronisation, capturable.
 *
 *   gms_gather_points_batch_device   SfMUtil.cpp:25-35. Zeroes d_tv, then n_points = the pair's n_inliers and the coordinates.
 *   gms_find_essential_batch_device  SfMUtil.cpp:39: cv::findEssentialMat(coords1, coords2, cameraMatrix, RANSAC, prob, threshold,
 *       mask) of OpenCV 4.5.2 -- points normalised with the camera matrix, threshold / ((fx + fy) / 2), RANSAC over five-point
 *       minimal solves (Nister) with cv::RNG((uint64)-1) drawing the samples, at most max_iters (OpenCV: 1000) iterations, the
 *       bound shrinking by RANSACUpdateNumIters(prob, ...) whenever a model with strictly more inliers appears; error =
 *       (x2^T E x1)^2 / (|E x1|_xy^2 + |E^T x2|_xy^2) as fp32 against (float)threshold^2. E: row-major, unit Frobenius norm, largest
 *       entry positive (an SVD leaves the sign open); the models of one sample are tried in ascending order of E[0], E[1], ...
 *       (OpenCV's order is that of its polynomial root finder: it only matters between models of equal inlier count).
 *       d_mask: 1 / 0 per correspondence. Pairs with fewer than five correspondences or no model: status GMS_ERR_NO_MODEL.
 *       fp64; agrees with an SVD / eigenvalue based implementation to rounding, not bit for bit.
 *   gms_recover_pose_batch_device    SfMUtil.cpp:45: cv::recoverPose(E, coords1, coords2, cameraMatrix, R, t, mask), distance
 *       threshold 50; d_mask is in/out as in the reference (use_in_mask = 0: output only, 255 / 0).
 *   gms_triangulate_batch_device     SfMUtil.cpp:65-82,128-143: the correspondences with a non-zero mask byte (d_mask NULL: all),
 *       compacted in order, cv::undistortPoints, cv::triangulatePoints with [I|0] and [R|t], division by the fourth coordinate:
 *       pair i's n_triangulated points at d_points3d[3 * match_off ...]; reprojection error sums in normalised coordinates.
 *   gms_two_view_batch_device        all four, in stream order.
 *   gms_disparity_batch_device       DisparityUtil.cpp:170-201 per pair: pair i's map (width x height of frame_a, row-major) at
 *       d_disparity + i * map_stride, its ground truth (optional) at d_gt + i * gt_stride (gt_stride 0: one image for all),
 *       d_work: n_pairs * map_stride uint32 of scratch, d_stats one record per pair. */
typedef struct gms_camera {   /* cameraMatrix and distCoeffs as structureFromMotion receives them (SfMUtil.cpp:4; main.cpp:59-67) */
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3;
} gms_camera;
typedef struct gms_two_view {
    double  E[9];                      /* findEssentialMat                                                   */
    double  R[9], t[3];                /* recoverPose                                                        */
    double  sum_sq_err1, sum_sq_err2;  /* sums of squared reprojection errors of the triangulated points     */
    int64_t n_finite, n_behind;        /* triangulated points that are finite / of those, behind a camera    */
    int32_t n_points;                  /* correspondences of the pair (the filter's n_inliers)               */
    int32_t n_ransac;                  /* inliers of E (non-zero bytes of findEssentialMat's mask)           */
    int32_t ransac_iters;              /* RANSAC iterations run                                              */
    int32_t n_pose;                    /* recoverPose's return value                                         */
    int32_t pose_which;                /* which of (R1,t) (R2,t) (R1,-t) (R2,-t) won: informational          */
    int32_t n_triangulated;            /* points written to d_points3d                                       */
    int32_t status;                    /* GMS_OK, GMS_ERR_DOMAIN, GMS_ERR_NO_MODEL, or the filter's status   */
    int32_t reserved;
} gms_two_view;
int gms_gather_points_batch_device(gms_ctx* ctx, const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames,
                                   const gms_pair* d_pairs, int n_pairs, int max_m, const gms_dmatch* d_filtered,
                                   const gms_pair_result* d_results, float* d_coords1, float* d_coords2, gms_two_view* d_tv);
int gms_find_essential_batch_device(gms_ctx* ctx, const gms_camera* camera, double prob, double threshold, int max_iters,
                                    const gms_pair* d_pairs, int n_pairs, const float* d_coords1, const float* d_coords2,
                                    uint8_t* d_mask, gms_two_view* d_tv);
int gms_recover_pose_batch_device(gms_ctx* ctx, const gms_camera* camera, int use_in_mask, const gms_pair* d_pairs, int n_pairs,
                                  const float* d_coords1, const float* d_coords2, uint8_t* d_mask, gms_two_view* d_tv);
int gms_triangulate_batch_device(gms_ctx* ctx, const gms_camera* camera, const gms_pair* d_pairs, int n_pairs,
                                 const float* d_coords1, const float* d_coords2, const uint8_t* d_mask, double* d_points3d,
                                 gms_two_view* d_tv);
int gms_two_view_batch_device(gms_ctx* ctx, const gms_camera* camera, double prob, double threshold, int max_iters,
                              const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, const gms_pair* d_pairs, int n_pairs,
                              int max_m, const gms_dmatch* d_filtered, const gms_pair_result* d_results, float* d_coords1,
                              float* d_coords2, uint8_t* d_mask, double* d_points3d, gms_two_view* d_tv);
int gms_disparity_batch_device(gms_ctx* ctx, const gms_keypoint* d_kp, const int64_t* d_frame_off, const int32_t* d_wh, int n_frames,
                               const gms_pair* d_pairs, int n_pairs, int max_m, const gms_dmatch* d_filtered,
                               const gms_pair_result* d_results, const uint8_t* d_gt, int64_t gt_stride, int disp_ratio,
                               uint8_t* d_disparity, int64_t map_stride, uint32_t* d_work, gms_disparity_stats* d_stats);

/* ---- many views into one frame (the library's own step behind the batched two-view stage) -----------------------
 * Every pair of gms_two_view_batch_device has its own frame (camera frame_a) and its own unit (|t| = 1). This stage joins the pairs
 * of a spanning forest out of a root frame: per pair a scale from the scene points it shares with the pair it hangs on, per frame
 * a pose [R | t] in the root's frame and the first pair's unit, every pair's points in that frame, and the tracks the surviving
 * matches chain keypoints into, as one cloud. The inputs are exactly what the two-view stage leaves on the device: d_frame_off,
 * d_pairs, the survivors d_filtered, d_mask, d_points3d (pair i's points at match_off + rank, rank = non-zero mask bytes before the
 * match) and d_tv. tests/sfm_register_ref.py is the definition in numpy.
 *
 * gms_sfm_plan (host, pure arithmetic): walks the pairs in order with registered = {root}. Pair i registers frame_b when frame_a is
 *   registered and frame_b is not; its link is the pair that registered frame_a (role 1: the shared frame is that pair's frame_b),
 *   or for frame_a = root the first registering pair out of the root (role 0; that pair has link -1). depth = the link's + 1.
 *   Every other pair (reverse direction, both frames registered -- loop closure is not done --, neither registered) has
 *   registers = 0 and ends as GMS_SFM_SKIPPED. A frame index or root out of range: GMS_ERR_BAD_ARG.
 * gms_sfm_register_device: d_plan is the plan of the same pairs, in device memory. Pair i is ok when it registers, its two-view status
 *   is GMS_OK with n_triangulated > 0 and, with a link j, pair j is ok and n_links >= min_links; otherwise GMS_ERR_NO_MODEL, and the
 *   pairs that hang on it fail the same way. A link: a match of pair i (non-zero mask) whose queryIdx is named by a non-zero-mask
 *   match of pair j (through its queryIdx for role 0, its trainIdx for role 1; the lowest such match counts), with both points finite
 *   and z > 0 (pair j's point for role 1 as R_j p + t_j); n_links counts them, r is the lower median of |X| / |Y| over them, S the
 *   product of r along the links (1 without). Views: G_root = [I | 0], G_b = [R_i G_a.R | R_i G_a.t + S_i t_i]. d_points_world
 *   (3 doubles per match slot, as d_points3d) = G_a.R^T (S_i p - G_a.t), 0 in every slot that holds no point of an ok pair; d_track
 *   (int32 per match slot): the point's track, -1 without one. Both are written for every slot below total_matches. A track is a connected component of the edges (frame_off[a] + queryIdx, frame_off[b] +
 *   trainIdx) of the ok pairs' non-zero-mask matches; its id is its least global keypoint index. The cloud has one entry per track
 *   in ascending id, the first cloud_cap of them: d_cloud (3 doubles: the world point of the track's estimate of lowest (pair,
 *   rank)), d_cloud_id, d_cloud_obs (keypoints), d_cloud_est (estimates), d_cloud_spread (largest distance from that point to
 *   another estimate of the track; a distance that is not a number does not count). Matches that index outside their frames are ignored. Integers are exact; doubles agree with the
 *   numpy statement to rounding. root out of range, min_links < 1, a null pointer, total_kp >= 2^31 - 1, a workspace that is not
 *   256-byte aligned or too small: GMS_ERR_BAD_ARG, nothing run. Stream-ordered on the context's stream; no allocation, no
 *   synchronisation, no readback (graph-capturable).
 * gms_sfm_register_workspace_bytes: the workspace for n_pairs pairs over total_kp keypoints and total_matches match slots (0: refused).
 * gms_sfm_register: plan + the device call on host arrays, synchronous, on the current HIP device; the outputs cover every match
 *   slot below max(match_off + m) and cloud_cap entries (what the device call leaves untouched is 0). A pair with m < 0,
 *   match_off < 0 or match_off > 2^40 - m (held so, before the sum is formed): GMS_ERR_BAD_ARG, nothing run. */
#define GMS_SFM_SKIPPED 1   /* gms_sfm_pair_reg.status of a pair the plan does not use */
typedef struct gms_sfm_plan_entry {
    int32_t registers;  /* 1: the pair registers its frame_b                     */
    int32_t link;       /* the pair it takes its scale from; -1: none            */
    int32_t role;       /* 0: the shared frame is the link's frame_a, 1: frame_b */
    int32_t depth;      /* links between the pair and one without a link         */
} gms_sfm_plan_entry;
typedef struct gms_sfm_view {
    double  R[9], t[3];  /* x_camera = R x_world + t; zeros when not registered  */
    int32_t registered;  /* 1: the root, or registered by an ok pair             */
    int32_t pair;        /* the pair that registered the frame; -1: none         */
} gms_sfm_view;
typedef struct gms_sfm_pair_reg {
    double  r, S;        /* the pair's scale against its link (0 when not measured) and the cumulative scale (0 when not ok) */
    int32_t n_links;     /* valid links (0 when either pair has no two-view result)                                           */
    int32_t depth, link, role;  /* the plan's                                                                                 */
    int32_t status;      /* GMS_OK, GMS_SFM_SKIPPED or GMS_ERR_NO_MODEL                                                      */
    int32_t reserved;
} gms_sfm_pair_reg;
typedef struct gms_sfm_summary {
    int64_t n_tracks;      /* tracks (also when more than cloud_cap)                */
    int64_t n_points;      /* estimates: points of ok pairs that belong to a track  */
    int64_t n_multi;       /* tracks that hold two keypoints of one frame (kept)    */
    int32_t n_registered;  /* registered frames, the root included                  */
    int32_t n_ok_pairs;
} gms_sfm_summary;
int gms_sfm_plan(const gms_pair* pairs, int n_pairs, int n_frames, int root, gms_sfm_plan_entry* plan);
size_t gms_sfm_register_workspace_bytes(int n_frames, int n_pairs, int64_t total_kp, int64_t total_matches);
int gms_sfm_register_device(gms_ctx* ctx, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                            const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_matches, const gms_dmatch* d_filtered,
                            const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links,
                            void* d_ws, size_t ws_bytes, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_points_world,
                            int32_t* d_track, int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs,
                            int32_t* d_cloud_est, double* d_cloud_spread, gms_sfm_summary* d_summary);
int gms_sfm_register(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const double* points3d, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                     gms_sfm_pair_reg* reg, double* points_world, int32_t* track, int64_t cloud_cap, double* cloud, int32_t* cloud_id,
                     int32_t* cloud_obs, int32_t* cloud_est, double* cloud_spread, gms_sfm_summary* summary);

/* ---- one-to-one matches per pair, and the registration on them (the library's own; tests/match_unique_ref.py is
 * the definition in numpy) ---------------------------------------------------------------------------------------------------------
 * A nearest-neighbour matcher gives every keypoint of frame_a a match, so several may name one keypoint of frame_b, and the tracks
 * then chain two keypoints of one frame together. This stage keeps, per pair, a one-to-one subset of the matches.
 *   Match k of pair i is live when k < n_i (n_i as in the registration: clamp(tv.n_points, 0, m) when tv.status is GMS_OK, else 0),
 *   its mask byte is non-zero and both indices lie inside their frames. With null d_tv: n_i = m; with null d_mask: every byte counts
 *   as set. key(k) = (ord(distance) << 32) | k, ord(d) = the bit pattern of a finite d > 0, 0 for +0 and -0, 0xFFFFFFFF for anything
 *   else (negative, infinite, no number: last, ordered by k). A live match is kept when its key is the least among the live matches
 *   of its pair that share its trainIdx and the least among those that share its queryIdx. Everything else -- the losers, the
 *   matches that are not live, the slots in [n_i, m) -- gets 0. It is not a maximum matching: a match may lose on one side to a
 *   match that loses on the other, and then neither is kept. Integer minima only: the same bytes run after run.
 * gms_match_unique_device: writes d_keep (one uint8 per match slot) for [match_off, match_off + m) of every pair whose record fits
 *   the arrays (as in the registration; a pair that does not fit has nothing read or written and counts {0, 0}; other slots are not
 *   written), and d_counts (two int32 per pair: live, kept). Any pair list: a frame may be frame_a or frame_b of any number of pairs,
 *   and a pair of frames may appear more than once; the match ranges of different pairs do not overlap. d_mask and d_tv may be null
 *   (above). A null ctx, d_frame_off, d_ws, or (n_pairs > 0) d_pairs, d_counts, or (total_matches > 0) d_filtered, d_keep; max_m
 *   outside [0, 2^24); total_kp >= 2^31 - 1; a workspace that is not 256-byte aligned or too small: GMS_ERR_BAD_ARG, nothing run.
 *   Stream-ordered on the context's stream; no allocation, no synchronisation, no readback (graph-capturable); three launches.
 * gms_match_unique_workspace_bytes: 32 bytes per match slot (two open-addressing tables of 2 m keys per pair, laid out by match_off),
 *   rounded up to 256; at least 256. It does not grow with n_pairs or total_kp. 0: sizes refused.
 * gms_match_unique: the same on host arrays, synchronous, on the current HIP device; keep covers every slot below max(match_off + m)
 *   (what the device call leaves untouched is 0). mask and tv may be null. It refuses what gms_sfm_register refuses of the pair
 *   records and offsets: a frame index out of range, m < 0, match_off < 0 or beyond 2^40 - m, decreasing frame_off.
 * gms_sfm_register_keep_device / gms_sfm_register_keep: gms_sfm_register_device / gms_sfm_register with a keep plane (one uint8 per
 *   match slot, as above). A null d_keep / keep: the same bytes as those calls. With a plane, a match of the registration whose byte
 *   is 0 does not feed the tracks: it is no edge and no estimate, and d_track at its slot (match_off + rank) stays -1. d_track, the
 *   cloud arrays and the summary's n_tracks, n_points, n_multi follow the kept matches (n_points and d_cloud_est count kept
 *   estimates only). d_views, d_reg, d_points_world and the links do not read the plane: the same bytes as without it. When every ok
 *   pair's kept matches are one-to-one and the ok pairs form a tree over the frames -- gms_sfm_plan's always do -- no track holds two
 *   keypoints of a frame: n_multi = 0. With a caller's plan that is no tree, n_multi is still counted. */
size_t gms_match_unique_workspace_bytes(int n_pairs, int64_t total_kp, int64_t total_matches);
int gms_match_unique_device(gms_ctx* ctx, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs,
                            int max_m, int64_t total_matches, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_two_view* d_tv,
                            void* d_ws, size_t ws_bytes, uint8_t* d_keep, int32_t* d_counts);
int gms_match_unique(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                     const uint8_t* mask, const gms_two_view* tv, uint8_t* keep, int32_t* counts);
int gms_sfm_register_keep_device(gms_ctx* ctx, const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs,
                                 const gms_sfm_plan_entry* d_plan, int n_pairs, int max_m, int64_t total_matches, const gms_dmatch* d_filtered,
                                 const uint8_t* d_mask, const double* d_points3d, const gms_two_view* d_tv, int root, int min_links,
                                 void* d_ws, size_t ws_bytes, gms_sfm_view* d_views, gms_sfm_pair_reg* d_reg, double* d_points_world,
                                 int32_t* d_track, int64_t cloud_cap, double* d_cloud, int32_t* d_cloud_id, int32_t* d_cloud_obs,
                                 int32_t* d_cloud_est, double* d_cloud_spread, gms_sfm_summary* d_summary, const uint8_t* d_keep);
int gms_sfm_register_keep(const int64_t* frame_off, int n_frames, const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered,
                          const uint8_t* mask, const double* points3d, const gms_two_view* tv, int root, int min_links, gms_sfm_view* views,
                          gms_sfm_pair_reg* reg, double* points_world, int32_t* track, int64_t cloud_cap, double* cloud, int32_t* cloud_id,
                          int32_t* cloud_obs, int32_t* cloud_est, double* cloud_spread, gms_sfm_summary* summary, const uint8_t* keep);

/* ---- bundle adjustment behind the registration (the library's own; tests/sfm_ba_ref.py is the definition) --------
 * Refines the registered views and the cloud over all the keypoints a track chains together. Inputs: the keypoints, d_frame_off,
 * d_pairs, the survivors d_filtered and d_mask as the two-view stage took and left them, and d_views, d_reg, d_track, d_cloud,
 * d_cloud_id and d_reg_summary as gms_sfm_register_device left them (cloud_cap: the capacity of that call).
 *   Observations: a keypoint belongs to cloud entry c when a match of an ok pair (d_reg status GMS_OK) with a non-zero mask byte and
 *   both indices inside their frames names it and d_track at the match's slot (match_off + rank) is d_cloud_id[c], c below
 *   min(n_tracks, cloud_cap). Its measurement is cv::undistortPoints of its pt. A track with two keypoints of one frame, or with fewer
 *   than two observations, is excluded whole: its point comes back unchanged. Sums over a track's or a frame's observations run in
 *   ascending global keypoint index or in a tree fixed by the counts; no floating-point atomics: the same bytes run after run.
 *   retriangulate: X = (sum (I - d d^T))^-1 sum (I - d d^T) c over a track's rays first; taken when finite and in front of every
 *   camera that sees the track, otherwise the cloud's point stays (status 3). Residual r = f (pi(R X + t) - (u, v)), f = (fx + fy) / 2,
 *   inactive at z <= 0 or a non-finite camera point; Huber weights at huber_px (0: none). Parameters: (omega, tau) of every registered
 *   frame but the root (R <- exp([omega]x) R, t <- t + tau) and every used track's point. Levenberg-Marquardt with lambda diag
 *   damping, points eliminated, the reduced camera system by conjugate gradients preconditioned with its 6 x 6 diagonal blocks,
 *   Schur-implicit, at most n_cg iterations, done at r.z <= cg_tol^2 r0.z0. A step is accepted when the Huber cost falls and no
 *   observation turns inactive (lambda <- max(lambda / 10, 1e-12)), else dropped (lambda <- 10 lambda); done when an accepted step
 *   lowers the cost by no more than ftol cost. n_iters outer iterations are always launched (flags on the device turn the rest into
 *   no-ops). At the end (n_iters > 0) every t and every refined point is multiplied by one factor that puts the camera of the first ok
 *   pair without a link at distance 1 from the root. n_iters = 0: re-triangulation and the statistics alone.
 * Outputs: d_views_out (n_frames records; d_views is not written), d_cloud_out (3 doubles per cloud entry), d_track_status (int32 per
 *   cloud entry: 0 refined, 1 excluded: two keypoints of a frame, 2 excluded: fewer than two observations, 3 refined from its cloud
 *   point: re-triangulation was refused) and one gms_sfm_ba_summary. A null pointer, n_iters < 0, n_cg < 1, a negative or non-finite
 *   lambda0, cg_tol, ftol or huber_px, total_kp or cloud_cap >= 2^31 - 1, more than 2^24 frames, a workspace that is not 256-byte aligned or too small:
 *   GMS_ERR_BAD_ARG, nothing run. Stream-ordered on the context's stream; no allocation, no synchronisation, no readback
 *   (graph-capturable); 12 + n_iters (8 + 3 n_cg) launches.
 * gms_sfm_ba: the same on host arrays, synchronous, on the current HIP device; n_tracks: the registration summary's. A pair with
 *   m < 0, match_off < 0 or match_off > 2^40 - m (held so, before the sum is formed): GMS_ERR_BAD_ARG, nothing run. */
typedef struct gms_sfm_ba_params {
    double  lambda0, cg_tol, ftol, huber_px;   /* 1e-3, 1e-8, 1e-10, 2.0 */
    int32_t n_iters, n_cg, retriangulate;      /* 10, 50, 1              */
    int32_t reserved;
} gms_sfm_ba_params;
typedef struct gms_sfm_ba_summary {
    double  cost0, cost;          /* Huber cost in px^2 before (after re-triangulation) and after                  */
    double  rms0_px, rms_px;      /* unweighted, over the active observations                                      */
    double  lambda;               /* the damping the last iteration left                                           */
    int64_t n_obs, n_active;      /* observations of the used tracks; those active at the end                      */
    int64_t n_tracks_used, n_tracks_multi;
    int32_t n_frames_free;        /* registered frames other than the root                                         */
    int32_t iters_run, iters_accepted, cg_iters;
    int32_t status;               /* GMS_OK, or GMS_ERR_NO_MODEL when no observation is active                     */
    int32_t reserved;
} gms_sfm_ba_summary;
size_t gms_sfm_ba_workspace_bytes(int n_frames, int n_pairs, int64_t total_kp, int64_t cloud_cap);
int gms_sfm_ba_device(gms_ctx* ctx, const gms_camera* camera, const gms_sfm_ba_params* params, const gms_keypoint* d_kp,
                      const int64_t* d_frame_off, int n_frames, int64_t total_kp, const gms_pair* d_pairs, int n_pairs,
                      int64_t total_matches, const gms_dmatch* d_filtered, const uint8_t* d_mask, const gms_sfm_view* d_views,
                      const gms_sfm_pair_reg* d_reg, const int32_t* d_track, int64_t cloud_cap, const double* d_cloud,
                      const int32_t* d_cloud_id, const gms_sfm_summary* d_reg_summary, void* d_ws, size_t ws_bytes,
                      gms_sfm_view* d_views_out, double* d_cloud_out, int32_t* d_track_status, gms_sfm_ba_summary* d_summary);
int gms_sfm_ba(const gms_camera* camera, const gms_sfm_ba_params* params, const gms_keypoint* kp, const int64_t* frame_off, int n_frames,
               const gms_pair* pairs, int n_pairs, const gms_dmatch* filtered, const uint8_t* mask, const gms_sfm_view* views,
               const gms_sfm_pair_reg* reg, const int32_t* track, int64_t cloud_cap, const double* cloud, const int32_t* cloud_id,
               int64_t n_tracks, gms_sfm_view* views_out, double* cloud_out, int32_t* track_status, gms_sfm_ba_summary* summary);

/* ---- pair records from a view array (the library's own; tests/sfm_pair_pose_ref.py is the definition) -----------
 * The dense stage (gms_dense_pairs_device) and the fusion (gms_dense_fuse_device) read a pair's pose from gms_two_view.R/t/status and
 * its scale from gms_sfm_pair_reg.S/status when they run. This stage writes such records for ANY frame pairs of ANY view array --
 * gms_sfm_register_device's d_views or gms_sfm_ba_device's d_views_out --, so that the dense stages run on those poses, also for
 * pairs the sparse stage never matched. Stated in csrc/sfm_pair_pose_core.h: fp64, only + - * / sqrt, every sum in index order; the
 * GPU, a host build of the header and numpy agree byte for byte.
 *   For pair i with frames a = frame_a, b = frame_b (m and match_off are not read) and views x_cam = R x_world + t:
 *     R_ab[r][c] = sum_k R_b[r][k] R_a[c][k], T = t_b - R_ab t_a, S = sqrt(T0^2 + T1^2 + T2^2), t = T / S per component.
 *   GMS_OK when both indices are in 0..n_frames-1 (checked before a view's address is formed), a != b, both views are registered,
 *   every entry of R_ab and T is finite and S is finite and > 0; otherwise GMS_ERR_NO_MODEL.
 *   d_tv_out[i]: R = R_ab, t, status; d_reg_out[i]: S, status, link = -1; every other field of both records is 0, and a pair that
 *   is not ok has R, t and S zero as well. Every byte of both records is written. Fed the registration's own views, an ok pair's
 *   R, t and S come back up to rounding.
 * gms_sfm_pair_poses_device: one kernel, one lane per pair; stream-ordered on the context's stream; no allocation, no
 *   synchronisation, no readback (graph-capturable). n_pairs < 0 or above 2^30, n_frames < 1, or with n_pairs > 0 a NULL pointer or
 *   one that is not 8-byte aligned: GMS_ERR_BAD_ARG, nothing run. n_pairs = 0 succeeds and writes nothing.
 * gms_sfm_pair_poses: the same on host arrays, synchronous, on the current HIP device. */
int gms_sfm_pair_poses_device(gms_ctx* ctx, const gms_sfm_view* d_views, int n_frames, const gms_pair* d_pairs, int n_pairs,
                              gms_two_view* d_tv_out, gms_sfm_pair_reg* d_reg_out);
int gms_sfm_pair_poses(const gms_sfm_view* views, int n_frames, const gms_pair* pairs, int n_pairs, gms_two_view* tv_out,
                       gms_sfm_pair_reg* reg_out);

/* ---- ingest format -----------------------------------------------------------------------------------------
 * The reference keeps detector and matcher output in process (std::vector<cv::KeyPoint>, cv::Mat descriptors,
 * std::vector<cv::DMatch>: FeatureMatchUtil.cpp:9-12,58-68; DisparityUtil.cpp:108,137-143) and has no on-disk form. One
 * little-endian file ("GMSFRM01", layout in gms_io.cpp) carries a sequence in exactly the arrays the batch API takes --
 * cv::KeyPoint / cv::DMatch records verbatim -- so that a caller can dump its vectors and any process can filter them.
 * gms_dataset_read allocates one block (owner) that gms_dataset_free releases; on write, owner is ignored. Host only. */
typedef struct gms_dataset {
    int32_t n_frames, desc_kind;        /* desc_kind: GMS_DESC_NONE / _HAMMING256 / _L2_F32X128                    */
    int64_t n_pairs, total_matches;
    int32_t* wh;                        /* 2 * n_frames: (width, height)                                           */
    int64_t* frame_off;                 /* n_frames + 1 keypoint offsets; frame_off[n_frames] = number of keypoints */
    gms_keypoint* keypoints;
    void* descriptors;                  /* one row per keypoint (32 B or 128 floats), or NULL                      */
    gms_pair* pairs;                    /* match_off indexes `matches`                                             */
    gms_dmatch* matches;
    void* owner;
} gms_dataset;
int  gms_dataset_write(const char* path, const gms_dataset* d);
int  gms_dataset_read(const char* path, gms_dataset* d);
void gms_dataset_free(gms_dataset* d);

/* ---- introspection --------------------------------------------------------------------------- */
int         gms_max_matches(void);        /* largest m per pair this build accepts                 */
int         gms_last_hip_error(void);     /* last hipError_t seen by this thread's calls           */
/* ---- keypoint source ---------------------------------------------------------------------
 * Stands where the reference calls OpenCV's detectors (FeatureMatchUtil.cpp:9-12 SIFT::create(10000)->detectAndCompute;
 * DisparityUtil.cpp:108,123-138 ORB::create(), detectAndCompute / compute at every pixel). NOT cv::ORB: a FAST-9 + steered-BRIEF
 * detector of this library's own, in integer arithmetic (definition: DESIGN.md section 7b; CPU statement oracle/detect_ref.c).
 * What cv::ORB has and this has: FAST-9 corners, an intensity-centroid direction, 256 steered comparisons on a smoothed image and --
 * through gms_detect_pyramid_batch_device below -- a scale pyramid with size and octave per keypoint. What it still has not: Harris
 * ranking (the FAST score ranks), cv::ORB's learned pattern (the pattern is this library's own) and cv::resize's pyramid (the resize is
 * this library's own). The functions of this block are the single-scale form. Same records out: cv::KeyPoint {pt, size 31, angle = 11.25 * direction bin, response = FAST score, octave 0,
 * class_id -1} and one 32-byte row per keypoint for NORM_HAMMING -- what gms_normalize_device / gms_bf_prepare_device take.
 * Images: 8-bit grey, row-major, pitch = width, n_images of one size back to back in device memory. Keypoints sit at least
 * GMS_DETECT_BORDER pixels from every edge. */
#define GMS_DETECT_BORDER 16
size_t gms_detect_workspace_bytes(int width, int height, int n_images, int max_keypoints);

/* detectAndCompute for a batch: per image the max_keypoints strongest FAST-9 corners with score > threshold (equal scores in raster
 * order), written in raster order: d_keypoints[i * max_keypoints ..], d_descriptors[(i * max_keypoints ..) * 32], d_counts[i].
 * Errors: GMS_ERR_BAD_ARG (NULL, width/height outside (32, 65535], threshold outside [0, 254], workspace too small). */
int gms_detect_batch_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                            void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors, int32_t* d_counts);

/* Feature2D::compute on ONE image (DisparityUtil.cpp:123-133, a keypoint per pixel): direction (written to angle) and row at each
 * of the caller's n keypoints. A keypoint off the integer pixel grid or inside the border sets *d_status = 1 and keeps its row
 * (OpenCV would have dropped the keypoint and renumbered the rest; here the caller keeps control of the indices).
 * Workspace: gms_detect_workspace_bytes(width, height, 1, 0). */
int gms_describe_device(gms_ctx* ctx, const uint8_t* d_image, int width, int height, gms_keypoint* d_keypoints, int n,
                        void* d_workspace, size_t workspace_bytes, uint8_t* d_descriptors, int32_t* d_status);

/* ---- pyramid keypoint source (CPU statement tests/pyramid_ref.py) ------------------------------------
 * The detector above on every level of an image pyramid, as SIFT::create / ORB::create search one: keypoints come back in level-0
 * pixel coordinates with size and octave, so that matchGMS(withScale), matchLOGOS and a resized pair ("Change Scale", main.cpp:42-47)
 * get a scale from the keypoint source.
 *   levels   level 0 is the image; w_l = (5 w_{l-1} + 3) / 6, the same for h (a ratio of about 1.2, cv::ORB's). They end at n_levels
 *            (1 .. GMS_PYRAMID_MAX_LEVELS) or before the first level the detector refuses (width or height <= 32).
 *   resize   level l from level l - 1: bilinear with pixel centres aligned, 8-bit fixed-point weights, rounded to nearest, edges
 *            clamped -- integer arithmetic, this library's own definition (not cv::resize's).
 *   quotas   q_l = max_keypoints * w_l h_l / sum_j w_j h_j in 64-bit integers, the remainder to level 0. What a level does not use of
 *            its quota is not handed to another level (cv::ORB does not either).
 *   records  level 0 first, raster order inside a level. pt = ((x + 0.5) * f - 0.5) in fp32, each operation rounded once, with
 *            f = (float)w_0 / (float)w_l for x and (float)h_0 / (float)h_l for y; size = 31 * (float)w_0 / (float)w_l; octave = l; angle,
 *            response, class_id and the 32-byte row as the detector above gives them on the level's image.
 * n_levels = 1 gives the bytes of gms_detect_batch_device. */
#define GMS_PYRAMID_MAX_LEVELS 16
/* Host: the sizes of the levels actually used -> widths[], heights[] (room for n_levels each). Returns their number (>= 1), or
 * GMS_ERR_BAD_ARG (NULL, n_levels outside [1, 16], width/height outside (32, 65535]). */
int gms_pyramid_level_sizes(int width, int height, int n_levels, int32_t* widths, int32_t* heights);
size_t gms_detect_pyramid_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels);   /* 0: bad arguments */

/* detectAndCompute over the pyramid for a batch: image i's keypoints at d_keypoints[i * max_keypoints ..], its rows at
 * d_descriptors[(i * max_keypoints ..) * 32], d_counts[i] of them; d_level_counts[i * n_levels + l] come from level l (0 for a level
 * that is not used). On the context's stream; allocates nothing, waits for nothing, so it can be captured into a graph.
 * Errors: those of gms_detect_batch_device, and n_levels outside [1, GMS_PYRAMID_MAX_LEVELS]. */
int gms_detect_pyramid_batch_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int threshold, int max_keypoints,
                                    int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                    int32_t* d_counts, int32_t* d_level_counts);

/* The level images alone: levels 1, 2, .. of the batch into d_levels, level after level, the n_images images of a level back to back
 * (pitch = the level's width), nothing between them: n_images * sum_{l >= 1} w_l h_l bytes. levels_bytes: room in d_levels. */
int gms_pyramid_build_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int n_levels, uint8_t* d_levels,
                             size_t levels_bytes);

/* ---- gradient descriptor: SIFT-format rows from the pyramid keypoint source (CPU statement
 * tests/grad_desc_ref.py) -------------------------------------------------------------------------------------------------------
 * Where the reference gets keypoints it gets 128-float SIFT rows with them (FeatureMatchUtil.cpp:9-12, DisparityUtil.cpp:101-133). These
 * calls make rows of that structure and format at the detector's keypoints: 4 x 4 cells x 8 orientations of weighted gradient
 * magnitude on the keypoint's own pyramid level, in the frame of its direction, normalised, clipped at 0.2, normalised again and
 * scaled by 512: 128 fp32 values per keypoint, each an integer 0..255 -- what gms_bf_prepare_device(GMS_DESC_L2_F32X128) sends to its
 * exact int8 path. NOT cv::SIFT: this library's own definition in integer arithmetic (no equality with OpenCV's rows; the DoG detector for them is
 * gms_detect_dog_batch_device below),
 * so the rows are the same bytes on every run and equal the CPU statement.
 *
 * gms_detect_pyramid_grad_batch_device: gms_detect_pyramid_batch_device with one output more. Keypoints, 32-byte rows, counts and level
 * counts are the bytes that call writes; image i's 128-float rows go to d_rows128[(i * max_keypoints ..) * 128] (8-byte aligned), in the
 * keypoints' order. n_levels = 1 is the single-scale form. Same stream rule (nothing allocated, nothing waited for: can be captured) and
 * same errors; the workspace has its own size function. */
size_t gms_detect_pyramid_grad_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels);   /* 0: bad arguments */
int gms_detect_pyramid_grad_batch_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int threshold,
                                         int max_keypoints, int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints,
                                         uint8_t* d_descriptors, int32_t* d_counts, int32_t* d_level_counts, float* d_rows128);

/* Feature2D::compute with these rows on ONE image, the counterpart of gms_describe_device: direction (written to angle) and the
 * 128-float row at each of the caller's n keypoints, on the image itself (level 0). The same status rule: a keypoint off the integer
 * pixel grid or inside the border sets *d_status = 1 and keeps its row. Workspace: gms_detect_workspace_bytes(width, height, 1, 0). */
int gms_describe_grad_device(gms_ctx* ctx, const uint8_t* d_image, int width, int height, gms_keypoint* d_keypoints, int n,
                             void* d_workspace, size_t workspace_bytes, float* d_rows128, int32_t* d_status);

/* ---- difference-of-Gaussians (DoG) detector on the pyramid (CPU statement tests/dog_ref.py) ----------------
 * The reference's keypoints are SIFT's: DoG blobs (FeatureMatchUtil.cpp:9-12, DisparityUtil.cpp:101-120,232). This call puts a DoG
 * detector in the place of the FAST-9 corner detector of gms_detect_pyramid_(grad_)batch_device: a corner is found on every level on
 * which it still is a corner, a DoG extremum picks the level on which the structure has its size -- the `size` that matchGMS(withScale)
 * and LOGOS read. On every pyramid level: four integer Gaussian blurs (sigma 1.217 .. 2.103, taps that sum to 4096), three layers
 * D_k = B_{k+1} - B_k in 1/256 grey level, a candidate where |D_1| > contrast, D_1 is strictly above or strictly below its 26 neighbours
 * and the Hessian of D_1 passes SIFT's edge test (r = 10); score = clamp(|D_1| >> 4, 1, 255). Selection (strongest q_l per level, equal
 * scores in raster order), records (pt in level-0 coordinates, size = 31 f, octave = level, angle = the centroid direction, response =
 * score), 32-byte rows and 128-float rows are those of the calls above, unchanged. All integer: the same bytes on every run, equal to
 * the CPU statement. NOT cv::SIFT: no sub-pixel or sub-scale refinement (gms_detect_dog_refined_batch_device below has one step of it); one layer per level, so a blob is usually reported on two
 * neighbouring levels; the direction is the intensity centroid's, not a gradient histogram's.
 *
 * contrast in [0, GMS_DOG_MAX_CONTRAST], in 1/256 grey level (128 = half a grey level). d_rows128 may be NULL (no 128-float rows; else
 * 8-byte aligned). Everything else -- outputs, stream rule (nothing allocated, nothing waited for: can be captured), errors -- as
 * gms_detect_pyramid_grad_batch_device. */
#define GMS_DOG_MAX_CONTRAST 65535
size_t gms_detect_dog_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels);   /* 0: bad arguments */
int gms_detect_dog_batch_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int contrast, int max_keypoints,
                                int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints, uint8_t* d_descriptors,
                                int32_t* d_counts, int32_t* d_level_counts, float* d_rows128 /* may be NULL */);
/* The candidate planes alone, single level: d_cand[n_images][height][width] = the score (1..255) where the image has a DoG candidate,
 * else 0 -- before any selection. */
int gms_dog_candidates_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int contrast, uint8_t* d_cand);

/* The same detector with one refinement step (CPU statement tests/dog_refine_ref.py): after selection -- same
 * candidates, same quotas, same order -- every keypoint is moved to 1/16 pixel of its level by the Newton step -H^-1 g on D_1 and to
 * 1/16 layer by the parabola through D_0, D_1, D_2, all in int64 with floor divisions; an offset beyond half a pixel is clamped to
 * it (SIFT re-centres and refits; this does not). With ox, oy, os the offsets in sixteenths (-8 .. 8), fx = width / level width:
 *   x = ((x_level + ox / 16) + 0.5) * fx - 0.5, y likewise, size = (31 * fx) * 1.2^(os / 16) (17 fp32 constants),
 * each operation rounded once in fp32. angle, response, octave, class_id, the 32-byte rows, the 128-float rows, counts and level
 * counts are the bytes gms_detect_dog_batch_device writes; a keypoint whose three offsets are zero has that call's record.
 * Arguments, checks, outputs and stream rule (nothing allocated, nothing waited for: can be captured) as gms_detect_dog_batch_device;
 * the workspace is larger by one uint16 plane of offsets per image. */
size_t gms_detect_dog_refined_workspace_bytes(int width, int height, int n_images, int max_keypoints, int n_levels);   /* 0: bad arguments */
int gms_detect_dog_refined_batch_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int contrast,
                                        int max_keypoints, int n_levels, void* d_workspace, size_t workspace_bytes, gms_keypoint* d_keypoints,
                                        uint8_t* d_descriptors, int32_t* d_counts, int32_t* d_level_counts, float* d_rows128 /* may be NULL */);
/* The offset planes alone, single level, the counterpart of gms_dog_candidates_device: d_codes[n_images][height][width] =
 * 1 + (ox + 8) + 17 (oy + 8) + 289 (os + 8) where the image has a DoG candidate, else 0. */
int gms_dog_offsets_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int contrast, uint16_t* d_codes);

/* ---- from photographs to the tables ---------------------------------------------------------------------
 * The reference hands BGR Mats to every entry point (main.cpp:21-75) and gets one keypoint vector per image back from
 * detectAndCompute; the detector above takes grey planes and leaves [n, max_keypoints] blocks, the tables (gms_normalize_device,
 * gms_bf_prepare_device, gms_logos_prepare_device, gms_two_view_batch_device) take all frames back to back with an offset per frame.
 * These two calls stand between them, so that neither pixels nor keypoints nor rows pass through the host. Both run on the context's
 * stream, allocate nothing and wait for nothing, so they can be captured into a graph.
 *
 * gms_bgr_to_gray_device: n_images of height x width x 3 bytes, B, G, R interleaved (a CV_8UC3 Mat without padding), back to back ->
 * n_images grey planes, pitch = width, back to back: grey = (299 R + 587 G + 114 B + 500) / 1000 in integer arithmetic (the weights of
 * cv::cvtColor's BGR2GRAY; not its fixed-point rounding). Either buffer may start at any byte address.
 * Errors: GMS_ERR_BAD_ARG (NULL, n_images < 0, width/height outside (0, 65535]). */
int gms_bgr_to_gray_device(gms_ctx* ctx, const uint8_t* d_bgr, int n_images, int width, int height, uint8_t* d_gray);

/* gms_detect_pack_device: the detector's blocks -> frames back to back. d_frame_off[0] = 0, d_frame_off[i + 1] = d_frame_off[i] +
 * min(d_counts[i], max_keypoints) (a negative count counts as 0); record and row j of image i go from slot i * max_keypoints + j of
 * the blocks to slot d_frame_off[i] + j of d_keypoints / d_rows32 / d_rows128, in their order. d_rows32_blocks with d_rows32, and
 * d_rows128_blocks with d_rows128, may be NULL together (rows the detector did not make). The outputs have room for n_images *
 * max_keypoints slots; what lies behind slot d_frame_off[n_images] is left as it was. d_frame_off: n_images + 1 values.
 * Errors: GMS_ERR_BAD_ARG (NULL, n_images outside [1, 65535], max_keypoints < 0, a row pointer without its partner, a pointer that
 * is not 4-byte aligned). 16-byte aligned buffers are moved with 16-byte accesses. */
int gms_detect_pack_device(gms_ctx* ctx, const gms_keypoint* d_keypoint_blocks, const uint8_t* d_rows32_blocks, const float* d_rows128_blocks,
                           const int32_t* d_counts, int n_images, int max_keypoints, gms_keypoint* d_keypoints, uint8_t* d_rows32,
                           float* d_rows128, int64_t* d_frame_off);

/* ---- LOGOS match filter -----------------------------------------------------------------------
 * cv::xfeatures2d::matchLOGOS(keypoints1, keypoints2, nn1, nn2, matches1to2) (FeatureMatchUtil.cpp:86-131; DESIGN.md, LOGOS):
 * candidates are the pairs (i, j) with nn1[i] == nn2[j]; a candidate survives if it has local support among the five nearest
 * neighbours of i and of j, and its relative orientation lies within 0.1 rad of the peak of the supported candidates' histogram.
 * Reads pt, size and angle of each keypoint. Output: (queryIdx = i, trainIdx = j, imgIdx = -1, distance = 0), i ascending, then j.
 * Host pointers; synchronous; uses the current HIP device. out_cap: room in `out`. *n_out: the number of survivors -- also when
 * that exceeds out_cap, in which case nothing is written and GMS_ERR_CAPACITY is returned. result may be NULL.
 * Neighbours at equal distances are taken in the order the reference's (unstable) std::sort leaves them in, restated in
 * logos_core.h. Frames of 1..5 keypoints use the neighbours there are (the reference reads past its list there).
 * Keypoint domain (every LOGOS entry point): pt.x, pt.y and angle finite, |angle| <= 3600 degrees; size is not restricted (0,
 * negative, NaN and inf give a log scale that fails every comparison, as in the reference). Outside the domain the reference's
 * orientation wrap does not terminate. gms_logos_match checks both frames on the host before any allocation or copy: it returns
 * GMS_ERR_DOMAIN with *n_out = 0 and result->status = GMS_ERR_DOMAIN, and writes nothing to `out`. */
typedef struct gms_logos_result {
    int64_t n_candidates; /* pairs with equal labels                                   */
    int64_t n_supported;  /* candidates with local support                             */
    int64_t n_out;        /* survivors (the needed count on overflow)                  */
    int32_t peak_bin;     /* 0..188, -1 when no candidate had support                  */
    int32_t status;       /* GMS_OK, GMS_ERR_CAPACITY or GMS_ERR_DOMAIN (batched path also: _BAD_ARG) */
} gms_logos_result;

int gms_logos_match(const gms_keypoint* kp1, int n1, const gms_keypoint* kp2, int n2, const int32_t* nn1, const int32_t* nn2,
                    gms_dmatch* out, int64_t out_cap, int64_t* n_out, gms_logos_result* result);

/* ---- LOGOS on resident frames (throughput API) ----------------------------------------------------------------
 * The same filter for many pairs of resident frames, with everything per frame worked out once. Device pointers on the context's
 * device, stream-ordered on the context's stream; these calls neither allocate nor synchronise nor read anything back, so they can
 * be captured into a hipGraph. Every buffer comes from the caller, sized by the two *_bytes functions.
 *
 * gms_logos_prepare_device: the frame table d_table (gms_logos_table_bytes(total_kp, n_frames, n_words) bytes, 16-byte aligned,
 *   opaque) for the keypoints d_kp of n_frames frames (d_frame_off: n_frames + 1 offsets) and one word per keypoint, d_words,
 *   in [0, n_words): the LOGOS point of each keypoint, its five nearest neighbours in its frame (ties at the fifth place in the
 *   order of the reference's sort, as gms_logos_match), and per frame its keypoints sorted by word (stable) with bucket offsets.
 *   A word outside [0, n_words), or a keypoint outside the keypoint domain stated at gms_logos_match, marks its frame: pairs that
 *   touch it, in either role, get GMS_ERR_DOMAIN and none of their queries is run. The workspace holds the slices of the tie
 *   pass: with fewer than gms_logos_workspace_bytes(largest frame, 0, 0) bytes, a frame whose ties do not fit is marked and its
 *   pairs get GMS_ERR_BAD_ARG.
 * gms_logos_filter_device: n_pairs pairs of the table's frames. For a gms_pair here, m is the pair's OUTPUT CAPACITY and match_off
 *   where its survivors start in d_out; ranges must be disjoint, as for gms_filter_device. Survivors are written as gms_logos_match
 *   writes them, (i, j, -1, 0), i then j ascending, byte for byte the same. d_logos_results gets one record per pair (as
 *   gms_logos_match reports it); when the survivors do not fit in m nothing of the pair is written, its status is GMS_ERR_CAPACITY and
 *   n_out the count needed. A frame index out of range or m < 0: GMS_ERR_BAD_ARG. d_pair_results (optional, NULL allowed) gets
 *   gms_pair_result records {n_inliers = survivors written, -1, -1, status}, so that gms_two_view_batch_device and
 *   gms_disparity_batch_device take the output as it is. The workspace needs gms_logos_workspace_bytes(0, n_pairs, largest query
 *   frame) bytes; pairs whose queries do not fit in it get GMS_ERR_BAD_ARG.
 * gms_logos_workspace_bytes(max_frame_kp, n_pairs, max_query_kp): enough for both calls.
 * gms_logos_words_device: the visual word of each of total_desc descriptor rows: the index of its EXACT nearest row of d_dict
 *   (n_words rows, 1 <= n_words <= 65535; lowest index on ties), where the reference's FLANN lookup is approximate.
 *     GMS_DESC_L2_F32X128  fp32 rows of 128; squared distance accumulated in fp32 in flann::L2's order: per group of four
 *                          dimensions ((d0*d0 + d1*d1) + d2*d2) + d3*d3, groups added to the running sum in order, no FMA. A NaN
 *                          distance counts as +inf.
 *     GMS_DESC_HAMMING256  rows of 32 bytes; popcount of the xor.
 * gms_logos_host_batch: prepare + filter on host arrays, synchronous (the C++ shim's batch form); pairs / out / results as for
 *   gms_logos_filter_device, in host memory. The keypoint domain is checked per frame by its prepare step, on the device: the
 *   call returns GMS_OK and the pairs of a frame outside the domain carry GMS_ERR_DOMAIN in their records. */
int64_t gms_logos_table_bytes(int64_t total_kp, int n_frames, int n_words);
size_t  gms_logos_workspace_bytes(int64_t max_frame_kp, int n_pairs, int64_t max_query_kp);
int gms_logos_prepare_device(gms_ctx* ctx, const gms_keypoint* d_kp, const int64_t* d_frame_off, int n_frames, int64_t total_kp,
                             const int32_t* d_words, int n_words, void* d_workspace, size_t ws_bytes, void* d_table);
int gms_logos_filter_device(gms_ctx* ctx, const void* d_table, const gms_pair* d_pairs, int n_pairs, void* d_workspace, size_t ws_bytes,
                            gms_dmatch* d_out, gms_logos_result* d_logos_results, gms_pair_result* d_pair_results);
int gms_logos_words_device(gms_ctx* ctx, int desc_kind, const void* d_desc, int64_t total_desc, const void* d_dict, int n_words,
                           int32_t* d_words);
int gms_logos_host_batch(gms_ctx* ctx, const gms_keypoint* kp, const int64_t* frame_off, int n_frames, const int32_t* words, int n_words,
                         const gms_pair* pairs, int n_pairs, gms_dmatch* out, gms_logos_result* results);

/* ---- Training the LOGOS dictionary ("Training the dictionary") -----------------------------------------------------
 * The reference builds its dictionary with BOWKMeansTrainer(50 | 100).cluster(desc1) (FeatureMatchUtil.cpp:100-104). cv::kmeans
 * seeds from a global RNG and sums in float, so its rows cannot be reproduced; the definition here is this library's own, and every
 * order-dependent step of it is integer arithmetic: the result is, byte for byte, that of the numpy statement
 * tests/logos_dict_ref.py, on every run. It is k-means with k-means++ seeding (three trials per centre), `attempts` restarts and at
 * most `max_iters` assignments, on the distances of gms_logos_words_device.
 *
 * A training set is a run of descriptor rows: set s is rows [d_set_off[s], d_set_off[s + 1]) of d_desc (n_sets + 1 offsets within
 * [0, total_rows], never decreasing). desc_kind: GMS_DESC_L2_F32X128 or GMS_DESC_HAMMING256. n_words 1..65535, attempts 1..16,
 * max_iters 1..1000, n_sets 0..65535 (others: GMS_ERR_BAD_ARG for the call, nothing run). Per set:
 *   d_dict     n_words rows per set, set after set; zero-filled for a set whose status is not GMS_OK.
 *   d_results  one record per set. status: GMS_ERR_BAD_ARG for a set with fewer than n_words rows, more than 2^20 rows or unusable
 *              offsets (negative, past total_rows, end before start, or a start before the end of an earlier set with usable
 *              offsets: sets that run never overlap); GMS_ERR_DOMAIN for an L2 set with an element that is not finite or outside [-4096, 4096]. Such a set
 *              does not disturb the others. attempt: the attempt with the smallest compactness (lowest index on ties), -1 on
 *              failure; iterations: the assignments it ran; compactness: the sum of the integer weights of its last assignment
 *              (a Hamming distance is its own weight, an L2 squared distance d weighs floor(d 2^8)); empty_clusters: dictionary
 *              rows that no row of the set is nearest to.
 *   d_labels   optional (NULL allowed), one int32 per row of d_desc: the word of every row of every set under its dictionary
 *              (what gms_logos_words_device gives for it), -1 for the rows of a failed set; rows outside every set, and those of a set with unusable
 *              offsets, are left alone.
 * gms_logos_dict_train_device: stream-ordered on the context's stream; no allocation, synchronisation or read-back; capturable.
 *   The workspace (16-byte aligned) needs gms_logos_dict_workspace_bytes(...) bytes for the same arguments; 0 means they are refused.
 * gms_logos_dict_train: the same on host arrays, synchronous, on device 0. */
typedef struct gms_logos_dict_result {
    int32_t  status;
    int32_t  attempt;
    int32_t  iterations;
    int32_t  empty_clusters;
    uint64_t compactness;
} gms_logos_dict_result;

size_t gms_logos_dict_workspace_bytes(int desc_kind, int64_t total_rows, int n_sets, int n_words, int attempts, int max_iters);
int gms_logos_dict_train_device(gms_ctx* ctx, int desc_kind, const void* d_desc, const int64_t* d_set_off, int n_sets, int64_t total_rows,
                                int n_words, int attempts, int max_iters, uint64_t seed, void* d_workspace, size_t ws_bytes, void* d_dict,
                                gms_logos_dict_result* d_results, int32_t* d_labels);
int gms_logos_dict_train(int desc_kind, const void* desc, const int64_t* set_off, int n_sets, int n_words, int attempts, int max_iters,
                         uint64_t seed, void* dict, gms_logos_dict_result* results, int32_t* labels);

/* ---- StereoBM block matching: the reference's dense baseline (DisparityUtil.cpp:22-49) -------------------------------
 *     StereoBM::create(16, 5); setNumDisparities(224); ...; compute(g1, g2, disparity);            CV_16S, 4 fractional bits
 *     normalize(disparity, disparity, 0, 255, NORM_MINMAX, CV_8U); every 0 pixel -> 255
 * OpenCV 4.5.2's integer path, restated (tests/stereo_bm_ref.py): XSOBEL pre-filter, blockSize^2 SADs for numDisparities disparities,
 * texture and uniqueness tests, the subpixel step, the left-right check (validateDisparity, disp12_max_diff >= 0) and FILTERED =
 * (min_disparity - 1) * 16 outside the valid ROI. Equal costs go to the largest disparity. Accepted (others: GMS_ERR_BAD_ARG):
 * pre_filter_type XSOBEL, pre_filter_size odd in 5..255 (unused by XSOBEL), pre_filter_cap 1..63, block_size odd in 5..51,
 * num_disparities a positive multiple of 16 up to 512, min_disparity >= -2047 with min_disparity + num_disparities <= 2048,
 * texture_threshold >= 0, uniqueness_ratio 0..1000, speckle_window_size 0 (speckle_range is then unused), width 1..8192 and
 * block_size < min(width, height).
 * Images: 8-bit grey, row y of image i at d_left / d_right + (i * height + y) * pitch (pitch >= width). Maps: int16 [n][height][width];
 * costs (optional): int32 [n][height][width], sad[best] where the winner-take-all step gave a disparity, -1 elsewhere. */
#define GMS_STEREO_BM_PREFILTER_NORMALIZED_RESPONSE 0
#define GMS_STEREO_BM_PREFILTER_XSOBEL              1
#define GMS_STEREO_BM_MAX_WIDTH                  8192
typedef struct gms_stereo_bm_params {
    int32_t block_size;          /* SADWindowSize                          */
    int32_t num_disparities;
    int32_t min_disparity;
    int32_t pre_filter_type;     /* GMS_STEREO_BM_PREFILTER_XSOBEL only    */
    int32_t pre_filter_size;
    int32_t pre_filter_cap;
    int32_t texture_threshold;
    int32_t uniqueness_ratio;
    int32_t speckle_window_size; /* 0 only                                 */
    int32_t speckle_range;
    int32_t disp12_max_diff;     /* < 0: no left-right check               */
} gms_stereo_bm_params;
/* The reference's values (DisparityUtil.cpp:24-36): gms_stereo_bm_params p = GMS_STEREO_BM_PARAMS_REFERENCE; a NULL params pointer
 * means the same. */
#define GMS_STEREO_BM_PARAMS_REFERENCE {5, 224, -39, GMS_STEREO_BM_PREFILTER_XSOBEL, 5, 61, 507, 0, 0, 8, 1}

/* gms_stereo_bm_workspace_bytes: the workspace of gms_stereo_bm_device (256-byte aligned pointer); 0 for arguments it rejects.
 * gms_stereo_bm_device: n_pairs (up to 65535) pairs on the context's stream; no allocation, no synchronisation, no readback
 *   (graph-capturable). d_cost may be NULL.
 * gms_stereo_bm_normalize_device: the reference's 8-bit map of each of n int16 maps (d_out8: n * width * height bytes).
 * gms_stereo_bm: ONE pair on host pointers, synchronous, on the current HIP device; disp16 / cost / disp8 (the reference's 8-bit map)
 *   are each optional. */
size_t gms_stereo_bm_workspace_bytes(int width, int height, int n_pairs, const gms_stereo_bm_params* params);
int gms_stereo_bm_device(gms_ctx* ctx, const gms_stereo_bm_params* params, const uint8_t* d_left, const uint8_t* d_right, int n_pairs,
                         int width, int height, int pitch, void* d_ws, size_t ws_bytes, int16_t* d_disp16, int32_t* d_cost);
int gms_stereo_bm_normalize_device(gms_ctx* ctx, const int16_t* d_disp16, int n, int width, int height, uint8_t* d_out8);
int gms_stereo_bm(const gms_stereo_bm_params* params, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                  int16_t* disp16, int32_t* cost, uint8_t* disp8);

/* ---- Semi-global matching on StereoBM's costs (tests/stereo_sgm_ref.py states it) ---------------------------------
 * The library's own definition, NOT cv::StereoSGBM: no Birchfield-Tomasi cost, no OpenCV source restated. The matching cost
 * C[y][x][k] is StereoBM's window SAD after its XSOBEL pre-filter, over the region StereoBM computes (rows [w2, H - w2), its output
 * columns), k meaning disparity num_disparities - 1 + min_disparity - k. Along each of n_paths directions (dy, dx) = (0,1), (0,-1),
 * (1,0), (-1,0), then (1,1), (1,-1), (-1,1), (-1,-1), a pixel whose predecessor (y - dy, x - dx) lies outside the region has L = C, every
 * other pixel L[k] = C[k] + min(Lp[k], Lp[k-1] + p1, Lp[k+1] + p1, m + p2) - m with m = min Lp (terms with k +- 1 outside the range left
 * out). S is the sum of L over the paths. StereoBM's rules then run on S in place of its SADs: the winner (the lowest k on ties), the
 * texture rule on StereoBM's texture sum, the uniqueness rule, the subpixel step, the left-right check and the ROI fill. Outputs as
 * gms_stereo_bm_device's: int16 maps with 4 fractional bits, FILTERED = (min_disparity - 1) * 16; costs S[winner], -1 elsewhere.
 * With p1 = p2 = 0 and uniqueness_ratio = 0 the map is StereoBM's and the cost n_paths times StereoBM's.
 * Accepted (others: GMS_ERR_BAD_ARG): what gms_stereo_bm_device accepts for bm, 0 <= p1 <= p2, n_paths 4 or 8, and
 * n_paths * (block_size^2 * 2 * pre_filter_cap + p2) <= 65535 (every path cost and their sum fit 16 unsigned bits). */
typedef struct gms_stereo_sgm_params {
    gms_stereo_bm_params bm;
    int32_t p1;                  /* penalty of a disparity step of one      */
    int32_t p2;                  /* penalty of a larger step                */
    int32_t n_paths;             /* 4 or 8                                  */
} gms_stereo_sgm_params;
/* The reference's StereoBM values, p1 = 8 * block_size^2, p2 = 32 * block_size^2, eight paths; a NULL params pointer means the same. */
#define GMS_STEREO_SGM_PARAMS_REFERENCE {GMS_STEREO_BM_PARAMS_REFERENCE, 200, 800, 8}

/* gms_stereo_sgm_workspace_bytes: the workspace of gms_stereo_sgm_device (256-byte aligned pointer): StereoBM's regions, the texture
 *   sums and the two 16-bit volumes C and S, 4 * num_disparities bytes per pixel of the region; 0 for arguments it rejects and for a
 *   size beyond size_t.
 * gms_stereo_sgm_device: n_pairs (up to 65535) pairs on the context's stream, arguments as gms_stereo_bm_device's; no allocation, no
 *   synchronisation, no readback (graph-capturable). d_cost may be NULL. gms_stereo_bm_normalize_device gives the 8-bit maps.
 * gms_stereo_sgm: ONE pair on host pointers, synchronous, on the current HIP device; disp16 / cost / disp8 are each optional. */
size_t gms_stereo_sgm_workspace_bytes(int width, int height, int n_pairs, const gms_stereo_sgm_params* params);
int gms_stereo_sgm_device(gms_ctx* ctx, const gms_stereo_sgm_params* params, const uint8_t* d_left, const uint8_t* d_right, int n_pairs,
                          int width, int height, int pitch, void* d_ws, size_t ws_bytes, int16_t* d_disp16, int32_t* d_cost);
int gms_stereo_sgm(const gms_stereo_sgm_params* params, const uint8_t* left, const uint8_t* right, int width, int height, int pitch,
                   int16_t* disp16, int32_t* cost, uint8_t* disp8);

/* ---- Portrait mode: the image tail of the reference's createPortraitMode (DisparityUtil.cpp:317-412) -----------------
 *     disparity 255 -> 0; threshold(60); dilate(3 x 3, 2 iterations, BORDER_REPLICATE); findContours(RETR_LIST, CHAIN_APPROX_NONE);
 *     the 5 borders of largest |contourArea|, drawContours(FILLED); medianBlur(image, 15); the photograph's own pixels back where a
 *     filled border covers them, except in the last three rows and columns
 * restated in tests/portrait_ref.py (OpenCV parity is unpinned; the choices are in DESIGN.md §4.9). Borders: Suzuki-Abe, set pixels
 * 8-connected, every outer and every hole border; ranked by the doubled shoelace area of the chain, equal areas by the raster order of
 * the border's start pixel, outer before hole (this project's rule, not the reference's); fewer than num_contours borders = all of
 * them. A border's fill is its chain and what the chain encloses, even-odd. The median is the exact (ksize^2 / 2)-th smallest per
 * channel, border replicated.
 * Accepted (others: GMS_ERR_BAD_ARG): threshold 0..255, dilate_iterations 0..8, num_contours 1..64, median_ksize odd in 3..31, width
 * and height 1..8192 (smaller than the window is legal), n 1..65535.
 * Images: 8-bit BGR, pixel (x, y) of image i at d_bgr + (i * height + y) * pitch_bgr + 3 x (pitch_bgr >= 3 width); disparity maps:
 * 8-bit, 255 = no value, row y of map i at d_disparity + (i * height + y) * pitch_disp (pitch_disp >= width). Outputs are dense:
 * d_out_bgr and d_blurred [n][height][width][3]; d_mask (the dilated mask, 0 / 255) and d_selected (255 where a chosen border's fill
 * covers the pixel, else 0) [n][height][width]. */
#define GMS_PORTRAIT_MAX_SIDE 8192
#define GMS_PORTRAIT_STAGES   9
typedef struct gms_portrait_params {
    int32_t threshold;
    int32_t dilate_iterations;
    int32_t num_contours;
    int32_t median_ksize;
} gms_portrait_params;
/* The reference's values (DisparityUtil.cpp:341, :351, :380, :394); a NULL params pointer means the same. */
#define GMS_PORTRAIT_PARAMS_REFERENCE {60, 2, 5, 15}

/* gms_portrait_workspace_bytes: the workspace of gms_portrait_device (256-byte aligned pointer); 0 for arguments it rejects. With
 *   px = n * width * height and up(x) = x rounded up to 256: 4 up(px) + up(4 px) + up(8 px) + up(8 n height ((width + 1) / 2)) +
 *   up(264 n) bytes (mask, neighbour codes, frame flags and selection, a byte each; labels, int32; even-odd toggles, one bit per
 *   chosen border; one 64-bit rank key per border; the chosen borders).
 * gms_portrait_device: n images on the context's stream; no allocation, no synchronisation, no readback (graph-capturable). d_mask,
 *   d_selected and d_blurred may each be NULL; without d_blurred the blurred image never goes to memory on its own. Cost: every
 *   border is walked by one lane, a dependent byte load per step, so the call's time grows with the longest chain; a ragged mask
 *   that is one component can have a chain of the order of the pixel count (measured figures: DESIGN.md §4.9).
 * gms_portrait_profile_device: a diagnostic, NOT capturable: the same launches with a device event between them, then a
 *   synchronisation; stage_ms (host, GMS_PORTRAIT_STAGES floats) receives the time of each kernel in launch order: mask, init, merge,
 *   flatten, area, select, trace, fill, median. tools/portrait_bench.py reads its per-kernel times here.
 * gms_median_blur_device: medianBlur of n images of 1 or 3 interleaved channels; source and destination rows both `pitch` bytes
 *   apart (pitch >= channels * width), image i at i * height * pitch. d_dst must not overlap d_src (tiles read their neighbours'
 *   pixels while others write): overlapping ranges are GMS_ERR_BAD_ARG.
 * gms_median_blur: ONE image on host pointers (dense rows), synchronous, on the current HIP device.
 * gms_portrait: ONE image on host pointers (dense rows), synchronous, on the current HIP device; mask / selected / blurred optional. */
size_t gms_portrait_workspace_bytes(int width, int height, int n, const gms_portrait_params* params);
int gms_portrait_device(gms_ctx* ctx, const gms_portrait_params* params, const uint8_t* d_bgr, const uint8_t* d_disparity, int n,
                        int width, int height, int pitch_bgr, int pitch_disp, void* d_ws, size_t ws_bytes, uint8_t* d_out_bgr,
                        uint8_t* d_mask, uint8_t* d_selected, uint8_t* d_blurred);
int gms_median_blur_device(gms_ctx* ctx, const uint8_t* d_src, int n, int width, int height, int channels, int pitch, int ksize,
                           uint8_t* d_dst);
int gms_portrait_profile_device(gms_ctx* ctx, const gms_portrait_params* params, const uint8_t* d_bgr, const uint8_t* d_disparity, int n,
                                int width, int height, int pitch_bgr, int pitch_disp, void* d_ws, size_t ws_bytes, uint8_t* d_out_bgr,
                                uint8_t* d_mask, uint8_t* d_selected, uint8_t* d_blurred, float* stage_ms);
int gms_median_blur(const uint8_t* src, int width, int height, int channels, int ksize, uint8_t* dst);
int gms_portrait(const gms_portrait_params* params, const uint8_t* bgr, const uint8_t* disparity, int width, int height,
                 uint8_t* out_bgr, uint8_t* mask, uint8_t* selected, uint8_t* blurred);

/* ---- cv::resize and cv::warpAffine, the reference main()'s image transforms (main.cpp:36, :44, :114-120) -------------
 * 8-bit images of 1 or 3 interleaved channels. Both are OpenCV 4.5.2's 8-bit INTER_LINEAR paths restated as integer arithmetic in
 * tests/warp_ref.py and csrc/warp_core.h (parity with an OpenCV build is unpinned; DESIGN.md §4.11 has the statement):
 *   resize: 11-bit column and row weights from float32 fractions; when both axes halve exactly, the 2 x 2 mean (a+b+c+d+2)>>2.
 *   warpAffine: the FORWARD 2 x 3 matrix (source -> destination, row-major doubles), inverted as OpenCV inverts it; source positions
 *     with 5 fractional bits; BORDER_CONSTANT 0: a tap outside the source is 0; every destination pixel is written. Non-finite
 *     entries, or ones whose positions overflow int32, are outside the domain: the result is then unspecified, but nothing outside
 *     the source is read.
 * Accepted (others: GMS_ERR_BAD_ARG): channels 1 or 3; every side 1..GMS_WARP_MAX_SIDE; n 1..65535; src_pitch >= channels * src_width,
 * dst_pitch >= channels * dst_width; the destination range must not overlap the source range; n_matrices 1 or n.
 * Pixel (x, y) of image i at d_src + (i * src_height + y) * src_pitch + channels * x; the destination likewise. Bytes between a row's
 * end and the next row are not written.
 * gms_resize_device / gms_warp_affine_device: n images on the context's stream; no allocation, no synchronisation, no readback, no
 *   workspace (graph-capturable). d_M: device doubles [n_matrices][6], read by the kernel: a captured graph follows new matrices.
 * gms_rotation_matrix_2d: getRotationMatrix2D on the host (the centre is rounded to float32 first); M receives 6 doubles.
 * gms_resize, gms_warp_affine, gms_img_rotate: ONE image on host pointers (dense rows; M on the host), synchronous, on the current HIP
 *   device. gms_img_rotate is the reference's img_rotate: the rotation about (width / 2., height / 2.), scale 1, same size. */
#define GMS_WARP_MAX_SIDE 8192
int gms_resize_device(gms_ctx* ctx, const uint8_t* d_src, int n, int src_width, int src_height, int channels, int src_pitch,
                      uint8_t* d_dst, int dst_width, int dst_height, int dst_pitch);
int gms_warp_affine_device(gms_ctx* ctx, const uint8_t* d_src, int n, int src_width, int src_height, int channels, int src_pitch,
                           const double* d_M, int n_matrices, uint8_t* d_dst, int dst_width, int dst_height, int dst_pitch);
int gms_rotation_matrix_2d(double center_x, double center_y, double angle, double scale, double* M);
int gms_resize(const uint8_t* src, int src_width, int src_height, int channels, uint8_t* dst, int dst_width, int dst_height);
int gms_warp_affine(const uint8_t* src, int src_width, int src_height, int channels, const double* M, uint8_t* dst, int dst_width,
                    int dst_height);
int gms_img_rotate(const uint8_t* src, int width, int height, int channels, double angle, uint8_t* dst);

/* ---- a dense cloud from a posed pair: rectify, match, reproject (the library's own step) --------------------------
 * The two-view stage leaves a pose (R, t) with X2 = R X1 + t; the stereo matchers read rectified pairs. This stage joins them. It
 * follows cv::stereoRectify, initUndistortRectifyMap, remap and reprojectImageTo3D in structure; the definition is this library's
 * (parity with an OpenCV build is unpinned), stated in csrc/rectify_core.h and in numpy in tests/rectify_ref.py: fp64, only
 * + - * / sqrt rint in one fixed order, so that the GPU, a host build of the header and numpy agree bit for bit.
 *   The plan of a pair: Rh = R^(-1/2) from the half-angle quaternion; b = -Rh t; a quarter turn Z about the optical axis that brings
 *     b nearest +x (turn 0: none, 1: half turn, 2 / 3: quarter turns for a baseline along +y / -y); the rotation A that takes
 *     g = Z b onto +x; R2 = A Z Rh, R1 = R2 R. Then R2 R R1^T = I and R2 t = (-B, 0, 0): camera 1 is the left image and points in
 *     front have positive disparity. The new camera: fx' = fy' = min(fx, fy); each camera's principal point puts the mean of its four
 *     undistorted, rotated source corners at the centre of the output, and both use the mean of the two, so that a point at
 *     infinity has disparity 0. Output size: as asked, or for out_width / out_height <= 0 the source's (swapped for turns 2 and 3).
 *     Not rectifiable (status GMS_ERR_NO_MODEL, every other field 0): trace R <= 0; g_x <= 0 or g_x < |g_z| (a baseline more than 45
 *     degrees out of the image plane); a source corner with z <= 0 after the rotation.
 *   A rectified byte: the ray R_k^T ((u - cx') / fx', (v - cy') / fy', 1); z <= 0: the byte is 0. Else the distortion model on
 *     (x / z, y / z), the source position with 5 fractional bits (rint), the integer part saturated to int16, and gms_warp_affine's
 *     blend of the four taps; a tap outside the source is 0 and is never read. valid (optional): 1 where all four taps are inside.
 *   A point: pixel (u, v) of the int16 map (4 fractional bits) is a point when d16 != filtered16, d16 >= min_disp16 and its valid
 *     byte is set. Z = fx' B 16 / d16, X = (u - cx') Z / fx', Y = (v - cy') Z / fx', p = R1^T (X, Y, Z): camera 1's frame in the unit
 *     of t, as the pair's sparse points3d. With a registration (d_pairs, d_reg, d_views all given) p_world = G_a.R^T (S p - G_a.t),
 *     as gms_sfm_register_device's d_points_world, and a pair whose registration status is not GMS_OK, or whose frame_a is not below n_frames, has no points. fp64, stored
 *     as float32.
 * gms_rectify_plan: one pair on the host, pure arithmetic. gms_rectify_plan_device: n_pairs pairs, R, t and status read from
 *   d_tv on the device (a pair whose two-view status is not GMS_OK gets the zeroed plan); camera is a HOST pointer.
 * gms_rectify_q: reprojectImageTo3D's 4 x 4 Q (row-major) of a plan, for disparities in pixels; host arithmetic.
 * gms_rectify_device: n images (layout and accepted arguments as gms_warp_affine_device's) through plan i, or through one plan
 *   (n_plans 1); which: 1 or 2, the camera of the pair. The plans are read by the kernel, so a captured graph follows new poses; a
 *   plan whose status is not GMS_OK gives zeros. d_valid (optional): dense [n][dst_height][dst_width]. No workspace, no allocation,
 *   no synchronisation, no readback (graph-capturable).
 * gms_rectify, gms_undistort: ONE image on host pointers (dense rows), synchronous, on the current HIP device. gms_rectify writes
 *   plan->out_w x out_h pixels; gms_undistort is cv::undistort with the new camera equal to the camera: no rotation, same size.
 * gms_dense_cloud_device: per pair, in raster order, the first `cap` points: d_xyz float32 [n][cap][3], d_color (optional) the
 *   bytes of d_image's pixel [n][cap][channels], d_pixel int32 [n][cap] = v * width + u; d_count int32 [n] states all the points,
 *   also beyond cap. Entries past the count are left as they were. d_disp16 and d_valid are dense [n][height][width]; d_image
 *   (optional: camera 1's rectified image, 1 or 3 channels) has rows image_pitch bytes apart. The order is fixed: counts per block
 *   of 1024 pixels, a scan, then the writes; no atomic. min_disp16 >= 1; cap >= 0; width and height 1..GMS_WARP_MAX_SIDE;
 *   d_workspace 256-byte aligned, gms_dense_cloud_workspace_bytes (0 for arguments that are refused). Stream-ordered, capturable.
 * gms_dense_pairs_device: the whole stage for n_pairs pairs in stream order, with no allocation, synchronisation or readback
 *   (graph-capturable): the plan kernel on d_tv; for BGR input (channels 3) gms_bgr_to_gray_device of both images; the grey images
 *   rectified into d_rect1 / d_rect2 with camera 1's valid plane in d_valid; for BGR input camera 1's colour image rectified into
 *   d_color; gms_stereo_sgm_device on the rectified pair into d_disp16; gms_dense_cloud_device with filtered16 =
 *   (min_disparity - 1) * 16 and colours from d_color (d_rect1 for grey input), in the world frame with a registration. Images
 *   are dense: pair i's image of camera k at d_imgk + i * height * width * channels. out_width, out_height >= 1: the rectified
 *   size of every pair (the plans are made for it). params NULL: GMS_STEREO_SGM_PARAMS_DENSE, the reference's record with
 *   min_disparity 0 and num_disparities 128 (the shared principal point makes every true disparity positive). d_plans [n],
 *   d_rect1, d_rect2, d_valid [n][out_height][out_width], d_color [n][out_height][out_width][3] (BGR input only), d_disp16 likewise
 *   int16; the cloud outputs as gms_dense_cloud_device's, d_cloud_color with `channels` bytes per point. A pair whose two-view
 *   status is not GMS_OK, or that is not rectifiable, has zero images, no valid pixel and count 0.
 * gms_dense_pairs_workspace_bytes: its workspace (256-byte aligned pointer); 0 for arguments that are refused.
 * gms_dense_pair: ONE pair on host pointers (dense rows; R [9] and t [3] on the host), synchronous, on the current HIP device. The
 *   plan comes back in *plan; out_width / out_height <= 0: its default size, which the caller reads from gms_rectify_plan_host
 *   beforehand to size rect1, rect2, valid [plan.out_h][plan.out_w], color (BGR input; optional) and disp16. Returns
 *   GMS_ERR_NO_MODEL when the pair is not rectifiable (nothing but *plan is written). cap points at most; *count states all. */
#define GMS_STEREO_SGM_PARAMS_DENSE {{5, 128, 0, GMS_STEREO_BM_PREFILTER_XSOBEL, 5, 61, 507, 0, 0, 8, 1}, 200, 800, 8}
typedef struct gms_rectify_plan {
    double  R1[9], R2[9];          /* x_rectified = R_k x_camera_k                                            */
    double  fx, fy, cx, cy;        /* the new camera of both images (fx = fy from gms_rectify_plan)           */
    double  B;                     /* the baseline |t|: R2 t = (-B, 0, 0)                                     */
    int32_t out_w, out_h;          /* the size the principal point was made for                               */
    int32_t turn;                  /* 0: none, 1: half turn, 2: quarter turn (baseline +y), 3: (baseline -y)  */
    int32_t status;                /* GMS_OK or GMS_ERR_NO_MODEL                                              */
} gms_rectify_plan;
int gms_rectify_plan_host(const gms_camera* camera, const double* R, const double* t, int width, int height, int out_width,
                          int out_height, gms_rectify_plan* plan);
int gms_rectify_plan_device(gms_ctx* ctx, const gms_camera* camera, const gms_two_view* d_tv, int n_pairs, int width, int height,
                            int out_width, int out_height, gms_rectify_plan* d_plans);
int gms_rectify_q(const gms_rectify_plan* plan, double* Q);
int gms_rectify_device(gms_ctx* ctx, const gms_camera* camera, const uint8_t* d_src, int n, int src_width, int src_height, int channels,
                       int src_pitch, const gms_rectify_plan* d_plans, int n_plans, int which, uint8_t* d_dst, int dst_width,
                       int dst_height, int dst_pitch, uint8_t* d_valid);
int gms_rectify(const gms_camera* camera, const gms_rectify_plan* plan, int which, const uint8_t* src, int src_width, int src_height,
                int channels, uint8_t* dst, uint8_t* valid);
int gms_undistort(const gms_camera* camera, const uint8_t* src, int width, int height, int channels, uint8_t* dst);
size_t gms_dense_cloud_workspace_bytes(int width, int height, int n_pairs);
int gms_dense_cloud_device(gms_ctx* ctx, const int16_t* d_disp16, const uint8_t* d_valid, const uint8_t* d_image, int channels,
                           int image_pitch, int n_pairs, int width, int height, const gms_rectify_plan* d_plans, int filtered16,
                           int min_disp16, const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views,
                           int n_frames, void* d_workspace, size_t workspace_bytes, int cap, float* d_xyz, uint8_t* d_color, int32_t* d_pixel,
                           int32_t* d_count);
size_t gms_dense_pairs_workspace_bytes(int src_width, int src_height, int channels, int out_width, int out_height, int n_pairs,
                                       const gms_stereo_sgm_params* params);
int gms_dense_pairs_device(gms_ctx* ctx, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1,
                           const uint8_t* d_img2, int n_pairs, int src_width, int src_height, int channels, const gms_two_view* d_tv,
                           int out_width, int out_height, int min_disp16, const gms_pair* d_pairs, const gms_sfm_pair_reg* d_reg,
                           const gms_sfm_view* d_views, int n_frames, void* d_workspace, size_t workspace_bytes, gms_rectify_plan* d_plans,
                           uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid, uint8_t* d_color, int16_t* d_disp16, int cap, float* d_xyz,
                           uint8_t* d_cloud_color, int32_t* d_pixel, int32_t* d_count);
int gms_dense_pair(const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* img1, const uint8_t* img2, int width,
                   int height, int channels, const double* R, const double* t, int out_width, int out_height, int min_disp16,
                   gms_rectify_plan* plan, uint8_t* rect1, uint8_t* rect2, uint8_t* valid, uint8_t* color, int16_t* disp16, int cap,
                   float* xyz, uint8_t* cloud_color, int32_t* pixel, int32_t* count);

/* ---- the clouds of several pairs fused into one by depth consistency (the library's own step) ----------------------
 * Stated in csrc/dense_fuse_core.h and in numpy in tests/dense_fuse_ref.py: fp64, only + - * / rint, every sum in one order; the GPU,
 * a host build of the header and numpy agree byte for byte.
 *   A source is one pair's output of the dense stage: gms_dense_fuse_src, an array of them in DEVICE memory whose pointers are device
 *   pointers (the kernels read everything through them when they run, so a captured graph follows new maps and poses). d_color, d_view
 *   (NULL: identity) and d_reg (NULL: S = 1, ok) are optional. A source is live when its plan's status is GMS_OK, its registration's
 *   is GMS_OK with S > 0 (or d_reg is NULL), its view is registered (or d_view is NULL), width and height are 1..GMS_WARP_MAX_SIDE and
 *   0 <= cap <= max_cap. A source that is not live has no points and sees nothing; a live one has n_i = min(*d_count, cap) points.
 *   look(P, j), P's three float32 widened: p = (G.R P + G.t) / S with source j's view and scale; r = R1 p; r.z <= 0: UNSEEN;
 *   u = fx (r.x / r.z) + cx, v likewise; (ui, vi) = rint, clamped, NaN -> INT32_MIN; outside the map: UNSEEN (checked before an address
 *   is formed); valid 0, d16 == filtered16 or d16 < min_disp16: UNSEEN; e = fx B 16 / r.z; |d16 - e| <= tol16: CONSISTENT, else CONFLICT.
 *   d_neighbors int32 [n_src][n_nb]: entry j of source i is skipped when j < 0, j >= n_src, j == i or source j is not live.
 *   Per point k < n_i of source i, over its neighbour slots in order: support = 1 + #CONSISTENT, conflict = #CONFLICT, duplicate = some
 *   CONSISTENT j < i. Kept: not a duplicate and support >= min_support. A rule per point, not a clustering: the lower copy of a
 *   dropped duplicate is not guaranteed to be kept itself.
 *   Kept points in source order, then the source's own order; the first fused_cap of them get d_xyz (the source's bits), d_color
 *   (optional; zeros for a source without colours), d_source, d_index (k), d_support, d_conflict. d_counts int32 [n_src + 1]: kept per
 *   source, then the total, also beyond fused_cap. Nothing past min(total, fused_cap) is written. No atomic decides a position.
 * gms_dense_fuse_device: stream-ordered on the context's stream; no allocation, no synchronisation, no readback; capturable (one
 *   stream, no parallel branches). max_cap bounds every source's cap and sizes the grid (the caps themselves are on the device).
 *   Refused (GMS_ERR_BAD_ARG, nothing run): n_src outside 1..65535, n_nb outside 1..32, channels not 1 or 3, tol16 < 0,
 *   min_support < 1, max_cap outside 1..GMS_WARP_MAX_SIDE^2, n_src * max_cap >= 2^31, fused_cap < 0, a NULL or misaligned pointer
 *   (d_workspace 256 bytes, d_src 8), a workspace below gms_dense_fuse_workspace_bytes (0 for arguments that are refused).
 * gms_dense_fuse: the same on HOST pointers, synchronous, on the current HIP device: src is a host array whose pointers are host
 *   pointers; also refuses a source whose width, height or cap is out of range. */
typedef struct gms_dense_fuse_src {
    const int16_t*          d_disp16;  /* [height][width]                                            */
    const uint8_t*          d_valid;   /* [height][width]                                            */
    const gms_rectify_plan* d_plan;
    const float*            d_xyz;     /* [cap][3]                                                   */
    const uint8_t*          d_color;   /* [cap][channels]; optional                                  */
    const int32_t*          d_count;
    const gms_sfm_view*     d_view;    /* the view of the pair's frame_a; NULL: identity             */
    const gms_sfm_pair_reg* d_reg;     /* the pair's registration; NULL: S = 1, ok                   */
    int32_t width, height;
    int32_t filtered16, min_disp16;    /* as passed to gms_dense_cloud_device                        */
    int32_t cap;
    int32_t reserved;
} gms_dense_fuse_src;
size_t gms_dense_fuse_workspace_bytes(int n_src, int max_cap);
int gms_dense_fuse_device(gms_ctx* ctx, const gms_dense_fuse_src* d_src, int n_src, int max_cap, const int32_t* d_neighbors, int n_nb,
                          int channels, int tol16, int min_support, void* d_workspace, size_t workspace_bytes, int fused_cap, float* d_xyz,
                          uint8_t* d_color, int32_t* d_source, int32_t* d_index, uint8_t* d_support, uint8_t* d_conflict, int32_t* d_counts);
int gms_dense_fuse(const gms_dense_fuse_src* src, int n_src, const int32_t* neighbors, int n_nb, int channels, int tol16, int min_support,
                   int fused_cap, float* xyz, uint8_t* color, int32_t* source, int32_t* index, uint8_t* support, uint8_t* conflict,
                   int32_t* counts);

/* ---- the speckle filter behind the matchers (cv::filterSpeckles for CV_16S) ----------------------------------------
 * Stated in csrc/speckle_core.h and twice in numpy in tests/speckle_ref.py; integer, free of any scan order, so the GPU, a host build
 * of the header and numpy agree byte for byte. Written from the published algorithm: parity with an OpenCV build is unpinned.
 *   On an int16 map [height][width] (dense rows): two pixels are linked when they are 4-neighbours, neither equals new_val and
 *   |a - b| <= max_diff, the difference taken in 32 bits (32767 beside -32768 differ by 65535). Components are the transitive
 *   closure of the links. Every pixel that is not new_val and whose component has at most max_speckle_size pixels becomes new_val;
 *   nothing else changes. max_diff is in the map's own units -- sixteenths of a pixel for the matchers' maps; it is not scaled, and
 *   neither of OpenCV's matcher conventions is claimed. max_speckle_size 0 leaves the maps as they are.
 * gms_filter_speckles_device: n maps, image i at d_disp16 + i * height * width, in place; d_removed (optional) int32 [n]: the pixels
 *   changed per map. Stream-ordered on the context's stream; no allocation, no synchronisation, no readback; capturable (one
 *   stream, no parallel branches). Refused (GMS_ERR_BAD_ARG, nothing run): width or height outside 1..8192, n outside 1..65535,
 *   new_val outside int16, max_speckle_size < 0, max_diff < 0, a NULL or misaligned pointer (d_workspace 256 bytes, d_disp16 2,
 *   d_removed 4), a workspace below gms_filter_speckles_workspace_bytes (8 bytes per pixel; 0 for arguments that are refused).
 * gms_filter_speckles: ONE map on host pointers, in place, synchronous, on the current HIP device; *removed (optional) the pixels
 *   changed.
 * gms_dense_pairs_filtered_device: gms_dense_pairs_device with the filter between the matcher and the cloud: on d_disp16 with
 *   new_val = (min_disparity - 1) * 16, the matcher's FILTERED code, max_speckle_size = speckle_size and max_diff = speckle_diff16;
 *   d_removed (optional) int32 [n_pairs]. The filter works in a region of its own behind gms_dense_pairs_device's workspace
 *   (gms_dense_pairs_filtered_workspace_bytes). speckle_size 0 is gms_dense_pairs_device: the same bytes.
 * gms_dense_pair_filtered: gms_dense_pair likewise; *removed (optional). */
size_t gms_filter_speckles_workspace_bytes(int width, int height, int n);
int gms_filter_speckles_device(gms_ctx* ctx, int16_t* d_disp16, int n, int width, int height, int new_val, int max_speckle_size,
                               int max_diff, void* d_workspace, size_t workspace_bytes, int32_t* d_removed);
int gms_filter_speckles(int16_t* disp16, int width, int height, int new_val, int max_speckle_size, int max_diff, int32_t* removed);
size_t gms_dense_pairs_filtered_workspace_bytes(int src_width, int src_height, int channels, int out_width, int out_height, int n_pairs,
                                                const gms_stereo_sgm_params* params);
int gms_dense_pairs_filtered_device(gms_ctx* ctx, const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* d_img1,
                                    const uint8_t* d_img2, int n_pairs, int src_width, int src_height, int channels,
                                    const gms_two_view* d_tv, int out_width, int out_height, int min_disp16, const gms_pair* d_pairs,
                                    const gms_sfm_pair_reg* d_reg, const gms_sfm_view* d_views, int n_frames, void* d_workspace,
                                    size_t workspace_bytes, gms_rectify_plan* d_plans, uint8_t* d_rect1, uint8_t* d_rect2, uint8_t* d_valid,
                                    uint8_t* d_color, int16_t* d_disp16, int cap, float* d_xyz, uint8_t* d_cloud_color, int32_t* d_pixel,
                                    int32_t* d_count, int speckle_size, int speckle_diff16, int32_t* d_removed);
int gms_dense_pair_filtered(const gms_camera* camera, const gms_stereo_sgm_params* params, const uint8_t* img1, const uint8_t* img2,
                            int width, int height, int channels, const double* R, const double* t, int out_width, int out_height,
                            int min_disp16, gms_rectify_plan* plan, uint8_t* rect1, uint8_t* rect2, uint8_t* valid, uint8_t* color,
                            int16_t* disp16, int cap, float* xyz, uint8_t* cloud_color, int32_t* pixel, int32_t* count, int speckle_size,
                            int speckle_diff16, int32_t* removed);

/* ---- camera calibration from chessboard photographs (main.cpp:53-68, CalibrationUtil.cpp:3-53) ---------------------
 * The corner finder is THIS LIBRARY'S OWN definition, not OpenCV's quad-based findChessboardCorners; cornerSubPix restates OpenCV
 * 4.5.2's algorithm in fp64; calibrateCamera follows its structure. Parity with an OpenCV build is unpinned. tests/calib_ref.py states
 * every step in numpy and csrc/calib_core.h holds the arithmetic.
 *   candidates: B = 5 x 5 box sum of the image, S = 5 x 5 box sum of B; with d = 4, sxx = S(x+d,y) + S(x-d,y) - 2 S, syy likewise along
 *     y, sxy = S(x+d,y+d) + S(x-d,y-d) - S(x+d,y-d) - S(x-d,y+d); R = max(0, sxy^2 - 4 sxx syy) >> 10 (64-bit products; R < 2^29), and
 *     R = 0 closer than GMS_DETECT_BORDER to an edge. A peak: R > 0, greater than every 17 x 17 neighbour earlier in raster order and
 *     not smaller than any later one. Per image the max_candidates peaks of largest R (ties cut and ordered in raster order), written
 *     in descending R, then raster order. Exact, whatever ties.
 * gms_chess_candidates_device: n (1..65535) equally sized grey images (sides 1..GMS_WARP_MAX_SIDE), pitch = width, back to back, on
 *   the context's stream; no allocation, no synchronisation, no readback (graph-capturable). d_workspace: 256-byte aligned,
 *   gms_chess_candidates_workspace_bytes (0 for arguments that are refused). d_out: [n][max_candidates] records, image i's first
 *   d_counts[i] are written, the others are left as they were. max_candidates 1..GMS_CHESS_MAX_CANDIDATES.
 * gms_corner_subpix_device: cv::cornerSubPix(win (5, 5), zeroZone (-1, -1), MAX_ITER + EPS (max_iter, eps)) on n_corners corners
 *   d_corners [n_corners][2] doubles (x, y), refined in place; corner i lies in image d_image_of[i] (NULL: all in image 0; an index
 *   outside 0..n_images-1 leaves the corner and reports status 2). d_status (may be NULL) [n_corners]: 0 refined; 1 the start kept, as the
 *   result moved more than win; 2 the start kept, as the 13 x 13 patch of samples left the image (OpenCV replicates the border there;
 *   this library refuses); 3 stopped on a singular system. win must be 5 (the committed mask), max_iter >= 1, eps >= 0.
 * gms_find_chessboard_corners: ONE grey image on host pointers (dense rows), synchronous, on the current HIP device: the nx * ny
 *   strongest candidates ordered onto the board of nx points per row and ny rows (nx != ny, both >= 2, nx * ny <= 4096). *found = 1 and
 *   corners [nx * ny][2] floats in findChessboardCorners' order (row by row; of the two half turns the one whose first point is smaller
 *   in (y, x); never mirrored), or *found = 0 (fewer candidates, or they do not lie on such a grid within a quarter cell).
 * gms_order_chessboard: the ordering alone, on the host, no GPU work: points [nx * ny][2] doubles (the first nx * ny candidates of an
 *   image) -> *found and ordered [nx * ny][2], by the same rule.
 * gms_corner_subpix: the same one image and corners [n][2] doubles on host pointers; a start whose patch leaves the image is
 *   GMS_ERR_BAD_ARG, and nothing is changed.
 * gms_calibrate_camera: host fp64, no GPU work (540 points and 69 parameters: not a kernel). n_views views; view v has counts[v] (>= 4)
 *   points: object_points [total][3] and image_points [total][2] doubles, the views back to back. Out: K [9] row-major, dist [5]
 *   (k1, k2, p1, p2, k3: OpenCV's flags = 0), rvecs and tvecs [n_views][3], *rms. GMS_ERR_DOMAIN: a view's points give no homography. */
#define GMS_CHESS_MAX_CANDIDATES 4096
typedef struct gms_chess_candidate {
    int32_t x, y;
    uint32_t response;
} gms_chess_candidate;
size_t gms_chess_candidates_workspace_bytes(int width, int height, int n_images);
int gms_chess_candidates_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, int max_candidates,
                                void* d_workspace, size_t workspace_bytes, gms_chess_candidate* d_out, int32_t* d_counts);
int gms_corner_subpix_device(gms_ctx* ctx, const uint8_t* d_images, int n_images, int width, int height, const int32_t* d_image_of,
                             double* d_corners, int n_corners, int win, int max_iter, double eps, int32_t* d_status);
int gms_find_chessboard_corners(const uint8_t* image, int width, int height, int nx, int ny, int* found, float* corners);
int gms_order_chessboard(const double* points, int nx, int ny, int* found, double* ordered);
int gms_corner_subpix(const uint8_t* image, int width, int height, double* corners, int n_corners, int win, int max_iter, double eps,
                      int32_t* status);
int gms_calibrate_camera(const double* object_points, const double* image_points, const int32_t* counts, int n_views, int width,
                         int height, double* K, double* dist, double* rvecs, double* tvecs, double* rms);

const char* gms_error_string(int code);
const char* gms_version(void);

/* Test hook (no production use): evaluates thresh = sqrt(T / n) * factor > score in device fp64 for
 * `count` (T, n, score) triples, so the tests can pin the device's div/sqrt/mul against IEEE.
 * Host pointers; out[i] = 1 iff the cell would be rejected. */
int gms_selftest_threshold(gms_ctx* ctx, const int32_t* T, const int32_t* n, const int32_t* score,
                           double factor, int count, uint8_t* out);

/* Test hook (no production use): the five-point minimal solver of gms_find_essential_batch_device alone, exactly as the RANSAC
 * kernel runs it, on n_samples caller-given samples of NORMALISED points. Host pointers: pts[20 s ..] = x1[5], y1[5], x2[5], y2[5]
 * of sample s; models[90 s ..] receives up to ten 3 x 3 matrices (zeros beyond counts[s]). */
int gms_selftest_five_point(gms_ctx* ctx, const double* pts, int n_samples, double* models, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* MI355_GMS_H */
