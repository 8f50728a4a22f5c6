"""Python mirror of the reference's operator: same name, argument meaning and output as

    cv::xfeatures2d::matchGMS(size1, size2, keypoints1, keypoints2, matches1to2, matchesGMS,
                              withRotation=false, withScale=false, thresholdFactor=6.0)

(reference call sites: SfM-GMS/SfM-GMS/FeatureMatchUtil.cpp:69, DisparityUtil.cpp:149,299).
Inputs/outputs are numpy structured arrays laid out exactly like cv::KeyPoint / cv::DMatch.
All work happens in csrc/libgms_hip.so on the GPU; nothing here computes the filter.
"""
import ctypes as C

import numpy as np

from .capi import load_library
from .types import (BF_RESULT_DTYPE, DMATCH_DTYPE, LOGOS_DICT_RESULT_DTYPE, KEYPOINT_DTYPE, PAIR_DTYPE, RESULT_DTYPE, GMS_OK, GMS_ERR_CAPACITY,
                    GmsError, SFM_PAIR_REG_DTYPE, SFM_PLAN_DTYPE, SFM_SUMMARY_DTYPE, SFM_VIEW_DTYPE, TWO_VIEW_DTYPE, concat_frames, desc_layout,
                    portrait_params, stereo_bm_params, stereo_sgm_params, GMS_ERR_BAD_ARG, RECTIFY_PLAN_DTYPE, STEREO_SGM_DENSE, RectifyPlan,
                    make_camera, rectify_plan_records, DENSE_FUSE_SRC_DTYPE, dense_fuse_neighbors, sfm_view_record, sfm_pair_reg_record)


def _as(arr, dtype, name):
    a = np.ascontiguousarray(arr)
    if a.dtype != dtype:
        raise TypeError(f"{name} must have dtype {dtype}, got {a.dtype}")
    return a


def _check(rc, lib, what):
    if rc != GMS_OK:
        msg = lib.gms_error_string(rc).decode()
        if rc == -3:
            msg += f" (hipError {lib.gms_last_hip_error()})"
        raise GmsError(rc, f"{what}: {msg}")


def _c_int(v):
    """An argument the C ABI takes as int: refused here when it does not fit, since ctypes would pass its low 32 bits."""
    v = int(v)
    if not -2 ** 31 <= v < 2 ** 31:
        raise GmsError(GMS_ERR_BAD_ARG, f"{v} does not fit a C int")
    return v


# one record of GmsContext.read_side_records (gms_ctx_read_side_records, GMS_SIDE_RECORD_BYTES)
SIDE_RECORD_DTYPE = np.dtype([("off", "<i8"), ("n", "<i4"), ("flags", "<u4"), ("stamp", "<u8"), ("pad", "<u4", (2,)), ("hist", "<u4", (400,))])
assert SIDE_RECORD_DTYPE.itemsize == 1632


class GmsContext:
    """gms_ctx: one per (process, device). Thread-safe for the one-shot call; stream-ordered batch calls."""

    OPTION_DEAL, OPTION_SCALE_PROBE, OPTION_IDENT = 1, 2, 3  # gms_ctx_set_option
    QUERY_LAST_IDENT, QUERY_IDENT_MISSES = 9, 10            # gms_ctx_query (the earlier ids: see query)

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.gms_ctx_create(int(device), C.byref(h)), self._lib, "gms_ctx_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gms_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def max_matches(self):
        return int(self._lib.gms_max_matches())

    def set_stream(self, hip_stream_handle):
        """Launch on a caller-owned HIP stream (e.g. torch.cuda.Stream().cuda_stream); 0/None = own stream."""
        _check(self._lib.gms_ctx_set_stream(self._h, C.c_void_p(hip_stream_handle or 0)), self._lib, "set_stream")

    def synchronize(self):
        _check(self._lib.gms_ctx_synchronize(self._h), self._lib, "synchronize")

    def set_option(self, option, value):
        """gms_ctx_set_option: option 1 = deal the matches to the lanes, 2 = probe scale hypotheses, 3 = the identity-query instantiation
        (OPTION_IDENT); value -1 (library's choice), 0, 1."""
        _check(self._lib.gms_ctx_set_option(self._h, int(option), int(value)), self._lib, "gms_ctx_set_option")

    def query(self, what):
        """gms_ctx_query: 1 = last launch dealt, 2 = its scale-probe mask, 3 = its matches per thread, 4 = launches, 5 = CUs, 6 / 7 = touch-ahead grid type / pairs ahead, 8 = last launch's first-round stagger (10 ns ticks),
        9 = last launch ran the identity-query instantiation (QUERY_LAST_IDENT), 10 = pairs that instantiation handed to the generic body so
        far (QUERY_IDENT_MISSES)."""
        v = C.c_int64(0)
        _check(self._lib.gms_ctx_query(self._h, int(what), C.byref(v)), self._lib, "gms_ctx_query")
        return int(v.value)

    # -- one-shot, host arrays ---------------------------------------------------------------------
    def match(self, size1, size2, keypoints1, keypoints2, matches1to2, withRotation=False, withScale=False,
              thresholdFactor=6.0, return_result=False):
        kp1 = _as(keypoints1, KEYPOINT_DTYPE, "keypoints1")
        kp2 = _as(keypoints2, KEYPOINT_DTYPE, "keypoints2")
        mt = _as(matches1to2, DMATCH_DTYPE, "matches1to2")
        out = np.empty(max(len(mt), 1), dtype=DMATCH_DTYPE)
        n_out = C.c_int(0)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        rc = self._lib.gms_match_ctx(self._h, kp1.ctypes.data, len(kp1), int(size1[0]), int(size1[1]),
                                     kp2.ctypes.data, len(kp2), int(size2[0]), int(size2[1]),
                                     mt.ctypes.data, len(mt), int(bool(withRotation)), int(bool(withScale)),
                                     float(thresholdFactor), out.ctypes.data, C.byref(n_out), res.ctypes.data)
        _check(rc, self._lib, "gms_match_ctx")
        kept = out[: n_out.value].copy()
        return (kept, res[0]) if return_result else kept

    # -- host-pointer batch path: many pairs per call, pinned staging and three lanes inside the library ----------
    def filter_host_batch(self, keypoints_per_frame, sizes, pairs, matches, withRotation=False, withScale=False,
                          thresholdFactor=6.0, out=None, results=None):
        """gms_filter_host_batch: `pairs` (PAIR_DTYPE) index `matches` (DMATCH_DTYPE) by match_off. Returns
        (out, results): pair i's survivors at out[match_off : match_off + results[i].n_inliers].
        keypoints_per_frame: a list of per-frame KEYPOINT_DTYPE arrays, or (all keypoints back to back, frame offsets [n_frames + 1])
        as the C ABI takes them (no concatenation per call). out / results: arrays of a previous call to write into -- a fresh
        output array costs first-touch page faults inside the call (7 ms for 327 MB), a C++ caller's std::vector has been touched
        by its constructor."""
        if isinstance(keypoints_per_frame, tuple):
            kp, frame_off = keypoints_per_frame
            n_kp = len(kp)
            kp = _as(kp, KEYPOINT_DTYPE, "keypoints") if n_kp else np.zeros(1, dtype=KEYPOINT_DTYPE)
            frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
            n_frames = len(np.asarray(sizes).reshape(-1, 2))
            # the library reads frame_off[-1] keypoints from kp: a prefix of a longer array is fine, running past its end is not
            if (frame_off.shape != (n_frames + 1,) or frame_off[0] != 0 or (np.diff(frame_off) < 0).any()
                    or frame_off[-1] > n_kp):
                raise ValueError("frame_off: one offset per frame and one more, from 0, never decreasing, the last at most len(keypoints)")
        else:
            kp, frame_off = concat_frames([_as(k, KEYPOINT_DTYPE, "keypoints") for k in keypoints_per_frame])
            kp = kp if len(kp) else np.zeros(1, dtype=KEYPOINT_DTYPE)
            n_frames = len(frame_off) - 1
        wh = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
        if wh.shape[0] != n_frames:
            raise ValueError("one (width, height) per frame")
        pairs = _as(pairs, PAIR_DTYPE, "pairs")
        mt = _as(matches, DMATCH_DTYPE, "matches")
        if out is None:
            out = np.zeros(max(len(mt), 1), dtype=DMATCH_DTYPE)
        if results is None:
            results = np.zeros(max(len(pairs), 1), dtype=RESULT_DTYPE)
        if (out.dtype != DMATCH_DTYPE or results.dtype != RESULT_DTYPE or len(out) < len(mt) or len(results) < len(pairs)
                or not out.flags["C_CONTIGUOUS"] or not results.flags["C_CONTIGUOUS"]):
            raise ValueError("out / results: contiguous DMATCH_DTYPE / RESULT_DTYPE arrays of at least len(matches) / len(pairs)")
        rc = self._lib.gms_filter_host_batch(self._h, kp.ctypes.data, frame_off.ctypes.data, wh.ctypes.data, n_frames,
                                             pairs.ctypes.data, len(pairs), mt.ctypes.data, int(bool(withRotation)),
                                             int(bool(withScale)), float(thresholdFactor), out.ctypes.data, results.ctypes.data)
        _check(rc, self._lib, "gms_filter_host_batch")
        return out[: len(mt)], results[: len(pairs)]

    # -- device-resident batch path (raw device pointers; torch tensors' data_ptr() are fine) ---------
    def reserve(self, n_pairs, max_m, withRotation=False, withScale=False):
        """gms_ctx_reserve: after it, filter_device calls of that shape neither allocate nor synchronise."""
        _check(self._lib.gms_ctx_reserve(self._h, int(n_pairs), int(max_m), int(bool(withRotation)), int(bool(withScale))),
               self._lib, "gms_ctx_reserve")

    def frame_table_bytes(self, total_kp):
        return int(self._lib.gms_frame_table_bytes(int(total_kp)))

    def normalize_device(self, d_kp, d_frame_off, d_wh, n_frames, total_kp, d_pts):
        _check(self._lib.gms_normalize_device(self._h, d_kp, d_frame_off, d_wh, int(n_frames), int(total_kp), d_pts),
               self._lib, "gms_normalize_device")

    def read_side_records(self, max_frames):
        """gms_ctx_read_side_records (diagnostic): the per-frame side records of the context's latest table build, after waiting for
        its stream -- SIDE_RECORD_DTYPE, at most max_frames of them (none when that build left none)."""
        buf = np.zeros(max(int(max_frames), 1), dtype=SIDE_RECORD_DTYPE)
        n = C.c_int(0)
        _check(self._lib.gms_ctx_read_side_records(self._h, buf.ctypes.data, int(max_frames) * SIDE_RECORD_DTYPE.itemsize, C.byref(n)),
               self._lib, "gms_ctx_read_side_records")
        return buf[: min(int(n.value), int(max_frames))]

    def filter_device(self, d_pts, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_matches, d_out, d_results,
                      d_mask=None, withRotation=False, withScale=False, thresholdFactor=6.0):
        _check(self._lib.gms_filter_device(self._h, d_pts, d_frame_off, int(n_frames), d_pairs, int(n_pairs),
                                           int(max_m), d_matches, int(bool(withRotation)), int(bool(withScale)),
                                           float(thresholdFactor), d_out, d_results, d_mask or None),
               self._lib, "gms_filter_device")

    # -- brute-force descriptor matcher on the resident frame table (FeatureMatchUtil.cpp:66-68) -----------------------
    def bf_prepared_bytes(self, desc_kind, total_desc, n_frames):
        return int(self._lib.gms_bf_prepared_bytes(int(desc_kind), int(total_desc), int(n_frames)))

    def bf_prepare_device(self, desc_kind, d_desc, d_frame_off, n_frames, total_desc, d_prepared):
        _check(self._lib.gms_bf_prepare_device(self._h, int(desc_kind), d_desc, d_frame_off, int(n_frames), int(total_desc),
                                               d_prepared or None), self._lib, "gms_bf_prepare_device")

    def bfmatch_device(self, desc_kind, d_desc, d_prepared, total_desc, d_frame_off, n_frames, d_pairs, n_pairs, max_query,
                       d_matches):
        _check(self._lib.gms_bfmatch_device(self._h, int(desc_kind), d_desc, d_prepared or None, int(total_desc), d_frame_off,
                                            int(n_frames), d_pairs, int(n_pairs), int(max_query), d_matches),
               self._lib, "gms_bfmatch_device")

    # -- bruteForceMatch: cross-check, sort and ratio prune behind the matcher (FeatureMatchUtil.cpp:20-31) ----------------
    def bf_select_workspace_bytes(self, n_pairs, max_rows, total_backward_rows):
        return int(self._lib.gms_bf_select_workspace_bytes(int(n_pairs), int(max_rows), int(total_backward_rows)))

    def bf_select_device(self, desc_kind, d_desc, d_prepared, total_desc, d_frame_off, n_frames, d_pairs, n_pairs, max_rows, cross_check,
                         distance_coef, max_size, d_ws, ws_bytes, d_out, d_bf_results, d_pair_results=None):
        _check(self._lib.gms_bf_select_device(self._h, int(desc_kind), d_desc or None, d_prepared or None, int(total_desc), d_frame_off,
                                              int(n_frames), d_pairs, int(n_pairs), int(max_rows), int(bool(cross_check)),
                                              float(distance_coef), int(max_size), d_ws, int(ws_bytes), d_out, d_bf_results,
                                              d_pair_results or None), self._lib, "gms_bf_select_device")

    # -- consumers of the filtered matches (DisparityUtil.cpp:179-201, SfMUtil.cpp:25-35) -------------------------------
    def disparity_device(self, d_kp1, n1, d_kp2, n2, d_matches, d_n_matches, max_matches, width, height, d_gt, disp_ratio,
                         d_disparity, d_work, d_stats):
        _check(self._lib.gms_disparity_device(self._h, d_kp1, int(n1), d_kp2, int(n2), d_matches, d_n_matches, int(max_matches),
                                              int(width), int(height), d_gt or None, int(disp_ratio), d_disparity, d_work,
                                              d_stats), self._lib, "gms_disparity_device")

    def gather_points_device(self, d_kp1, n1, d_kp2, n2, d_matches, d_n_matches, max_matches, d_coords1, d_coords2, d_status):
        _check(self._lib.gms_gather_points_device(self._h, d_kp1, int(n1), d_kp2, int(n2), d_matches, d_n_matches,
                                                  int(max_matches), d_coords1, d_coords2, d_status),
               self._lib, "gms_gather_points_device")

    def triangulate_device(self, camera, dist, P1, P2, d_coords1, d_coords2, d_n_matches, max_matches, d_points3d, d_stats):
        """gms_triangulate_device: camera = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3) or None, P1 / P2 3 x 4 (host values)."""
        cam = np.ascontiguousarray(camera, dtype=np.float64).reshape(4)
        dc = None if dist is None else np.ascontiguousarray(dist, dtype=np.float64).reshape(5)
        p1 = np.ascontiguousarray(P1, dtype=np.float64).reshape(12)
        p2 = np.ascontiguousarray(P2, dtype=np.float64).reshape(12)
        _check(self._lib.gms_triangulate_device(self._h, cam.ctypes.data, None if dc is None else dc.ctypes.data, p1.ctypes.data,
                                                p2.ctypes.data, d_coords1, d_coords2, d_n_matches, int(max_matches), d_points3d,
                                                d_stats), self._lib, "gms_triangulate_device")

    def recover_pose_device(self, E, camera, d_coords1, d_coords2, d_n_matches, max_matches, d_in_mask, d_pose, d_out_mask):
        """gms_recover_pose_device: E 3 x 3 and camera = (fx, fy, cx, cy) are host values; d_pose receives a POSE_DTYPE record."""
        e = np.ascontiguousarray(E, dtype=np.float64).reshape(9)
        cam = np.ascontiguousarray(camera, dtype=np.float64).reshape(4)
        _check(self._lib.gms_recover_pose_device(self._h, e.ctypes.data, cam.ctypes.data, d_coords1, d_coords2, d_n_matches,
                                                 int(max_matches), d_in_mask, d_pose, d_out_mask), self._lib, "gms_recover_pose_device")

    # -- the same consumers for a whole batch (SfMUtil.cpp:25-82, DisparityUtil.cpp:170-201): one launch per stage ---------------------
    def gather_points_batch_device(self, d_kp, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_coords1,
                                   d_coords2, d_tv):
        _check(self._lib.gms_gather_points_batch_device(self._h, d_kp, d_frame_off, int(n_frames), d_pairs, int(n_pairs), int(max_m),
                                                        d_filtered, d_results, d_coords1, d_coords2, d_tv),
               self._lib, "gms_gather_points_batch_device")

    def find_essential_batch_device(self, camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv, prob=0.999, threshold=1.0,
                                    max_iters=1000):
        """cv::findEssentialMat(..., RANSAC, prob, threshold, mask) per pair; camera: a CAMERA_DTYPE record (types.make_camera).
        The defaults are OpenCV's (0.999, 1.0); the reference's call, SfMUtil.cpp:39, passes 0.7 -- pipeline.run_dataset defaults to that."""
        _check(self._lib.gms_find_essential_batch_device(self._h, camera.ctypes.data, float(prob), float(threshold), int(max_iters),
                                                         d_pairs, int(n_pairs), d_coords1, d_coords2, d_mask, d_tv),
               self._lib, "gms_find_essential_batch_device")

    def recover_pose_batch_device(self, camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_tv, use_in_mask=True):
        _check(self._lib.gms_recover_pose_batch_device(self._h, camera.ctypes.data, int(bool(use_in_mask)), d_pairs, int(n_pairs),
                                                       d_coords1, d_coords2, d_mask, d_tv), self._lib, "gms_recover_pose_batch_device")

    def triangulate_batch_device(self, camera, d_pairs, n_pairs, d_coords1, d_coords2, d_mask, d_points3d, d_tv):
        _check(self._lib.gms_triangulate_batch_device(self._h, camera.ctypes.data, d_pairs, int(n_pairs), d_coords1, d_coords2,
                                                      d_mask or None, d_points3d, d_tv), self._lib, "gms_triangulate_batch_device")

    def two_view_batch_device(self, camera, d_kp, d_frame_off, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_coords1,
                              d_coords2, d_mask, d_points3d, d_tv, prob=0.999, threshold=1.0, max_iters=1000):
        """SfMUtil.cpp:25-82 for every pair of the batch: gather -> findEssentialMat -> recoverPose -> undistort + triangulate.
        prob defaults to OpenCV's 0.999; the reference passes 0.7 (SfMUtil.cpp:39): pass prob=0.7 to restate its flow."""
        _check(self._lib.gms_two_view_batch_device(self._h, camera.ctypes.data, float(prob), float(threshold), int(max_iters), d_kp,
                                                   d_frame_off, int(n_frames), d_pairs, int(n_pairs), int(max_m), d_filtered, d_results,
                                                   d_coords1, d_coords2, d_mask, d_points3d, d_tv), self._lib, "gms_two_view_batch_device")

    def disparity_batch_device(self, d_kp, d_frame_off, d_wh, n_frames, d_pairs, n_pairs, max_m, d_filtered, d_results, d_gt, gt_stride,
                               disp_ratio, d_disparity, map_stride, d_work, d_stats):
        _check(self._lib.gms_disparity_batch_device(self._h, d_kp, d_frame_off, d_wh, int(n_frames), d_pairs, int(n_pairs), int(max_m),
                                                    d_filtered, d_results, d_gt or None, int(gt_stride), int(disp_ratio), d_disparity,
                                                    int(map_stride), d_work, d_stats), self._lib, "gms_disparity_batch_device")

    # -- many views into one frame (include/gms.h) -------------------------------------------------------------------
    def sfm_register_workspace_bytes(self, n_frames, n_pairs, total_kp, total_matches):
        return int(self._lib.gms_sfm_register_workspace_bytes(int(n_frames), int(n_pairs), int(total_kp), int(total_matches)))

    def sfm_register_device(self, d_frame_off, n_frames, total_kp, d_pairs, d_plan, n_pairs, max_m, total_matches, d_filtered, d_mask,
                            d_points3d, d_tv, root, min_links, d_ws, ws_bytes, d_views, d_reg, d_points_world, d_track, cloud_cap, d_cloud,
                            d_cloud_id, d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary, d_keep=None):
        """gms_sfm_register_device on the pairs, survivors, mask, points and records gms_two_view_batch_device left; d_plan: sfm_plan's
        records in device memory. d_keep: a keep plane (match_unique_device's) -> gms_sfm_register_keep_device.
        Stream-ordered, capturable."""
        if d_keep:
            _check(self._lib.gms_sfm_register_keep_device(self._h, d_frame_off, int(n_frames), int(total_kp), d_pairs, d_plan, int(n_pairs),
                                                          int(max_m), int(total_matches), d_filtered, d_mask, d_points3d, d_tv, int(root),
                                                          int(min_links), d_ws, int(ws_bytes), d_views, d_reg, d_points_world, d_track,
                                                          int(cloud_cap), d_cloud, d_cloud_id, d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary,
                                                          d_keep), self._lib, "gms_sfm_register_keep_device")
            return
        _check(self._lib.gms_sfm_register_device(self._h, d_frame_off, int(n_frames), int(total_kp), d_pairs, d_plan, int(n_pairs), int(max_m),
                                                 int(total_matches), d_filtered, d_mask, d_points3d, d_tv, int(root), int(min_links), d_ws,
                                                 int(ws_bytes), d_views, d_reg, d_points_world, d_track, int(cloud_cap), d_cloud, d_cloud_id,
                                                 d_cloud_obs, d_cloud_est, d_cloud_spread, d_summary), self._lib, "gms_sfm_register_device")

    # -- one-to-one matches per pair (include/gms.h; batch.MatchUnique drives this) ---------------------------------
    def match_unique_workspace_bytes(self, n_pairs, total_kp, total_matches):
        return int(self._lib.gms_match_unique_workspace_bytes(int(n_pairs), int(total_kp), int(total_matches)))

    def match_unique_device(self, d_frame_off, n_frames, total_kp, d_pairs, n_pairs, max_m, total_matches, d_filtered, d_mask, d_tv, d_ws,
                            ws_bytes, d_keep, d_counts):
        """gms_match_unique_device on raw device pointers; d_mask / d_tv: None for every slot below m live. Stream-ordered, capturable."""
        _check(self._lib.gms_match_unique_device(self._h, d_frame_off or None, int(n_frames), int(total_kp), d_pairs or None, int(n_pairs),
                                                 int(max_m), int(total_matches), d_filtered or None, d_mask or None, d_tv or None, d_ws or None,
                                                 int(ws_bytes), d_keep or None, d_counts or None), self._lib, "gms_match_unique_device")

    # -- bundle adjustment behind the registration (include/gms.h) --------------------------------------------------
    def sfm_ba_workspace_bytes(self, n_frames, n_pairs, total_kp, cloud_cap):
        return int(self._lib.gms_sfm_ba_workspace_bytes(int(n_frames), int(n_pairs), int(total_kp), int(cloud_cap)))

    def sfm_ba_device(self, camera, params, d_kp, d_frame_off, n_frames, total_kp, d_pairs, n_pairs, total_matches, d_filtered, d_mask, d_views,
                      d_reg, d_track, cloud_cap, d_cloud, d_cloud_id, d_reg_summary, d_ws, ws_bytes, d_views_out, d_cloud_out, d_track_status,
                      d_summary):
        """gms_sfm_ba_device on what gms_two_view_batch_device and gms_sfm_register_device left; camera: a CAMERA_DTYPE record, params: a
        SFM_BA_PARAMS_DTYPE record (host values). Stream-ordered, capturable."""
        _check(self._lib.gms_sfm_ba_device(self._h, None if camera is None else camera.ctypes.data, None if params is None else params.ctypes.data,
                                           d_kp, d_frame_off, int(n_frames), int(total_kp), d_pairs, int(n_pairs), int(total_matches), d_filtered,
                                           d_mask, d_views, d_reg, d_track, int(cloud_cap), d_cloud, d_cloud_id, d_reg_summary, d_ws, int(ws_bytes),
                                           d_views_out, d_cloud_out, d_track_status, d_summary), self._lib, "gms_sfm_ba_device")

    # -- pair records from a view array (include/gms.h; batch.SfmPairPoses drives this) -------------------------------
    def sfm_pair_poses_device(self, d_views, n_frames, d_pairs, n_pairs, d_tv_out, d_reg_out):
        """gms_sfm_pair_poses_device on raw device pointers: SFM_VIEW_DTYPE views and PAIR_DTYPE pairs in, TWO_VIEW_DTYPE and
        SFM_PAIR_REG_DTYPE records out. Stream-ordered, capturable."""
        _check(self._lib.gms_sfm_pair_poses_device(self._h, d_views or None, int(n_frames), d_pairs or None, int(n_pairs), d_tv_out or None,
                                                   d_reg_out or None), self._lib, "gms_sfm_pair_poses_device")

    def detect_workspace_bytes(self, width, height, n_images, max_keypoints):
        return int(self._lib.gms_detect_workspace_bytes(int(width), int(height), int(n_images), int(max_keypoints)))

    def detect_batch_device(self, d_images, n_images, width, height, threshold, max_keypoints, d_ws, ws_bytes, d_kp, d_desc, d_counts):
        _check(self._lib.gms_detect_batch_device(self._h, d_images, int(n_images), int(width), int(height), int(threshold), int(max_keypoints),
                                                 d_ws, int(ws_bytes), d_kp, d_desc, d_counts), self._lib, "gms_detect_batch_device")

    def describe_device(self, d_image, width, height, d_kp, n, d_ws, ws_bytes, d_desc, d_status):
        _check(self._lib.gms_describe_device(self._h, d_image, int(width), int(height), d_kp, int(n), d_ws, int(ws_bytes), d_desc, d_status),
               self._lib, "gms_describe_device")

    # -- pyramid keypoint source (gms_detect_pyramid_*; batch.detect_images_pyramid / build_pyramid drive them) ---------------------
    def pyramid_level_sizes(self, width, height, n_levels):
        """[(w_l, h_l)] of the levels gms_detect_pyramid_batch_device uses for this image size (host arithmetic)."""
        n_levels = int(n_levels)
        ww, hh = np.zeros(max(n_levels, 1), np.int32), np.zeros(max(n_levels, 1), np.int32)
        n = self._lib.gms_pyramid_level_sizes(int(width), int(height), n_levels, ww.ctypes.data, hh.ctypes.data)
        _check(min(n, 0), self._lib, "gms_pyramid_level_sizes")
        return [(int(ww[l]), int(hh[l])) for l in range(n)]

    def detect_pyramid_workspace_bytes(self, width, height, n_images, max_keypoints, n_levels):
        return int(self._lib.gms_detect_pyramid_workspace_bytes(int(width), int(height), int(n_images), int(max_keypoints), int(n_levels)))

    def detect_pyramid_batch_device(self, d_images, n_images, width, height, threshold, max_keypoints, n_levels, d_ws, ws_bytes, d_kp, d_desc,
                                    d_counts, d_level_counts):
        _check(self._lib.gms_detect_pyramid_batch_device(self._h, d_images, int(n_images), int(width), int(height), int(threshold),
                                                         int(max_keypoints), int(n_levels), d_ws, int(ws_bytes), d_kp, d_desc, d_counts,
                                                         d_level_counts), self._lib, "gms_detect_pyramid_batch_device")

    def pyramid_build_device(self, d_images, n_images, width, height, n_levels, d_levels, levels_bytes):
        _check(self._lib.gms_pyramid_build_device(self._h, d_images, int(n_images), int(width), int(height), int(n_levels), d_levels,
                                                  int(levels_bytes)), self._lib, "gms_pyramid_build_device")

    # -- gradient descriptor: 128-float rows at the detector's keypoints (batch.detect_images_pyramid / describe_image drive them) -----
    def detect_pyramid_grad_workspace_bytes(self, width, height, n_images, max_keypoints, n_levels):
        return int(self._lib.gms_detect_pyramid_grad_workspace_bytes(int(width), int(height), int(n_images), int(max_keypoints), int(n_levels)))

    def detect_pyramid_grad_batch_device(self, d_images, n_images, width, height, threshold, max_keypoints, n_levels, d_ws, ws_bytes, d_kp,
                                         d_desc, d_counts, d_level_counts, d_rows128):
        _check(self._lib.gms_detect_pyramid_grad_batch_device(self._h, d_images, int(n_images), int(width), int(height), int(threshold),
                                                              int(max_keypoints), int(n_levels), d_ws, int(ws_bytes), d_kp, d_desc, d_counts,
                                                              d_level_counts, d_rows128), self._lib, "gms_detect_pyramid_grad_batch_device")

    def describe_grad_device(self, d_image, width, height, d_kp, n, d_ws, ws_bytes, d_rows128, d_status):
        _check(self._lib.gms_describe_grad_device(self._h, d_image, int(width), int(height), d_kp, int(n), d_ws, int(ws_bytes), d_rows128,
                                                  d_status), self._lib, "gms_describe_grad_device")

    # -- difference-of-Gaussians detector on the pyramid (batch.detect_images_pyramid(detector="dog") / dog_candidates drive them) -----
    def detect_dog_workspace_bytes(self, width, height, n_images, max_keypoints, n_levels):
        return int(self._lib.gms_detect_dog_workspace_bytes(int(width), int(height), int(n_images), int(max_keypoints), int(n_levels)))

    def detect_dog_batch_device(self, d_images, n_images, width, height, contrast, max_keypoints, n_levels, d_ws, ws_bytes, d_kp, d_desc,
                                d_counts, d_level_counts, d_rows128):
        _check(self._lib.gms_detect_dog_batch_device(self._h, d_images, int(n_images), int(width), int(height), int(contrast),
                                                     int(max_keypoints), int(n_levels), d_ws, int(ws_bytes), d_kp, d_desc, d_counts,
                                                     d_level_counts, d_rows128), self._lib, "gms_detect_dog_batch_device")

    def dog_candidates_device(self, d_images, n_images, width, height, contrast, d_cand):
        _check(self._lib.gms_dog_candidates_device(self._h, d_images, int(n_images), int(width), int(height), int(contrast), d_cand),
               self._lib, "gms_dog_candidates_device")

    # -- ... with its keypoints refined to 1/16 pixel and 1/16 layer (batch.detect_images_pyramid(refine=True) / dog_offsets drive them) --
    def detect_dog_refined_workspace_bytes(self, width, height, n_images, max_keypoints, n_levels):
        return int(self._lib.gms_detect_dog_refined_workspace_bytes(int(width), int(height), int(n_images), int(max_keypoints), int(n_levels)))

    def detect_dog_refined_batch_device(self, d_images, n_images, width, height, contrast, max_keypoints, n_levels, d_ws, ws_bytes, d_kp, d_desc,
                                        d_counts, d_level_counts, d_rows128):
        _check(self._lib.gms_detect_dog_refined_batch_device(self._h, d_images, int(n_images), int(width), int(height), int(contrast),
                                                             int(max_keypoints), int(n_levels), d_ws, int(ws_bytes), d_kp, d_desc, d_counts,
                                                             d_level_counts, d_rows128), self._lib, "gms_detect_dog_refined_batch_device")

    def dog_offsets_device(self, d_images, n_images, width, height, contrast, d_codes):
        _check(self._lib.gms_dog_offsets_device(self._h, d_images, int(n_images), int(width), int(height), int(contrast), d_codes),
               self._lib, "gms_dog_offsets_device")

    # -- from photographs to the tables (gms_bgr_to_gray_device / gms_detect_pack_device; batch.tables_from_detector drives them) ---
    def bgr_to_gray_device(self, d_bgr, n_images, width, height, d_gray):
        _check(self._lib.gms_bgr_to_gray_device(self._h, d_bgr or None, int(n_images), int(width), int(height), d_gray or None), self._lib,
               "gms_bgr_to_gray_device")

    def detect_pack_device(self, d_kp_blocks, d_rows32_blocks, d_rows128_blocks, d_counts, n_images, max_keypoints, d_kp, d_rows32, d_rows128,
                           d_frame_off):
        _check(self._lib.gms_detect_pack_device(self._h, d_kp_blocks or None, d_rows32_blocks or None, d_rows128_blocks or None, d_counts or None,
                                                int(n_images), int(max_keypoints), d_kp or None, d_rows32 or None, d_rows128 or None,
                                                d_frame_off or None), self._lib, "gms_detect_pack_device")

    # -- LOGOS on resident frames (gms_logos_*; batch.LogosTable / logos_pairs / logos_words drive them) ---------------------------
    def logos_table_bytes(self, total_kp, n_frames, n_words):
        return int(self._lib.gms_logos_table_bytes(int(total_kp), int(n_frames), int(n_words)))

    def logos_workspace_bytes(self, max_frame_kp, n_pairs, max_query_kp):
        return int(self._lib.gms_logos_workspace_bytes(int(max_frame_kp), int(n_pairs), int(max_query_kp)))

    def logos_prepare_device(self, d_kp, d_frame_off, n_frames, total_kp, d_words, n_words, d_ws, ws_bytes, d_table):
        _check(self._lib.gms_logos_prepare_device(self._h, d_kp or None, d_frame_off, int(n_frames), int(total_kp), d_words or None,
                                                  int(n_words), d_ws or None, int(ws_bytes), d_table), self._lib, "gms_logos_prepare_device")

    def logos_filter_device(self, d_table, d_pairs, n_pairs, d_ws, ws_bytes, d_out, d_logos_results, d_pair_results=None):
        _check(self._lib.gms_logos_filter_device(self._h, d_table, d_pairs, int(n_pairs), d_ws, int(ws_bytes), d_out, d_logos_results,
                                                 d_pair_results or None), self._lib, "gms_logos_filter_device")

    def logos_words_device(self, desc_kind, d_desc, total_desc, d_dict, n_words, d_words):
        _check(self._lib.gms_logos_words_device(self._h, int(desc_kind), d_desc or None, int(total_desc), d_dict, int(n_words),
                                                d_words or None), self._lib, "gms_logos_words_device")

    # -- LOGOS dictionary training (gms_logos_dict_*; batch.LogosDictionary / logos_dictionary drive them) ------------------------
    def logos_dict_workspace_bytes(self, desc_kind, total_rows, n_sets, n_words, attempts, max_iters):
        return int(self._lib.gms_logos_dict_workspace_bytes(int(desc_kind), int(total_rows), int(n_sets), int(n_words), int(attempts),
                                                            int(max_iters)))

    def logos_dict_train_device(self, desc_kind, d_desc, d_set_off, n_sets, total_rows, n_words, attempts, max_iters, seed, d_ws, ws_bytes,
                                d_dict, d_results, d_labels=None):
        _check(self._lib.gms_logos_dict_train_device(self._h, int(desc_kind), d_desc or None, d_set_off, int(n_sets), int(total_rows),
                                                     int(n_words), int(attempts), int(max_iters), int(seed) & 0xFFFFFFFFFFFFFFFF, d_ws,
                                                     int(ws_bytes), d_dict, d_results, d_labels or None),
               self._lib, "gms_logos_dict_train_device")

    # -- StereoBM block matching (DisparityUtil.cpp:22-49; batch.stereo_bm_batch drives these) ------------------------------------
    def stereo_bm_workspace_bytes(self, width, height, n_pairs, params=None):
        return int(self._lib.gms_stereo_bm_workspace_bytes(int(width), int(height), int(n_pairs), stereo_bm_params(params).ctypes.data))

    def stereo_bm_device(self, params, d_left, d_right, n_pairs, width, height, pitch, d_ws, ws_bytes, d_disp16, d_cost=None):
        """gms_stereo_bm_device; params: None (the reference's), a dict or a STEREO_BM_PARAMS_DTYPE record. Stream-ordered."""
        rec = stereo_bm_params(params)
        _check(self._lib.gms_stereo_bm_device(self._h, rec.ctypes.data, d_left, d_right, int(n_pairs), int(width), int(height), int(pitch),
                                              d_ws, int(ws_bytes), d_disp16, d_cost or None), self._lib, "gms_stereo_bm_device")

    # -- semi-global matching on StereoBM's costs (batch.stereo_sgm_batch drives these) --------------------------
    def stereo_sgm_workspace_bytes(self, width, height, n_pairs, params=None):
        return int(self._lib.gms_stereo_sgm_workspace_bytes(int(width), int(height), int(n_pairs), stereo_sgm_params(params).ctypes.data))

    def stereo_sgm_device(self, params, d_left, d_right, n_pairs, width, height, pitch, d_ws, ws_bytes, d_disp16, d_cost=None):
        """gms_stereo_sgm_device; params: None (the reference's), a dict or a STEREO_SGM_PARAMS_DTYPE record. Stream-ordered."""
        rec = stereo_sgm_params(params)
        _check(self._lib.gms_stereo_sgm_device(self._h, rec.ctypes.data, d_left, d_right, int(n_pairs), int(width), int(height), int(pitch),
                                               d_ws, int(ws_bytes), d_disp16, d_cost or None), self._lib, "gms_stereo_sgm_device")

    def stereo_bm_normalize_device(self, d_disp16, n, width, height, d_out8):
        _check(self._lib.gms_stereo_bm_normalize_device(self._h, d_disp16, int(n), int(width), int(height), d_out8), self._lib,
               "gms_stereo_bm_normalize_device")

    # -- portrait mode (DisparityUtil.cpp:317-412; batch.portrait_batch drives these) ---------------------------------------------
    def portrait_workspace_bytes(self, width, height, n, params=None):
        return int(self._lib.gms_portrait_workspace_bytes(int(width), int(height), int(n), portrait_params(params).ctypes.data))

    def portrait_device(self, params, d_bgr, d_disparity, n, width, height, pitch_bgr, pitch_disp, d_ws, ws_bytes, d_out_bgr,
                        d_mask=None, d_selected=None, d_blurred=None):
        """gms_portrait_device; params: None (the reference's), a dict or a PORTRAIT_PARAMS_DTYPE record. Stream-ordered."""
        rec = portrait_params(params)
        _check(self._lib.gms_portrait_device(self._h, rec.ctypes.data, d_bgr, d_disparity, int(n), int(width), int(height),
                                             int(pitch_bgr), int(pitch_disp), d_ws, int(ws_bytes), d_out_bgr, d_mask or None,
                                             d_selected or None, d_blurred or None), self._lib, "gms_portrait_device")

    PORTRAIT_STAGES = ("mask", "init", "merge", "flatten", "area", "select", "trace", "fill", "median")

    def portrait_profile_device(self, params, d_bgr, d_disparity, n, width, height, pitch_bgr, pitch_disp, d_ws, ws_bytes, d_out_bgr,
                                d_mask=None, d_selected=None, d_blurred=None):
        """gms_portrait_profile_device (a diagnostic; synchronises): the time of each kernel in ms, in PORTRAIT_STAGES' order."""
        rec = portrait_params(params)
        ms = np.zeros(len(self.PORTRAIT_STAGES), np.float32)
        _check(self._lib.gms_portrait_profile_device(self._h, rec.ctypes.data, d_bgr, d_disparity, int(n), int(width), int(height),
                                                     int(pitch_bgr), int(pitch_disp), d_ws, int(ws_bytes), d_out_bgr, d_mask or None,
                                                     d_selected or None, d_blurred or None, ms.ctypes.data), self._lib,
               "gms_portrait_profile_device")
        return ms

    def median_blur_device(self, d_src, n, width, height, channels, pitch, ksize, d_dst):
        _check(self._lib.gms_median_blur_device(self._h, d_src, int(n), int(width), int(height), int(channels), int(pitch), int(ksize),
                                                d_dst), self._lib, "gms_median_blur_device")

    # -- resize and warpAffine (main.cpp:36, :44, :114-120; batch.Warp drives these) ---------------------------------------------------
    def resize_device(self, d_src, n, src_width, src_height, channels, src_pitch, d_dst, dst_width, dst_height, dst_pitch):
        """gms_resize_device (cv::resize, INTER_LINEAR) on raw device pointers. Stream-ordered."""
        _check(self._lib.gms_resize_device(self._h, d_src, int(n), int(src_width), int(src_height), int(channels), int(src_pitch), d_dst,
                                           int(dst_width), int(dst_height), int(dst_pitch)), self._lib, "gms_resize_device")

    def warp_affine_device(self, d_src, n, src_width, src_height, channels, src_pitch, d_M, n_matrices, d_dst, dst_width, dst_height,
                           dst_pitch):
        """gms_warp_affine_device (cv::warpAffine, INTER_LINEAR, BORDER_CONSTANT 0); d_M: device doubles [n_matrices][6], the forward
        matrices, read when the kernel runs. Stream-ordered."""
        _check(self._lib.gms_warp_affine_device(self._h, d_src, int(n), int(src_width), int(src_height), int(channels), int(src_pitch),
                                                d_M, int(n_matrices), d_dst, int(dst_width), int(dst_height), int(dst_pitch)), self._lib,
               "gms_warp_affine_device")

    # -- a dense cloud from a posed pair (batch.Rectify / batch.DensePairs drive these) ------------------------------
    def rectify_plan_device(self, camera, d_tv, n_pairs, width, height, out_width, out_height, d_plans):
        """gms_rectify_plan_device: camera a CAMERA_DTYPE record (host), d_tv TWO_VIEW_DTYPE records and d_plans RECTIFY_PLAN_DTYPE
        records on the device. Stream-ordered."""
        _check(self._lib.gms_rectify_plan_device(self._h, camera.ctypes.data, d_tv or None, int(n_pairs), int(width), int(height),
                                                 int(out_width), int(out_height), d_plans or None), self._lib, "gms_rectify_plan_device")

    def rectify_device(self, camera, d_src, n, src_width, src_height, channels, src_pitch, d_plans, n_plans, which, d_dst, dst_width,
                       dst_height, dst_pitch, d_valid=None):
        """gms_rectify_device on raw device pointers; the plans are read when the kernel runs. Stream-ordered."""
        _check(self._lib.gms_rectify_device(self._h, camera.ctypes.data, d_src, int(n), int(src_width), int(src_height), int(channels),
                                            int(src_pitch), d_plans or None, int(n_plans), int(which), d_dst, int(dst_width), int(dst_height),
                                            int(dst_pitch), d_valid or None), self._lib, "gms_rectify_device")

    def dense_cloud_workspace_bytes(self, width, height, n_pairs):
        return int(self._lib.gms_dense_cloud_workspace_bytes(int(width), int(height), int(n_pairs)))

    def dense_cloud_device(self, d_disp16, d_valid, d_image, channels, image_pitch, n_pairs, width, height, d_plans, filtered16, min_disp16,
                           d_ws, ws_bytes, cap, d_xyz, d_color, d_pixel, d_count, d_pairs=None, d_reg=None, d_views=None, n_frames=0):
        """gms_dense_cloud_device on raw device pointers. Stream-ordered."""
        _check(self._lib.gms_dense_cloud_device(self._h, d_disp16 or None, d_valid or None, d_image or None, int(channels), int(image_pitch),
                                                int(n_pairs), int(width), int(height), d_plans or None, int(filtered16), int(min_disp16),
                                                d_pairs or None, d_reg or None, d_views or None, int(n_frames), d_ws or None, int(ws_bytes),
                                                int(cap), d_xyz or None, d_color or None, d_pixel or None, d_count or None), self._lib,
               "gms_dense_cloud_device")

    def dense_pairs_workspace_bytes(self, src_width, src_height, channels, out_width, out_height, n_pairs, params=None):
        return int(self._lib.gms_dense_pairs_workspace_bytes(int(src_width), int(src_height), int(channels), int(out_width), int(out_height),
                                                             int(n_pairs), dense_sgm_params(params).ctypes.data))

    def dense_pairs_device(self, camera, params, d_img1, d_img2, n_pairs, src_width, src_height, channels, d_tv, out_width, out_height,
                           min_disp16, d_ws, ws_bytes, d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color,
                           d_pixel, d_count, d_pairs=None, d_reg=None, d_views=None, n_frames=0):
        """gms_dense_pairs_device on raw device pointers; params: None (GMS_STEREO_SGM_PARAMS_DENSE), a dict or a record. Stream-ordered."""
        rec = dense_sgm_params(params)
        _check(self._lib.gms_dense_pairs_device(self._h, camera.ctypes.data, rec.ctypes.data, d_img1 or None, d_img2 or None, int(n_pairs),
                                                int(src_width), int(src_height), int(channels), d_tv or None, int(out_width), int(out_height),
                                                int(min_disp16), d_pairs or None, d_reg or None, d_views or None, int(n_frames), d_ws or None,
                                                int(ws_bytes), d_plans or None, d_rect1 or None, d_rect2 or None, d_valid or None,
                                                d_color or None, d_disp16 or None, int(cap), d_xyz or None, d_cloud_color or None,
                                                d_pixel or None, d_count or None), self._lib, "gms_dense_pairs_device")

    def dense_pairs_filtered_workspace_bytes(self, src_width, src_height, channels, out_width, out_height, n_pairs, params=None):
        return int(self._lib.gms_dense_pairs_filtered_workspace_bytes(int(src_width), int(src_height), int(channels), int(out_width),
                                                                      int(out_height), int(n_pairs), dense_sgm_params(params).ctypes.data))

    def dense_pairs_filtered_device(self, camera, params, d_img1, d_img2, n_pairs, src_width, src_height, channels, d_tv, out_width, out_height,
                                    min_disp16, d_ws, ws_bytes, d_plans, d_rect1, d_rect2, d_valid, d_color, d_disp16, cap, d_xyz, d_cloud_color,
                                    d_pixel, d_count, speckle_size, speckle_diff16, d_removed=None, d_pairs=None, d_reg=None, d_views=None,
                                    n_frames=0):
        """gms_dense_pairs_filtered_device: dense_pairs_device with the speckle filter (speckle_size, speckle_diff16 in sixteenths of a
        pixel) between the matcher and the cloud. Stream-ordered."""
        rec = dense_sgm_params(params)
        _check(self._lib.gms_dense_pairs_filtered_device(self._h, camera.ctypes.data, rec.ctypes.data, d_img1 or None, d_img2 or None, int(n_pairs),
                                                         int(src_width), int(src_height), int(channels), d_tv or None, int(out_width),
                                                         int(out_height), int(min_disp16), d_pairs or None, d_reg or None, d_views or None,
                                                         int(n_frames), d_ws or None, int(ws_bytes), d_plans or None, d_rect1 or None,
                                                         d_rect2 or None, d_valid or None, d_color or None, d_disp16 or None, int(cap),
                                                         d_xyz or None, d_cloud_color or None, d_pixel or None, d_count or None,
                                                         int(speckle_size), int(speckle_diff16), d_removed or None), self._lib,
               "gms_dense_pairs_filtered_device")

    # -- the speckle filter (batch.SpeckleFilter drives these) ----------------------------------------------------------
    def filter_speckles_workspace_bytes(self, width, height, n):
        return int(self._lib.gms_filter_speckles_workspace_bytes(int(width), int(height), int(n)))

    def filter_speckles_device(self, d_disp16, n, width, height, new_val, max_speckle_size, max_diff, d_ws, ws_bytes, d_removed=None):
        """gms_filter_speckles_device on raw device pointers: n int16 maps filtered in place. Stream-ordered."""
        _check(self._lib.gms_filter_speckles_device(self._h, d_disp16 or None, int(n), int(width), int(height), _c_int(new_val),
                                                    _c_int(max_speckle_size), _c_int(max_diff), d_ws or None, int(ws_bytes),
                                                    d_removed or None), self._lib, "gms_filter_speckles_device")

    # -- the clouds of several pairs fused into one (batch.DenseFuse drives these) --------------------------------------
    def dense_fuse_workspace_bytes(self, n_src, max_cap):
        return int(self._lib.gms_dense_fuse_workspace_bytes(int(n_src), int(max_cap)))

    def dense_fuse_device(self, d_src, n_src, max_cap, d_neighbors, n_nb, channels, tol16, min_support, d_ws, ws_bytes, fused_cap, d_xyz, d_color,
                          d_source, d_index, d_support, d_conflict, d_counts):
        """gms_dense_fuse_device on raw device pointers: d_src DENSE_FUSE_SRC_DTYPE records on the device. Stream-ordered."""
        _check(self._lib.gms_dense_fuse_device(self._h, d_src or None, int(n_src), int(max_cap), d_neighbors or None, int(n_nb), int(channels),
                                               int(tol16), int(min_support), d_ws or None, int(ws_bytes), int(fused_cap), d_xyz or None,
                                               d_color or None, d_source or None, d_index or None, d_support or None, d_conflict or None,
                                               d_counts or None), self._lib, "gms_dense_fuse_device")

    # -- chessboard corner candidates and cornerSubPix (batch.ChessCorners drives these) ---------------------------------
    def chess_candidates_workspace_bytes(self, width, height, n_images):
        return int(self._lib.gms_chess_candidates_workspace_bytes(int(width), int(height), int(n_images)))

    def chess_candidates_device(self, d_images, n_images, width, height, max_candidates, d_ws, ws_bytes, d_out, d_counts):
        """gms_chess_candidates_device on raw device pointers: d_out [n][max_candidates] CHESS_CANDIDATE_DTYPE, d_counts int32 [n].
        Stream-ordered."""
        _check(self._lib.gms_chess_candidates_device(self._h, d_images or None, int(n_images), int(width), int(height), int(max_candidates),
                                                     d_ws or None, int(ws_bytes), d_out or None, d_counts or None), self._lib,
               "gms_chess_candidates_device")

    def corner_subpix_device(self, d_images, n_images, width, height, d_image_of, d_corners, n_corners, win=5, max_iter=30, eps=0.1,
                             d_status=None):
        """gms_corner_subpix_device: d_corners float64 [n_corners, 2] refined in place; d_image_of int32 [n_corners] or None (image 0).
        Stream-ordered."""
        _check(self._lib.gms_corner_subpix_device(self._h, d_images or None, int(n_images), int(width), int(height), d_image_of or None,
                                                  d_corners or None, int(n_corners), int(win), int(max_iter), float(eps), d_status or None),
               self._lib, "gms_corner_subpix_device")

    def selftest_five_point(self, x1, x2):
        """gms_selftest_five_point: x1, x2 [n_samples, 5, 2] normalised points -> list of [k, 3, 3] model arrays, one per sample."""
        x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 5, 2)
        x2 = np.asarray(x2, dtype=np.float64).reshape(-1, 5, 2)
        n = len(x1)
        pts = np.ascontiguousarray(np.concatenate([x1[:, :, 0], x1[:, :, 1], x2[:, :, 0], x2[:, :, 1]], axis=1))
        models, counts = np.zeros((max(n, 1), 90)), np.zeros(max(n, 1), dtype=np.int32)
        _check(self._lib.gms_selftest_five_point(self._h, pts.ctypes.data, n, models.ctypes.data, counts.ctypes.data), self._lib, "selftest_five_point")
        return [models[i, :9 * counts[i]].reshape(-1, 3, 3) for i in range(n)]

    def selftest_threshold(self, T, n, score, factor):
        T = np.ascontiguousarray(T, dtype=np.int32)
        n = np.ascontiguousarray(n, dtype=np.int32)
        score = np.ascontiguousarray(score, dtype=np.int32)
        out = np.zeros(len(T), dtype=np.uint8)
        _check(self._lib.gms_selftest_threshold(self._h, T.ctypes.data, n.ctypes.data, score.ctypes.data,
                                                float(factor), len(T), out.ctypes.data), self._lib, "selftest")
        return out


_default_ctx = None


def matchGMS(size1, size2, keypoints1, keypoints2, matches1to2, withRotation=False, withScale=False,
             thresholdFactor=6.0):
    """Drop-in for cv::xfeatures2d::matchGMS; returns matchesGMS (the surviving DMatch, in input order).

    size = (width, height) like cv::Size. Raises GmsError instead of the reference's undefined behaviour
    on out-of-domain input."""
    return default_context().match(size1, size2, keypoints1, keypoints2, matches1to2, withRotation, withScale, thresholdFactor)


def matchLOGOS(keypoints1, keypoints2, nn1, nn2):
    """cv::xfeatures2d::matchLOGOS(keypoints1, keypoints2, nn1, nn2, matches1to2) (FeatureMatchUtil.cpp:86-131) on the GPU.

    keypoints*: KEYPOINT_DTYPE arrays (pt, size and angle are read); nn*: the visual word of each keypoint (int32). Returns the
    surviving DMATCH_DTYPE records (queryIdx, trainIdx, imgIdx -1, distance 0) in the reference's order.

    Keypoint domain: pt.x, pt.y and angle finite, |angle| <= 3600 degrees (-1, OpenCV's "no orientation", is inside); size is not
    restricted. Outside it the reference does not terminate; here GmsError with code GMS_ERR_DOMAIN is raised before any device work."""
    lib = load_library()
    kp1 = _as(keypoints1, KEYPOINT_DTYPE, "keypoints1")
    kp2 = _as(keypoints2, KEYPOINT_DTYPE, "keypoints2")
    l1 = np.ascontiguousarray(nn1, dtype=np.int32)
    l2 = np.ascontiguousarray(nn2, dtype=np.int32)
    if l1.shape != (len(kp1),) or l2.shape != (len(kp2),):
        raise ValueError("nn1 / nn2 must hold one label per keypoint")
    # survivors rarely outnumber the larger frame: that first capacity avoids a second run in the common case
    cap = max(len(kp1), len(kp2))
    while True:
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        n = C.c_int64(0)
        rc = lib.gms_logos_match(kp1.ctypes.data, len(kp1), kp2.ctypes.data, len(kp2), l1.ctypes.data, l2.ctypes.data,
                                 out.ctypes.data, cap, C.byref(n), None)
        if rc == GMS_ERR_CAPACITY and n.value > cap:   # run again with room for what it reported
            cap = n.value
            continue
        _check(rc, lib, "gms_logos_match")
        return out[: n.value].copy()


def logos_dict_args(kind, n_words, attempts, max_iters):
    """The argument checks of the dictionary trainer, as include/gms.h states them -> (dtype, row width)."""
    layout = desc_layout(kind)
    if not 1 <= int(n_words) <= 65535:
        raise ValueError("1 <= n_words <= 65535")
    if not 1 <= int(attempts) <= 16 or not 1 <= int(max_iters) <= 1000:
        raise ValueError("1 <= attempts <= 16 and 1 <= max_iters <= 1000")
    return layout


def trainLogosDictionary(descriptors, kind, n_words=50, attempts=3, max_iters=100, seed=0, detail=False):
    """The dictionary the reference gets from BOWKMeansTrainer(n_words).cluster(descriptors) (FeatureMatchUtil.cpp:100-104), trained
    on the GPU (gms_logos_dict_train): k-means with k-means++ seeding, `attempts` restarts, at most `max_iters`
    assignments. It is not OpenCV's dictionary (cv::kmeans draws from a global RNG and sums in float): the definition is this
    library's own and gives the same bytes on every run for the same rows and seed.

    descriptors: uint8 [n, 32] for GMS_DESC_HAMMING256, float32 [n, 128] for GMS_DESC_L2_F32X128 (finite, |x| <= 4096), n_words <= n
    <= 2^20. Returns the dictionary [n_words, width]; with detail=True also the LOGOS_DICT_RESULT_DTYPE record and the word of every
    row. Rows outside the domain or too few of them raise GmsError."""
    dt, width = logos_dict_args(kind, n_words, attempts, max_iters)
    lib = load_library()
    rows = np.ascontiguousarray(descriptors, dtype=dt).reshape(-1, width)
    off = np.array([0, len(rows)], np.int64)
    dic = np.zeros((int(n_words), width), dt)
    rec = np.zeros(1, LOGOS_DICT_RESULT_DTYPE)
    labels = np.full(max(len(rows), 1), -1, np.int32)
    rc = lib.gms_logos_dict_train(int(kind), rows.ctypes.data if len(rows) else None, off.ctypes.data, 1, int(n_words), int(attempts),
                                  int(max_iters), int(seed) & 0xFFFFFFFFFFFFFFFF, dic.ctypes.data, rec.ctypes.data, labels.ctypes.data)
    _check(rc, lib, "gms_logos_dict_train")
    _check(int(rec[0]["status"]), lib, "gms_logos_dict_train (the training set)")
    return (dic, rec[0], labels[: len(rows)]) if detail else dic


def bruteForceMatch(desc1, desc2, kind, cross_check=True, distance_coef=4.0, max_size=500, detail=False):
    """The reference's bruteForceMatch (FeatureMatchUtil.cpp:20-31) on the GPU: BFMatcher(norm, crossCheck).match(desc1, desc2),
    std::sort by distance (MSVC's order among equal distances), then the survivors within distance_coef * d_min, at most max_size.

    desc1 / desc2: query / train rows -- uint8 [n, 32] for GMS_DESC_HAMMING256, float32 [n, 128] for GMS_DESC_L2_F32X128.
    cross_check=False: the reference's match() helper (no cross-check, same sort and prune). Returns DMATCH_DTYPE records
    (queryIdx, trainIdx, imgIdx 0, distance); with detail=True also the BF_RESULT_DTYPE record. An empty frame raises GmsError
    (GMS_ERR_DOMAIN): the reference reads front() of an empty vector there."""
    lib = load_library()
    kind = int(kind)
    dt, width = desc_layout(kind)
    d1 = np.ascontiguousarray(desc1, dtype=dt).reshape(-1, width)
    d2 = np.ascontiguousarray(desc2, dtype=dt).reshape(-1, width)
    cap = min(int(max_size), len(d1)) if max_size >= 0 else 0
    out = np.zeros(max(cap, 1), DMATCH_DTYPE)
    n = C.c_int64(0)
    res = np.zeros(1, BF_RESULT_DTYPE)
    rc = lib.gms_bf_match_select(kind, d1.ctypes.data if len(d1) else None, len(d1), d2.ctypes.data if len(d2) else None, len(d2),
                                 int(bool(cross_check)), float(distance_coef), int(max_size), out.ctypes.data, cap, C.byref(n),
                                 res.ctypes.data)
    _check(rc, lib, "gms_bf_match_select")
    got = out[: n.value].copy()
    return (got, res[0]) if detail else got


def structureFromMotion(img1, img2, camera, dist=None, method="logos", ctx=None, **params):
    """The reference's structureFromMotion(imgL, imgR, cameraMatrix, distCoeffs, points3D, ..., algo) (SfMUtil.cpp:4-83, called at
    main.cpp:71-75) on two photographs of one size, [H, W] grey or [H, W, 3] BGR, 8-bit, host arrays or device tensors: keypoints and
    rows of both, the method's matches, findEssentialMat(RANSAC, 0.7, 1.0), recoverPose, undistortPoints and triangulation, all on
    the GPU (pipeline.run_images; keypoints and rows do not pass through the host on the way).

    method  "bf"     algo 1, bruteForceMatch (cross-check, sort, ratio prune; FeatureMatchUtil.cpp:20-31)
            "gms"    algo 2, nearest neighbour then matchGMS(true, true) (FeatureMatchUtil.cpp:66-69)
            "logos"  algo 3, matchLOGOS on 50 visual words trained on image 1's rows (FeatureMatchUtil.cpp:101-102); what main.cpp:74 passes
    camera = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3) or None. params: run_images' keywords (threshold, max_keypoints, n_levels,
    detector, contrast, refine, descriptor, thresholdFactor, prob, ransac_threshold, cross_check, distance_coef, max_size, dictionary, train_dictionary, ...).
    The keypoints and rows are this library's own (detector="dog", and refine=True
    for its sub-pixel position and sub-level size: 4.7d), not SIFT's.

    Returns a dict: points3D float64 [k, 3] (the inliers' points, in their order), R [3, 3], t [3], E [3, 3], matches (the method's
    surviving DMATCH_DTYPE records), mask (uint8 per surviving match: 0 = not an inlier of the pose), keypoints1, keypoints2
    (KEYPOINT_DTYPE), two_view (the pair's TWO_VIEW_DTYPE record: counts, iterations, reprojection sums) and detail (run_images'
    record, with `tables`: the resident FrameTable and DescriptorTable). A pair without a pose raises GmsError with the two-view status.
    dense=True among params (run_images' min_disp16, dense_cap, dense_sgm): adds `dense`, the pair's dense cloud in
    points3D's frame and unit -- a dict of points, colors, pixel, count and plan, or None when the pose is not rectifiable.
    dense_speckle = (max_speckle_size, max_diff16) beside it: filterSpeckles on the matcher's map before the reprojection (DESIGN.md
    4.13c); the entry then also holds removed. None, the default: no filter."""
    from . import pipeline
    if method not in pipeline.METHODS:
        raise ValueError(f"unknown method {method!r}")
    shapes = [tuple(im.shape) for im in (img1, img2)]
    if len(shapes[0]) not in (2, 3) or (len(shapes[0]) == 3 and shapes[0][2] != 3):
        raise ValueError("img1 / img2: [H, W] grey or [H, W, 3] BGR")
    if shapes[0] != shapes[1]:
        raise ValueError("img1 and img2: one size and one channel count")
    opts = dict(params)
    if method == "gms":
        opts.setdefault("withRotation", True)
        opts.setdefault("withScale", True)
    if method == "logos" and opts.get("dictionary") is None:
        opts.setdefault("train_dictionary", True)
    r = pipeline.run_images(ctx or default_context(), [img1, img2], camera, dist, method=method, pairs=[(0, 1)], keep_tables=True, **opts)
    frames = r["tables"][0]
    tv, off, k = r["two_view"][0], int(r["pairs"]["match_off"][0]), int(r["results"]["n_inliers"][0])
    if int(r["results"]["status"][0]) != GMS_OK or int(tv["status"]) != GMS_OK:
        raise GmsError(int(r["results"]["status"][0]) or int(tv["status"]), "structureFromMotion: no pose for this pair")
    kp = frames.d_kp.cpu().numpy()[: frames.total * KEYPOINT_DTYPE.itemsize].view(KEYPOINT_DTYPE)
    f = frames.frame_off_host
    out = dict(points3D=r["points3d"][off:off + int(tv["n_triangulated"])].copy(), R=tv["R"].copy(), t=tv["t"].copy(), E=tv["E"].copy(),
               matches=r["out"][off:off + k].copy(), mask=r["mask"][off:off + k].copy(), keypoints1=kp[f[0]:f[1]].copy(),
               keypoints2=kp[f[1]:f[2]].copy(), two_view=tv, detail=r)
    if "dense" in r:
        out["dense"] = r["dense"][0]
    return out


def sfm_plan(pairs, n_frames, root=0):
    """gms_sfm_plan (host arithmetic, no device): which pairs of the list register a frame out of `root`, in list order, and which
    pair each takes its scale from. pairs: PAIR_DTYPE records or (frame_a, frame_b) rows -> SFM_PLAN_DTYPE [n]. A frame index or root
    out of range raises GmsError(GMS_ERR_BAD_ARG)."""
    recs = _pair_records(pairs)
    plan = np.zeros(len(recs), SFM_PLAN_DTYPE)
    lib = load_library()
    _check(lib.gms_sfm_plan(recs.ctypes.data, len(recs), int(n_frames), int(root), plan.ctypes.data), lib, "gms_sfm_plan")
    return plan


def _pair_records(pairs):
    a = np.asarray(pairs)
    if a.dtype == PAIR_DTYPE:
        return np.ascontiguousarray(a)
    fp = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    recs = np.zeros(len(fp), PAIR_DTYPE)
    recs["frame_a"], recs["frame_b"] = fp[:, 0], fp[:, 1]
    return recs


def sfm_outputs(n_frames, n_pairs, total_matches, cloud_cap):
    """Zeroed host arrays for the outputs of gms_sfm_register, in the order the C call takes them."""
    return dict(views=np.zeros(n_frames, SFM_VIEW_DTYPE), registration=np.zeros(n_pairs, SFM_PAIR_REG_DTYPE),
                points_world=np.zeros((total_matches, 3)), track=np.zeros(total_matches, np.int32), cloud=np.zeros((cloud_cap, 3)),
                cloud_id=np.zeros(cloud_cap, np.int32), cloud_obs=np.zeros(cloud_cap, np.int32), cloud_est=np.zeros(cloud_cap, np.int32),
                cloud_spread=np.zeros(cloud_cap), summary=np.zeros(1, SFM_SUMMARY_DTYPE))


def sfm_trim(out):
    """The cloud arrays of a registration cut to the tracks they hold (the summary's n_tracks, at most their capacity)."""
    n = min(int(out["summary"]["n_tracks"][0]), len(out["cloud_id"]))
    for k in ("cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread"):
        out[k] = out[k][:n]
    return out


def uniqueMatches(matches, n1, n2, mask=None):
    """gms_match_unique on one match list (synchronous, on the current device): matches DMATCH_DTYPE between n1 query and n2 train
    keypoints, mask uint8 per match or None -> (keep uint8 per match, (live, kept)). A match is live when its mask byte is non-zero
    and both indices lie inside; it is kept when it is the best (distance, then position; negative, infinite and NaN distances last)
    of the live matches on its train keypoint and of those on its query keypoint. One-to-one, not a maximum matching (DESIGN.md
    4.10e)."""
    m = _as(matches, DMATCH_DTYPE, "matches")
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if mk is not None and len(mk) != len(m):
        raise ValueError("mask: one byte per match")
    frame_off = np.array([0, int(n1), int(n1) + int(n2)], np.int64)
    recs = np.zeros(1, PAIR_DTYPE)
    recs[0] = (0, 1, len(m), 0, 0)
    keep, counts = np.zeros(len(m), np.uint8), np.zeros(2, np.int32)
    lib = load_library()
    _check(lib.gms_match_unique(frame_off.ctypes.data, 2, recs.ctypes.data, 1, m.ctypes.data, None if mk is None else mk.ctypes.data, None,
                                keep.ctypes.data, counts.ctypes.data), lib, "gms_match_unique")
    return keep, (int(counts[0]), int(counts[1]))


def registerViews(frame_off, pairs, matches, mask, points3d, two_view, root=0, min_links=8, cloud_cap=None, keep=None):
    """gms_sfm_register, the one-shot on host arrays (synchronous, on the current device): the two-view results of many pairs --
    frame_off int64 [n_frames + 1], pairs PAIR_DTYPE, and matches (DMATCH_DTYPE), mask (uint8), points3d ([.., 3] float64) laid out by
    the pairs' match_off, two_view TWO_VIEW_DTYPE per pair: pipeline.run_dataset's arrays -- joined into the frame of `root`. Returns
    dict(plan, views SFM_VIEW_DTYPE per frame, registration SFM_PAIR_REG_DTYPE per pair, points_world, track, cloud, cloud_id,
    cloud_obs, cloud_est, cloud_spread, summary). Loop closure is not done; re-triangulation over all views and
    bundle adjustment are bundleAdjust's, on this call's result. keep: a keep plane, uint8 per match slot (batch.unique_matches';
    DESIGN.md 4.10e) -> gms_sfm_register_keep: a match whose byte is 0 feeds no track; None: gms_sfm_register."""
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    recs = _as(pairs, PAIR_DTYPE, "pairs")
    n_frames, n = len(frame_off) - 1, len(recs)
    total = int((recs["match_off"] + np.maximum(recs["m"], 0)).max()) if n else 0
    m = _as(matches, DMATCH_DTYPE, "matches")
    mk, pts = np.ascontiguousarray(mask, dtype=np.uint8), np.ascontiguousarray(points3d, dtype=np.float64).reshape(-1, 3)
    tv = _as(two_view, TWO_VIEW_DTYPE, "two_view")
    if min(len(m), len(mk), len(pts)) < total or len(tv) != n:
        raise ValueError("matches, mask and points3d cover every pair's match range; one two_view record per pair")
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    if kp is not None and len(kp) < total:
        raise ValueError("keep covers every pair's match range")
    cap = max(int(frame_off[-1]) // 2, 0) if cloud_cap is None else int(cloud_cap)
    out = sfm_outputs(n_frames, n, total, max(cap, 0))   # (a negative capacity is the C call's to refuse)
    lib = load_library()
    args = (frame_off.ctypes.data, n_frames, recs.ctypes.data, n, m.ctypes.data, mk.ctypes.data, pts.ctypes.data, tv.ctypes.data, int(root),
            int(min_links), *(out[k].ctypes.data for k in ("views", "registration", "points_world", "track")), cap,
            *(out[k].ctypes.data for k in ("cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")))
    if kp is None:
        _check(lib.gms_sfm_register(*args), lib, "gms_sfm_register")
    else:
        _check(lib.gms_sfm_register_keep(*args, kp.ctypes.data), lib, "gms_sfm_register_keep")
    out["plan"] = sfm_plan(recs, n_frames, root)
    return sfm_trim(out)


def bundleAdjust(keypoints, frame_off, pairs, matches, mask, registration, camera, dist=None, **ba):
    """gms_sfm_ba, the one-shot on host arrays (synchronous, on the current device): bundle adjustment behind registerViews (DESIGN.md
    4.10c). keypoints: KEYPOINT_DTYPE, all frames back to back; frame_off, pairs, matches, mask as registerViews took them;
    registration: its dict (views, registration, track, cloud, cloud_id, summary); camera = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3)
    or None; ba: n_iters, n_cg, lambda0, cg_tol, ftol, huber_px, retriangulate. Returns dict(views_ba SFM_VIEW_DTYPE per frame,
    cloud_ba [n, 3], track_status int32 [n], ba_summary SFM_BA_SUMMARY_DTYPE [1]), n the cloud's entries."""
    from .types import SFM_BA_SUMMARY_DTYPE, make_camera, sfm_ba_params
    frame_off = np.ascontiguousarray(frame_off, dtype=np.int64)
    recs = _as(pairs, PAIR_DTYPE, "pairs")
    kp, m = _as(keypoints, KEYPOINT_DTYPE, "keypoints"), _as(matches, DMATCH_DTYPE, "matches")
    mk = np.ascontiguousarray(mask, dtype=np.uint8)
    views, reg = _as(registration["views"], SFM_VIEW_DTYPE, "views"), _as(registration["registration"], SFM_PAIR_REG_DTYPE, "registration")
    track = np.ascontiguousarray(registration["track"], dtype=np.int32)
    cloud = np.ascontiguousarray(registration["cloud"], dtype=np.float64).reshape(-1, 3)
    ids = np.ascontiguousarray(registration["cloud_id"], dtype=np.int32)
    n_frames, n, cap = len(frame_off) - 1, len(recs), len(ids)
    total = int((recs["match_off"] + np.maximum(recs["m"], 0)).max()) if n else 0
    if min(len(m), len(mk), len(track)) < total or len(reg) != n or len(views) != n_frames or len(kp) < frame_off[-1] or len(cloud) != cap:
        raise ValueError("keypoints cover every frame; matches, mask and track every pair's match range; one record per pair and per frame")
    cam, prm = make_camera(camera, dist), sfm_ba_params(**ba)
    out = dict(views_ba=np.zeros(n_frames, SFM_VIEW_DTYPE), cloud_ba=np.zeros((cap, 3)), track_status=np.zeros(cap, np.int32),
               ba_summary=np.zeros(1, SFM_BA_SUMMARY_DTYPE))
    lib = load_library()
    _check(lib.gms_sfm_ba(cam.ctypes.data, prm.ctypes.data, kp.ctypes.data, frame_off.ctypes.data, n_frames, recs.ctypes.data, n, m.ctypes.data,
                          mk.ctypes.data, views.ctypes.data, reg.ctypes.data, track.ctypes.data, cap, cloud.ctypes.data, ids.ctypes.data,
                          int(registration["summary"]["n_tracks"][0]), out["views_ba"].ctypes.data, out["cloud_ba"].ctypes.data,
                          out["track_status"].ctypes.data, out["ba_summary"].ctypes.data), lib, "gms_sfm_ba")
    return out


def structureFromMotionMulti(images, camera, dist=None, method="gms", pairs=None, root=0, min_links=8, ctx=None, bundle=False, unique=False,
                             **params):
    """structureFromMotion for a sequence: n photographs of one size (a list, or [n, H, W] / [n, H, W, 3]) -> every pair's two-view result
    and the registration that joins them into the frame of image `root` (pipeline.run_images(..., register=True)). pairs: (frame_a,
    frame_b) rows, default the chain (i, i + 1); they are walked in order, a pair registers frame_b when frame_a is registered.
    method, camera, dist and params as structureFromMotion (method="gms" runs matchGMS(true, true)). Returns run_images' dict:
    two_view, points3d, ... per pair, and views, registration, points_world, track, cloud, cloud_obs, cloud_est, cloud_spread, summary.
    A pair without a pose does not raise here: its registration status says so, and the frames behind it stay unregistered.
    bundle=True: bundle adjustment behind the registration (gms_sfm_ba_device; its keywords n_iters, n_cg, lambda0, cg_tol, ftol,
    huber_px, retriangulate among params) adds views_ba, cloud_ba, track_status and ba_summary; bundle=False returns the dict without.
    unique=True: the tracks are built from one-to-one matches only (gms_match_unique_device in front of the registration; DESIGN.md
    4.10e), so that no track holds two keypoints of a frame (summary n_multi = 0) and the bundle adjustment excludes none for it; adds
    `keep` (uint8 per match slot) and `unique_counts` (live, kept per pair). The views are the same bytes either way. unique=False
    returns the dict without.
    dense=True among params adds `dense`, one cloud per pair in the root's frame; fuse=True beside it (fuse_tol16, fuse_min_support,
    fuse_cap: run_images') adds `dense_fused`, those clouds fused into one by depth consistency; fuse=True without
    dense=True raises ValueError. dense_speckle = (max_speckle_size, max_diff16): filterSpeckles on every pair's map before the
    reprojection; the fusion then reads the filtered maps. None, the default: no filter.
    dense_poses = "pair" (the default: each pair's own two-view pose and the registration's scale), "registration" or "bundle" (needs
    bundle=True; ValueError otherwise): the dense stage and the fusion on records derived from `views` / `views_ba`
    (gms_sfm_pair_poses_device); the dict then also holds `dense_pose_records`. dense_pairs = [(a, b), ...] (needs
    dense_poses other than "pair"): those frame pairs are matched densely in place of `pairs` -- any two registered frames, matched
    sparsely or not --, and `dense`, `dense_fused["source"]` and the fusion's neighbour table index into dense_pairs."""
    from . import pipeline
    if method not in pipeline.METHODS:
        raise ValueError(f"unknown method {method!r}")
    if params.get("fuse") and not params.get("dense"):
        raise ValueError("fuse=True needs dense=True: the fusion reads the pairs' dense clouds")
    pipeline.check_dense_poses(params.get("dense_poses", "pair"), params.get("dense_pairs"), params.get("dense", False), True, bundle)
    stack, _ = pipeline.image_stack(images)
    n = stack.shape[0]
    if pairs is None:
        pairs = [(i, i + 1) for i in range(n - 1)]
    opts = dict(params)
    if method == "gms":
        opts.setdefault("withRotation", True)
        opts.setdefault("withScale", True)
    if method == "logos" and opts.get("dictionary") is None:
        opts.setdefault("train_dictionary", True)
    return pipeline.run_images(ctx or default_context(), stack, camera, dist, method=method, pairs=pairs, register=True, root=root,
                               min_links=min_links, bundle=bundle, unique=unique, **opts)


def default_context():
    """The process-wide context of device 0 that matchGMS uses, created on first use."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = GmsContext(0)
    return _default_ctx


def _stereo_one_shot(entry, make_params, left, right, params, want16, want_cost, want8):
    lib = load_library()
    lt = np.ascontiguousarray(left, dtype=np.uint8)
    rt = np.ascontiguousarray(right, dtype=np.uint8)
    if lt.ndim != 2 or rt.shape != lt.shape:
        raise ValueError("left and right: two 8-bit grey images [H, W] of one size")
    h, w = lt.shape
    rec = make_params(params)
    d16 = np.zeros((h, w), np.int16) if want16 else None
    cost = np.zeros((h, w), np.int32) if want_cost else None
    d8 = np.zeros((h, w), np.uint8) if want8 else None
    rc = getattr(lib, entry)(rec.ctypes.data, lt.ctypes.data, rt.ctypes.data, w, h, w, None if d16 is None else d16.ctypes.data,
                             None if cost is None else cost.ctypes.data, None if d8 is None else d8.ctypes.data)
    _check(rc, lib, entry)
    return d16, cost, d8


def _stereo_bm(left, right, params, want16, want_cost, want8):
    return _stereo_one_shot("gms_stereo_bm", stereo_bm_params, left, right, params, want16, want_cost, want8)


def stereoBM(left, right, return_cost=False, **params):
    """StereoBM::compute(left, right, disparity) of OpenCV 4.5.2 on the GPU (integer path; tests/stereo_bm_ref.py states it): the int16
    map with 4 fractional bits, FILTERED = (min_disparity - 1) * 16. Parameters by keyword (block_size, num_disparities, min_disparity,
    pre_filter_cap, texture_threshold, uniqueness_ratio, disp12_max_diff, ...; types.STEREO_BM_PARAMS_DTYPE), the reference's values
    (DisparityUtil.cpp:24-36) by default. return_cost=True: also the int32 cost map (sad of the winner, -1 where there is none).
    speckle_window_size > 0 is refused: pass the map to filterSpeckles(disp16, FILTERED, size, range * 16 or any max_diff in sixteenths)."""
    d16, cost, _ = _stereo_bm(left, right, params, True, return_cost, False)
    return (d16, cost) if return_cost else d16


def stereo_match(left, right, **params):
    """The reference's stereo_match (DisparityUtil.cpp:22-49): StereoBM with its parameters, normalize(NORM_MINMAX, 0..255, CV_8U),
    every 0 -> 255. Returns the uint8 map."""
    return _stereo_bm(left, right, params, False, False, True)[2]


def _stereo_sgm(left, right, params, want_cost, want8):
    """One pair: host arrays through gms_stereo_sgm, device tensors (torch, [H, W]) through a batch of one on the default context.
    Returns (int16 map, cost or None, 8-bit map or None), arrays for arrays and tensors for tensors."""
    if hasattr(left, "data_ptr"):
        from .batch import stereo_sgm_batch
        if left.dim() != 2 or right.shape != left.shape:
            raise ValueError("left and right: two 8-bit grey images [H, W] of one size")
        outs = stereo_sgm_batch(left[None], right[None], params, None, return_cost=want_cost, eight_bit=want8)
        outs = list(outs) if isinstance(outs, tuple) else [outs]
        return outs[0][0], (outs[1][0] if want_cost else None), (outs[-1][0] if want8 else None)
    return _stereo_one_shot("gms_stereo_sgm", stereo_sgm_params, left, right, params, True, want_cost, want8)


def stereoSGM(left, right, return_cost=False, p1=None, p2=None, n_paths=8, **bm_params):
    """Semi-global matching on StereoBM's costs (tests/stereo_sgm_ref.py states it) -- the library's own definition,
    not cv::StereoSGBM: StereoBM's window SADs, aggregated along n_paths (4 or 8) directions with the penalties p1 (a disparity step of
    one; default 8 block_size^2) and p2 (a larger step; default 32 block_size^2), then StereoBM's decision rules on the sums. left /
    right: uint8 [H, W] host arrays or device tensors. Returns the int16 map with 4 fractional bits, FILTERED = (min_disparity - 1) * 16;
    return_cost=True: also the int32 cost map (the winner's sum, -1 where there is none). bm_params: StereoBM's parameters by keyword
    (types.STEREO_SGM_PARAMS_DTYPE), the reference's values by default. p1 = p2 = 0 with uniqueness_ratio = 0 gives stereoBM's map.
    speckle_window_size > 0 is refused: pass the map to filterSpeckles (new_val = FILTERED, max_diff in sixteenths of a pixel)."""
    d16, cost, _ = _stereo_sgm(left, right, dict(bm_params, p1=p1, p2=p2, n_paths=n_paths), return_cost, False)
    return (d16, cost) if return_cost else d16


def stereo_match_sgm(left, right, **params):
    """stereo_match with semi-global matching in StereoBM's place: normalize(NORM_MINMAX, 0..255, CV_8U), every 0 -> 255. Returns the
    uint8 map."""
    return _stereo_sgm(left, right, params, False, True)[2]


def portraitMode(image_bgr, disparity, detail=False, **params):
    """The image tail of the reference's createPortraitMode (DisparityUtil.cpp:317-412) on the GPU: image_bgr uint8 [H, W, 3],
    disparity uint8 [H, W] (255 = no value; what gms_disparity_device or stereo_match write) -> the portrait image uint8 [H, W, 3]:
    the photograph where one of the num_contours largest borders of the thresholded, dilated map covers it, its median blur
    elsewhere. Parameters by keyword (threshold, dilate_iterations, num_contours, median_ksize), the reference's 60, 2, 5, 15 by
    default; tests/portrait_ref.py states every step. detail=True: (out, mask, selected, blurred)."""
    lib = load_library()
    img = np.ascontiguousarray(image_bgr, dtype=np.uint8)
    disp = np.ascontiguousarray(disparity, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3 or disp.shape != img.shape[:2]:
        raise ValueError("image_bgr: uint8 [H, W, 3]; disparity: uint8 [H, W] of the same size")
    h, w = disp.shape
    rec = portrait_params(params)
    out = np.zeros((h, w, 3), np.uint8)
    mask, sel, blur = (np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w, 3), np.uint8)) if detail else (None,) * 3
    rc = lib.gms_portrait(rec.ctypes.data, img.ctypes.data, disp.ctypes.data, w, h, out.ctypes.data,
                          None if mask is None else mask.ctypes.data, None if sel is None else sel.ctypes.data,
                          None if blur is None else blur.ctypes.data)
    _check(rc, lib, "gms_portrait")
    return (out, mask, sel, blur) if detail else out


def medianBlur(image, ksize):
    """cv::medianBlur(image, ksize) on the GPU (gms_median_blur): image uint8 [H, W] or [H, W, 3], ksize odd in 3..31, border
    replicated."""
    lib = load_library()
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)) or img.size == 0:
        raise ValueError("image: uint8 [H, W], [H, W, 1] or [H, W, 3]")
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    _check(lib.gms_median_blur(img.ctypes.data, w, h, 1 if img.ndim == 2 else img.shape[2], int(ksize), out.ctypes.data), lib,
           "gms_median_blur")
    return out


def _host_image(image, who):
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)) or img.size == 0:
        raise ValueError(f"{who}: uint8 [H, W], [H, W, 1] or [H, W, 3]")
    return img, img.shape[1], img.shape[0], 1 if img.ndim == 2 else img.shape[2]


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def getRotationMatrix2D(center, angle, scale):
    """cv::getRotationMatrix2D on the host (gms_rotation_matrix_2d): the forward 2 x 3 matrix, float64; the centre is rounded to
    float32 first, as OpenCV's Point2f does."""
    lib = load_library()
    M = np.zeros((2, 3), np.float64)
    _check(lib.gms_rotation_matrix_2d(float(center[0]), float(center[1]), float(angle), float(scale), M.ctypes.data), lib,
           "gms_rotation_matrix_2d")
    return M


def resize(image, dsize):
    """cv::resize(image, dsize, INTER_LINEAR) on the GPU: image uint8 [H, W] or [H, W, 3], dsize = (width, height). A host array gives
    a host array (gms_resize); a device tensor gives a device tensor (batch.resize_images). tests/warp_ref.py states every step."""
    if _is_tensor(image):
        from .batch import resize_images
        return resize_images(image[None], dsize)[0]
    lib = load_library()
    img, w, h, c = _host_image(image, "image")
    out = np.zeros((int(dsize[1]), int(dsize[0])) + img.shape[2:], np.uint8)
    _check(lib.gms_resize(img.ctypes.data, w, h, c, out.ctypes.data, int(dsize[0]), int(dsize[1])), lib, "gms_resize")
    return out


def warpAffine(image, M, dsize):
    """cv::warpAffine(image, M, dsize, INTER_LINEAR, BORDER_CONSTANT 0) on the GPU: M the forward 2 x 3 matrix, dsize = (width,
    height). Host array -> host array (gms_warp_affine); device tensor -> device tensor (batch.warp_affine_images)."""
    M = np.ascontiguousarray(M, dtype=np.float64)
    if M.size != 6:
        raise ValueError("M: a 2 x 3 matrix")
    if _is_tensor(image):
        from .batch import warp_affine_images
        return warp_affine_images(image[None], M.reshape(1, 6), dsize)[0]
    lib = load_library()
    img, w, h, c = _host_image(image, "image")
    out = np.zeros((int(dsize[1]), int(dsize[0])) + img.shape[2:], np.uint8)
    _check(lib.gms_warp_affine(img.ctypes.data, w, h, c, M.ctypes.data, out.ctypes.data, int(dsize[0]), int(dsize[1])), lib,
           "gms_warp_affine")
    return out


def imgRotate(image, angle):
    """The reference's img_rotate (main.cpp:114-120): warpAffine by getRotationMatrix2D((w / 2., h / 2.), angle, 1) into the same
    size. 180 degrees is NOT image[::-1, ::-1]: it is that flip moved by one pixel, behind a black first row and column."""
    h, w = image.shape[:2]
    return warpAffine(image, getRotationMatrix2D((w / 2., h / 2.), angle, 1.0), (w, h))


def dense_sgm_params(params=None, **kw):
    """The matcher's record of the dense stage: types.stereo_sgm_params with min_disparity 0 and num_disparities 128 unless given."""
    vals = dict(STEREO_SGM_DENSE)
    if params is not None:
        if not isinstance(params, dict):
            return stereo_sgm_params(params, **kw)
        vals.update(params)
    vals.update(kw)
    return stereo_sgm_params(vals)


def stereoRectify(camera, dist, R, t, image_size, out_size=None):
    """The rectifying plan of a posed pair X2 = R X1 + t (gms_rectify_plan_host; host arithmetic, no GPU work; DESIGN.md 4.13;
    tests/rectify_ref.py states it): a one-record RECTIFY_PLAN_DTYPE array with R1, R2 (x_rectified = R_k x_camera_k), the new camera
    fx = fy, cx, cy of both images, the baseline B, the output size and the quarter turn chosen. camera = (fx, fy, cx, cy), dist =
    (k1, k2, p1, p2, k3) or None, image_size = (W, H); out_size None: (W, H), or (H, W) for the quarter turns. A pair that is not
    rectifiable has status GMS_ERR_NO_MODEL and zeros elsewhere. rectifyQ(plan) gives reprojectImageTo3D's Q."""
    lib = load_library()
    cam = make_camera(camera, dist)
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    plan = np.zeros(1, RECTIFY_PLAN_DTYPE)
    ow, oh = (0, 0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    _check(lib.gms_rectify_plan_host(cam.ctypes.data, R.ctypes.data, t.ctypes.data, int(image_size[0]), int(image_size[1]), ow, oh,
                                     plan.ctypes.data), lib, "gms_rectify_plan_host")
    return RectifyPlan(plan, cam)


def rectifyQ(plan):
    """reprojectImageTo3D's 4 x 4 Q of a plan, for disparities in pixels (the int16 map / 16)."""
    lib = load_library()
    plan, Q = _plan_record(plan), np.zeros((4, 4))
    _check(lib.gms_rectify_q(plan.ctypes.data, Q.ctypes.data), lib, "gms_rectify_q")
    return Q


def _plan_record(plan):
    plan = rectify_plan_records(plan)
    if len(plan) != 1:
        raise ValueError("plan: one RECTIFY_PLAN_DTYPE record")
    return plan


def rectify(image, plan, which, camera=None, dist=None, return_valid=False):
    """The rectified image of camera `which` (1 or 2) of a pair under stereoRectify's plan: uint8 [plan.out_h, plan.out_w(, 3)]; a
    pixel whose ray leaves the source is 0. The source camera is the plan's own (a RectifyPlan); camera / dist state it for a bare
    RECTIFY_PLAN_DTYPE record. Host array -> host array (gms_rectify), device tensor -> device tensor (batch.Rectify).
    return_valid=True: also the uint8 plane that is 1 where all four taps lie inside the source."""
    if camera is None and not isinstance(plan, RectifyPlan):
        raise ValueError("rectify: a RectifyPlan, or a plan record with the source camera")
    cam = plan.camera if camera is None else make_camera(camera, dist)
    plan = _plan_record(plan)
    if _is_tensor(image):
        from .batch import Rectify
        if image.dim() not in (2, 3) or (image.dim() == 3 and image.shape[2] != 3):
            raise ValueError("rectify: [H, W] or [H, W, 3]")
        ctx = default_context()
        run = Rectify(ctx, 1, (image.shape[1], image.shape[0]), (int(plan["out_w"][0]), int(plan["out_h"][0])), cam,
                      1 if image.dim() == 2 else 3, n_plans=1, device=image.device)
        run.set_plans(plan)
        out = run.run(image.contiguous()[None], which)[0]
        ctx.synchronize()
        return (out, run.d_valid[0]) if return_valid else out
    lib = load_library()
    img, w, h, c = _host_image(image, "rectify")
    ow, oh = int(plan["out_w"][0]), int(plan["out_h"][0])
    if ow < 1 or oh < 1:
        raise ValueError("rectify: the plan has no output size (a pair that is not rectifiable?)")
    out = np.zeros((oh, ow) + img.shape[2:], np.uint8)
    valid = np.zeros((oh, ow), np.uint8) if return_valid else None
    _check(lib.gms_rectify(cam.ctypes.data, plan.ctypes.data, int(which), img.ctypes.data, w, h, c, out.ctypes.data,
                           None if valid is None else valid.ctypes.data), lib, "gms_rectify")
    return (out, valid) if return_valid else out


def undistort(image, camera, dist):
    """cv::undistort(image, cameraMatrix, distCoeffs) with the new camera equal to the camera (gms_undistort): the identity plan of
    the rectifying kernel. Host array -> host array, device tensor -> device tensor."""
    cam = make_camera(camera, dist)
    if _is_tensor(image):
        plan = np.zeros(1, RECTIFY_PLAN_DTYPE)
        plan["R1"][0] = plan["R2"][0] = np.eye(3)
        plan["fx"], plan["fy"], plan["cx"], plan["cy"] = [float(v) for v in camera]
        plan["out_w"], plan["out_h"] = int(image.shape[1]), int(image.shape[0])
        return rectify(image, plan, 1, camera, dist if dist is not None else np.zeros(5))
    lib = load_library()
    img, w, h, c = _host_image(image, "undistort")
    out = np.zeros_like(img)
    _check(lib.gms_undistort(cam.ctypes.data, img.ctypes.data, w, h, c, out.ctypes.data), lib, "gms_undistort")
    return out


def _speckle_pair(speckle, who):
    """speckle=None | (max_speckle_size, max_diff16) -> (size, diff16); None is (0, 0), the unfiltered stage."""
    if speckle is None:
        return 0, 0
    size, diff = (_c_int(v) for v in speckle)
    if size < 0 or diff < 0:
        raise GmsError(GMS_ERR_BAD_ARG, f"{who}: speckle = (max_speckle_size >= 0, max_diff16 >= 0)")
    return size, diff


def filterSpeckles(disp16, new_val, max_speckle_size, max_diff, return_removed=False):
    """cv::filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) for an int16 map [H, W] on the GPU (DESIGN.md 4.13c;
    tests/speckle_ref.py states it): pixels are linked when they are 4-neighbours, neither equals new_val and |a - b| <= max_diff
    (taken in 32 bits); every pixel that is not new_val and whose component has at most max_speckle_size pixels becomes new_val.
    max_diff is in the map's own units: sixteenths of a pixel for stereoBM's / stereoSGM's maps, whose new_val is their FILTERED code
    (min_disparity - 1) * 16. A host array gives a new host array (gms_filter_speckles); a device tensor (int16, contiguous) is
    filtered in place and returned (batch.SpeckleFilter). return_removed=True: also the number of pixels changed."""
    if _is_tensor(disp16):
        from .batch import filter_speckles_batch
        if disp16.dim() != 2:
            raise ValueError("filterSpeckles: an int16 map [H, W]")
        _, removed = filter_speckles_batch(disp16[None], new_val, max_speckle_size, max_diff, return_removed=True)
        return (disp16, int(removed[0])) if return_removed else disp16
    src = np.asarray(disp16)
    if src.dtype != np.int16 or src.ndim != 2 or src.size == 0:
        raise ValueError("filterSpeckles: an int16 map [H, W]")
    lib = load_library()
    out = np.array(src, dtype=np.int16, order="C", copy=True)
    removed = np.zeros(1, np.int32)
    _check(lib.gms_filter_speckles(out.ctypes.data, out.shape[1], out.shape[0], _c_int(new_val), _c_int(max_speckle_size), _c_int(max_diff),
                                   removed.ctypes.data), lib, "gms_filter_speckles")
    return (out, int(removed[0])) if return_removed else out


def denseStereo(img1, img2, camera, dist, R, t, min_disp16=16, out_size=None, cap=None, speckle=None, **sgm_params):
    """A dense, coloured cloud from a posed pair X2 = R X1 + t: stereoRectify's plan, both images rectified, stereoSGM
    on the rectified pair, every matched pixel reprojected into camera 1's frame in the unit of t -- the frame and unit of
    structureFromMotion's points3D. img1 / img2: uint8 [H, W] or [H, W, 3] BGR of one size, host arrays (gms_dense_pair) or device
    tensors (batch.DensePairs). sgm_params: stereoSGM's keywords; min_disparity 0 and num_disparities 128 unless given. cap: the most
    points returned (default: every pixel). Returns a dict: points float32 [k, 3], colors uint8 [k] or [k, 3], pixel int32 [k]
    (v * out_w + u of the rectified image, raster order), disp16 int16, rect1, rect2, valid (camera 1's), plan, count (all the points,
    also beyond cap). speckle = (max_speckle_size, max_diff16): filterSpeckles on the matcher's map before the reprojection, max_diff16 in
    sixteenths of a pixel; the dict then also holds removed. None: no filter. A pair that is not rectifiable raises
    GmsError(GMS_ERR_NO_MODEL)."""
    spk_size, spk_diff = _speckle_pair(speckle, "denseStereo")
    shapes = [tuple(im.shape) for im in (img1, img2)]
    if len(shapes[0]) not in (2, 3) or (len(shapes[0]) == 3 and shapes[0][2] != 3) or shapes[0] != shapes[1]:
        raise ValueError("img1 / img2: [H, W] grey or [H, W, 3] BGR, one size")
    if int(min_disp16) < 1:
        raise GmsError(GMS_ERR_BAD_ARG, "denseStereo: min_disp16 >= 1")
    h, w = shapes[0][:2]
    c = 1 if len(shapes[0]) == 2 else 3
    plan = stereoRectify(camera, dist, R, t, (w, h), out_size)
    if not plan.ok:
        raise GmsError(int(plan["status"]), "denseStereo: the pair is not rectifiable")
    ow, oh = plan.out_size
    cap = ow * oh if cap is None else int(cap)
    rec = dense_sgm_params(sgm_params)
    if _is_tensor(img1):
        from .batch import DensePairs
        import torch
        ctx = default_context()
        run = DensePairs(ctx, 1, (w, h), (ow, oh), camera, dist, c, cap=cap, min_disp16=min_disp16, params=rec, device=img1.device,
                         speckle=speckle)
        tv = np.zeros(1, TWO_VIEW_DTYPE)
        tv["R"][0], tv["t"][0] = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
        run.set_two_view(tv)
        torch.cuda.synchronize(img1.device)
        run.run(img1.contiguous()[None], img2.contiguous()[None])
        ctx.synchronize()
        k = min(int(run.d_count[0]), cap)
        more = {} if speckle is None else dict(removed=int(run.d_removed[0]))
        return dict(points=run.d_xyz[0, :k], colors=run.d_cloud_color[0, :k] if c == 3 else run.d_cloud_color[0, :k, 0], pixel=run.d_pixel[0, :k],
                    disp16=run.d_disp16[0], rect1=run.d_color[0] if c == 3 else run.d_rect1[0], rect2=run.d_rect2[0], valid=run.d_valid[0],
                    plan=plan, count=int(run.d_count[0]), **more)
    lib = load_library()
    cam = make_camera(camera, dist)
    a, b = np.ascontiguousarray(img1, dtype=np.uint8), np.ascontiguousarray(img2, dtype=np.uint8)
    Rv, tvec = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    rect1, rect2, valid = (np.zeros((oh, ow), np.uint8) for _ in range(3))
    color = np.zeros((oh, ow, 3), np.uint8) if c == 3 else None
    disp16 = np.zeros((oh, ow), np.int16)
    xyz, cc, pixel = np.zeros((max(cap, 1), 3), np.float32), np.zeros((max(cap, 1), c), np.uint8), np.zeros(max(cap, 1), np.int32)
    count = np.zeros(1, np.int32)
    out_plan = np.zeros(1, RECTIFY_PLAN_DTYPE)
    args = (cam.ctypes.data, rec.ctypes.data, a.ctypes.data, b.ctypes.data, w, h, c, Rv.ctypes.data, tvec.ctypes.data, ow, oh, int(min_disp16),
            out_plan.ctypes.data, rect1.ctypes.data, rect2.ctypes.data, valid.ctypes.data, None if color is None else color.ctypes.data,
            disp16.ctypes.data, cap, xyz.ctypes.data, cc.ctypes.data, pixel.ctypes.data, count.ctypes.data)
    more = {}
    if speckle is None:
        _check(lib.gms_dense_pair(*args), lib, "gms_dense_pair")
    else:
        removed = np.zeros(1, np.int32)
        _check(lib.gms_dense_pair_filtered(*args, spk_size, spk_diff, removed.ctypes.data), lib, "gms_dense_pair_filtered")
        more = dict(removed=int(removed[0]))
    k = min(int(count[0]), cap)
    return dict(points=xyz[:k], colors=cc[:k] if c == 3 else cc[:k, 0], pixel=pixel[:k], disp16=disp16, rect1=color if c == 3 else rect1,
                rect2=rect2, valid=valid, plan=RectifyPlan(out_plan, cam), count=int(count[0]), **more)


def denseFuse(sources, neighbors=None, tol16=16, min_support=1, fused_cap=None):
    """The clouds of several posed pairs fused into one by depth consistency (gms_dense_fuse on host arrays). A point
    of source i is looked up in each neighbour j: moved into j's rectified camera 1 and compared with the disparity j's own map
    holds at the pixel it falls on (nearest pixel; within tol16 sixteenths of a pixel: CONSISTENT, else CONFLICT; no valid disparity
    there, outside the map or behind the camera: UNSEEN). support = 1 + the consistent neighbours, conflict = the conflicting ones; a
    point is dropped when a consistent neighbour has a lower index (that source owns it) or support < min_support. A rule per point,
    not a clustering: the lower copy of a dropped point is not guaranteed to be kept. Positions are not averaged.
    sources: dicts of disp16 int16 [H, W], valid uint8 [H, W], plan (a RectifyPlan or a 200-byte record), points float32 [cap, 3],
    filtered16 (the matcher's FILTERED code, (min_disparity - 1) * 16; default -16), min_disp16 (default 16), and optionally colors
    uint8 [cap] or [cap, 3], count (default cap), view ((R, t) of the pair's frame_a, x_camera = R x_world + t, or an SFM_VIEW_DTYPE
    record; default identity) and reg ((S, status) or an SFM_PAIR_REG_DTYPE record; default S = 1, ok) -- what denseStereo returns
    holds the first four. neighbors: types.dense_fuse_neighbors' table (default every other source; more than 33 sources need one).
    Returns a dict: points float32 [k, 3], colors uint8 [k] or [k, 3], source, index int32 [k] (the source and the point's index in
    it), support, conflict uint8 [k], counts int32 [n + 1] (kept per source, then the total, also beyond fused_cap)."""
    n = len(sources)
    if n < 1:
        raise ValueError("denseFuse: at least one source")
    nb = dense_fuse_neighbors(n, neighbors)
    if int(min_support) < 1 or int(tol16) < 0:
        raise GmsError(GMS_ERR_BAD_ARG, "denseFuse: min_support >= 1 and tol16 >= 0")
    tab, keep = np.zeros(n, DENSE_FUSE_SRC_DTYPE), []
    channels = None
    for i, s in enumerate(sources):
        disp, valid = np.ascontiguousarray(s["disp16"], dtype=np.int16), np.ascontiguousarray(s["valid"], dtype=np.uint8)
        if disp.ndim != 2 or disp.shape != valid.shape:
            raise ValueError("denseFuse: disp16 and valid [H, W]")
        xyz = np.ascontiguousarray(s["points"], dtype=np.float32).reshape(-1, 3)
        plan, count = rectify_plan_records(s["plan"])[:1], np.array([s.get("count", len(xyz))], np.int32)
        row = [disp, valid, plan, xyz, None, count, None, None]
        if s.get("colors") is not None:
            col = np.ascontiguousarray(s["colors"], dtype=np.uint8).reshape(len(xyz), -1)
            if col.shape[1] not in (1, 3) or channels not in (None, col.shape[1]):
                raise ValueError("denseFuse: colors uint8 [cap] or [cap, 3], the same for every source that has them")
            channels, row[4] = col.shape[1], col
        if s.get("view") is not None:
            row[6] = sfm_view_record(s["view"])
        if s.get("reg") is not None:
            row[7] = sfm_pair_reg_record(s["reg"])
        keep.append(row)
        for name, a in zip(DENSE_FUSE_SRC_DTYPE.names[:8], row):
            tab[name][i] = 0 if a is None else a.ctypes.data
        tab["width"][i], tab["height"][i], tab["cap"][i] = disp.shape[1], disp.shape[0], len(xyz)
        tab["filtered16"][i], tab["min_disp16"][i] = int(s.get("filtered16", -16)), int(s.get("min_disp16", 16))
    c = channels or 1
    cap = int(tab["cap"].sum()) if fused_cap is None else int(fused_cap)
    if cap < 0:
        raise GmsError(GMS_ERR_BAD_ARG, "denseFuse: fused_cap >= 0")
    k1 = max(cap, 1)
    xyz, col, src, idx = np.zeros((k1, 3), np.float32), np.zeros((k1, c), np.uint8), np.zeros(k1, np.int32), np.zeros(k1, np.int32)
    sup, con, counts = np.zeros(k1, np.uint8), np.zeros(k1, np.uint8), np.zeros(n + 1, np.int32)
    lib = load_library()
    _check(lib.gms_dense_fuse(tab.ctypes.data, n, nb.ctypes.data, nb.shape[1], c, int(tol16), int(min_support), cap, xyz.ctypes.data, col.ctypes.data,
                              src.ctypes.data, idx.ctypes.data, sup.ctypes.data, con.ctypes.data, counts.ctypes.data), lib, "gms_dense_fuse")
    k = min(int(counts[n]), cap)
    return dict(points=xyz[:k], colors=col[:k] if c == 3 else col[:k, 0], source=src[:k], index=idx[:k], support=sup[:k], conflict=con[:k],
                counts=counts)


def _grey_host(image, who):
    img = np.ascontiguousarray(image, dtype=np.uint8)
    if img.ndim != 2 or img.size == 0:
        raise ValueError(f"{who}: an 8-bit grey image [H, W]")
    return img


def findChessboardCorners(image, patternSize):
    """(found, corners) for a grey image [H, W] and patternSize = (nx points per row, ny rows), nx != ny: the library's own finder
    (NOT OpenCV's quad-based one): the nx * ny strongest saddle-response peaks (gms_chess_candidates_device's), ordered
    onto the board. corners: float32 [nx * ny, 2] in findChessboardCorners' order (row by row; of the two half turns the one whose
    first point is smaller in (y, x); never mirrored), or None. tests/calib_ref.py states every step."""
    lib = load_library()
    img = _grey_host(image, "image")
    nx, ny = int(patternSize[0]), int(patternSize[1])
    found = C.c_int(0)
    corners = np.zeros((max(nx * ny, 1), 2), np.float32)
    _check(lib.gms_find_chessboard_corners(img.ctypes.data, img.shape[1], img.shape[0], nx, ny, C.byref(found), corners.ctypes.data), lib,
           "gms_find_chessboard_corners")
    return (True, corners) if found.value else (False, None)


def cornerSubPix(image, corners, win=(5, 5), criteria=(30, 0.1), return_status=False):
    """cv::cornerSubPix(image, corners, win, (-1, -1), TermCriteria(MAX_ITER + EPS, *criteria)) on the GPU, OpenCV 4.5.2's algorithm
    in fp64 (gms_corner_subpix): corners [n, 2] -> float64 [n, 2]. win must be (5, 5). A start whose 13 x 13 patch of samples leaves
    the image is refused (GmsError, bad argument). return_status: also the int32 status per corner (include/gms.h)."""
    lib = load_library()
    img = _grey_host(image, "image")
    if tuple(int(v) for v in win) != (5, 5):
        raise ValueError("win: (5, 5), the window whose mask is committed")
    pts = np.array(corners, dtype=np.float64).reshape(-1, 2)
    status = np.zeros(max(len(pts), 1), np.int32)
    _check(lib.gms_corner_subpix(img.ctypes.data, img.shape[1], img.shape[0], pts.ctypes.data, len(pts), 5, int(criteria[0]), float(criteria[1]),
                                 status.ctypes.data), lib, "gms_corner_subpix")
    return (pts, status[:len(pts)]) if return_status else pts


def calibrateCamera(object_points, image_points, image_size):
    """cv::calibrateCamera(objectPoints, imagePoints, imageSize, K, dist, rvecs, tvecs) with flags = 0, on the host in fp64
    (gms_calibrate_camera; 540 points and 69 parameters are no work for a GPU): object_points, image_points: one [m, 3] / [m, 2] array
    per view; image_size = (width, height). Returns (rms, K [3, 3], dist [5] = (k1, k2, p1, p2, k3), rvecs [n, 3], tvecs [n, 3])."""
    lib = load_library()
    obj = [np.asarray(o, dtype=np.float64).reshape(-1, 3) for o in object_points]
    img = [np.asarray(i, dtype=np.float64).reshape(-1, 2) for i in image_points]
    if len(obj) == 0 or len(obj) != len(img) or any(len(o) != len(i) for o, i in zip(obj, img)):
        raise ValueError("object_points, image_points: one array per view, of equal lengths")
    counts = np.array([len(o) for o in obj], np.int32)
    o, i = np.ascontiguousarray(np.concatenate(obj)), np.ascontiguousarray(np.concatenate(img))
    n = len(obj)
    K, dist, rv, tv, rms = np.zeros((3, 3)), np.zeros(5), np.zeros((n, 3)), np.zeros((n, 3)), C.c_double(0)
    _check(lib.gms_calibrate_camera(o.ctypes.data, i.ctypes.data, counts.ctypes.data, n, int(image_size[0]), int(image_size[1]), K.ctypes.data,
                                    dist.ctypes.data, rv.ctypes.data, tv.ctypes.data, C.byref(rms)), lib, "gms_calibrate_camera")
    return float(rms.value), K, dist, rv, tv


def chessboardObjectPoints(board_size):
    """The reference's object points (CalibrationUtil.cpp:13-17): point i * nx + j is (i, j, 0)."""
    nx, ny = int(board_size[0]), int(board_size[1])
    i, j = np.mgrid[0:ny, 0:nx]
    return np.stack([i.ravel(), j.ravel(), np.zeros(nx * ny)], 1).astype(np.float64)


def addChessboardPoints(images, board_size):
    """The reference's addChessboardPoints (CalibrationUtil.cpp:3-53): findChessboardCorners, then cornerSubPix((5, 5), (-1, -1),
    (30, 0.1)), per grey image; images where the board is not found are skipped. Returns (successes, object_points, image_points):
    one [nx * ny, 3] and one [nx * ny, 2] float64 array per success."""
    obj, img = [], []
    for im in images:
        found, corners = findChessboardCorners(im, board_size)
        if not found:
            continue
        img.append(cornerSubPix(im, corners, (5, 5), (30, 0.1)))
        obj.append(chessboardObjectPoints(board_size))
    return len(img), obj, img
