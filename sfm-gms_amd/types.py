"""PODs shared with the C ABI (include/gms.h), as numpy structured dtypes."""
import numpy as np

# cv::KeyPoint, 28 bytes (stride 0x1c at DLL@0x1800485d4); GMS reads only x, y.
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
# cv::DMatch, 16 bytes (stride 0x10 at DLL@0x180046aa3); copied verbatim to the output.
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
PAIR_DTYPE = np.dtype([("frame_a", "<i4"), ("frame_b", "<i4"), ("m", "<i4"), ("reserved", "<i4"),
                       ("match_off", "<i8")])
RESULT_DTYPE = np.dtype([("n_inliers", "<i4"), ("best_scale", "<i4"), ("best_rot", "<i4"), ("status", "<i4")])

assert KEYPOINT_DTYPE.itemsize == 28 and DMATCH_DTYPE.itemsize == 16
assert PAIR_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 16
# gms_logos_result (include/gms.h): one LOGOS pair's counts, peak bin and status
LOGOS_RESULT_DTYPE = np.dtype([("n_candidates", "<i8"), ("n_supported", "<i8"), ("n_out", "<i8"), ("peak_bin", "<i4"), ("status", "<i4")])
assert LOGOS_RESULT_DTYPE.itemsize == 32
# gms_logos_dict_result (include/gms.h): one training set's status, winning attempt, assignments run, empty words and compactness
LOGOS_DICT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("attempt", "<i4"), ("iterations", "<i4"), ("empty_clusters", "<i4"),
                                    ("compactness", "<u8")])
assert LOGOS_DICT_RESULT_DTYPE.itemsize == 24
# gms_bf_result (include/gms.h): one bruteForceMatch pair's candidate count, count within the ratio, survivors, d_min and status
BF_RESULT_DTYPE = np.dtype([("n_candidates", "<i8"), ("n_ratio", "<i8"), ("n_out", "<i8"), ("d_min", "<f4"), ("status", "<i4")])
assert BF_RESULT_DTYPE.itemsize == 32

# gms_stereo_bm_params (include/gms.h): StereoBM's parameters, eleven int32 in this order
STEREO_BM_PARAMS_DTYPE = np.dtype([(n, "<i4") for n in (
    "block_size", "num_disparities", "min_disparity", "pre_filter_type", "pre_filter_size", "pre_filter_cap", "texture_threshold",
    "uniqueness_ratio", "speckle_window_size", "speckle_range", "disp12_max_diff")])
assert STEREO_BM_PARAMS_DTYPE.itemsize == 44
GMS_STEREO_BM_PREFILTER_NORMALIZED_RESPONSE, GMS_STEREO_BM_PREFILTER_XSOBEL = 0, 1
# GMS_STEREO_BM_PARAMS_REFERENCE: the reference's StereoBM (DisparityUtil.cpp:24-36)
STEREO_BM_REFERENCE = dict(block_size=5, num_disparities=224, min_disparity=-39, pre_filter_type=GMS_STEREO_BM_PREFILTER_XSOBEL,
                           pre_filter_size=5, pre_filter_cap=61, texture_threshold=507, uniqueness_ratio=0, speckle_window_size=0,
                           speckle_range=8, disp12_max_diff=1)


def stereo_bm_params(params=None, **kw):
    """A one-record STEREO_BM_PARAMS_DTYPE array: the reference's values, updated from params (a dict or a record) and keywords."""
    rec = np.zeros(1, STEREO_BM_PARAMS_DTYPE)
    vals = dict(STEREO_BM_REFERENCE)
    if params is not None:
        vals.update(params if isinstance(params, dict) else {n: int(np.asarray(params).reshape(-1)[0][n]) for n in STEREO_BM_PARAMS_DTYPE.names})
    vals.update(kw)
    for k, v in vals.items():
        if k not in STEREO_BM_PARAMS_DTYPE.names:
            raise TypeError(f"unknown StereoBM parameter {k!r}")
        rec[k] = int(v)
    return rec


# gms_stereo_sgm_params (include/gms.h): StereoBM's eleven, then p1, p2, n_paths
STEREO_SGM_PARAMS_DTYPE = np.dtype([(n, "<i4") for n in STEREO_BM_PARAMS_DTYPE.names + ("p1", "p2", "n_paths")])
assert STEREO_SGM_PARAMS_DTYPE.itemsize == 56


def stereo_sgm_params(params=None, **kw):
    """A one-record STEREO_SGM_PARAMS_DTYPE array: the reference's StereoBM values, eight paths, p1 = 8 block_size^2 and
    p2 = 32 block_size^2 unless given (None means the default), updated from params (a dict or a record) and keywords."""
    vals = {}
    if params is not None:
        vals.update(params if isinstance(params, dict) else {n: int(np.asarray(params).reshape(-1)[0][n]) for n in STEREO_SGM_PARAMS_DTYPE.names})
    vals.update(kw)
    own = {k: vals.pop(k, None) for k in ("p1", "p2", "n_paths")}
    rec = np.zeros(1, STEREO_SGM_PARAMS_DTYPE)
    bm = stereo_bm_params(vals)
    for n in STEREO_BM_PARAMS_DTYPE.names:
        rec[n] = bm[n]
    bs2 = int(bm["block_size"][0]) ** 2
    rec["p1"] = 8 * bs2 if own["p1"] is None else int(own["p1"])
    rec["p2"] = 32 * bs2 if own["p2"] is None else int(own["p2"])
    rec["n_paths"] = 8 if own["n_paths"] is None else int(own["n_paths"])
    return rec

# gms_portrait_params (include/gms.h): portrait mode's parameters, four int32 in this order; the reference's values
# (DisparityUtil.cpp:341, :351, :380, :394)
PORTRAIT_PARAMS_DTYPE = np.dtype([(n, "<i4") for n in ("threshold", "dilate_iterations", "num_contours", "median_ksize")])
assert PORTRAIT_PARAMS_DTYPE.itemsize == 16
PORTRAIT_REFERENCE = dict(threshold=60, dilate_iterations=2, num_contours=5, median_ksize=15)


def portrait_params(params=None, **kw):
    """A one-record PORTRAIT_PARAMS_DTYPE array: the reference's values, updated from params (a dict or a record) and keywords."""
    rec = np.zeros(1, PORTRAIT_PARAMS_DTYPE)
    vals = dict(PORTRAIT_REFERENCE)
    if params is not None:
        vals.update(params if isinstance(params, dict) else {n: int(np.asarray(params).reshape(-1)[0][n]) for n in PORTRAIT_PARAMS_DTYPE.names})
    vals.update(kw)
    for k, v in vals.items():
        if k not in PORTRAIT_PARAMS_DTYPE.names:
            raise TypeError(f"unknown portrait parameter {k!r}")
        rec[k] = int(v)
    return rec


GMS_OK, GMS_ERR_BAD_ARG, GMS_ERR_DOMAIN, GMS_ERR_HIP, GMS_ERR_NO_DEVICE, GMS_ERR_CAPACITY = 0, -1, -2, -3, -4, -5
GMS_ERR_NOT_RESERVED, GMS_ERR_IO, GMS_ERR_NO_MODEL = -6, -7, -8
GMS_DETECT_BORDER = 16   # include/gms.h: keypoints of gms_detect_batch_device sit at least this far from every edge


class GmsError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = int(code)
        super().__init__(f"gms error {code}: {what}")

# descriptor kinds of the brute-force matcher (include/gms.h)
GMS_DESC_HAMMING256, GMS_DESC_L2_F32X128 = 0, 1


def desc_layout(kind):
    """(row dtype, row width) of a descriptor kind: uint8 x 32 (ORB) or float32 x 128 (SIFT)."""
    if int(kind) not in (GMS_DESC_HAMMING256, GMS_DESC_L2_F32X128):
        raise ValueError("kind: GMS_DESC_HAMMING256 or GMS_DESC_L2_F32X128")
    return (np.uint8, 32) if int(kind) == GMS_DESC_HAMMING256 else (np.float32, 128)


def concat_frames(keypoints_per_frame):
    """Per-frame KEYPOINT_DTYPE arrays -> (all keypoints back to back, frame_off int64 [n_frames + 1])."""
    frame_off = np.concatenate([[0], np.cumsum([len(k) for k in keypoints_per_frame])]).astype(np.int64)
    kp = (np.concatenate([np.ascontiguousarray(k, dtype=KEYPOINT_DTYPE) for k in keypoints_per_frame])
          if frame_off[-1] else np.zeros(0, dtype=KEYPOINT_DTYPE))
    return kp, frame_off

# gms_disparity_stats (include/gms.h)
DISPARITY_STATS_DTYPE = np.dtype([("count", "<i8"), ("sum_sq", "<i8"), ("max_abs", "<i4"), ("status", "<i4")])
assert DISPARITY_STATS_DTYPE.itemsize == 24
TRIANGULATION_STATS_DTYPE = np.dtype([("sum_sq_err1", "<f8"), ("sum_sq_err2", "<f8"), ("count", "<i8"), ("behind", "<i8")])
POSE_DTYPE = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("n_good", "<i4"), ("which", "<i4")])
assert POSE_DTYPE.itemsize == 104

# gms_camera / gms_two_view (include/gms.h): the batched two-view stage (SfMUtil.cpp:25-82)
CAMERA_DTYPE = np.dtype([("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("k1", "<f8"), ("k2", "<f8"), ("p1", "<f8"),
                         ("p2", "<f8"), ("k3", "<f8")])
TWO_VIEW_DTYPE = np.dtype([("E", "<f8", (3, 3)), ("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("sum_sq_err1", "<f8"), ("sum_sq_err2", "<f8"),
                           ("n_finite", "<i8"), ("n_behind", "<i8"), ("n_points", "<i4"), ("n_ransac", "<i4"), ("ransac_iters", "<i4"),
                           ("n_pose", "<i4"), ("pose_which", "<i4"), ("n_triangulated", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
assert CAMERA_DTYPE.itemsize == 72 and TWO_VIEW_DTYPE.itemsize == 232

# gms_sfm_plan_entry / gms_sfm_view / gms_sfm_pair_reg / gms_sfm_summary (include/gms.h): many views into one frame
GMS_SFM_SKIPPED = 1
SFM_PLAN_DTYPE = np.dtype([("registers", "<i4"), ("link", "<i4"), ("role", "<i4"), ("depth", "<i4")])
SFM_VIEW_DTYPE = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("registered", "<i4"), ("pair", "<i4")])
SFM_PAIR_REG_DTYPE = np.dtype([("r", "<f8"), ("S", "<f8"), ("n_links", "<i4"), ("depth", "<i4"), ("link", "<i4"), ("role", "<i4"),
                               ("status", "<i4"), ("reserved", "<i4")])
SFM_SUMMARY_DTYPE = np.dtype([("n_tracks", "<i8"), ("n_points", "<i8"), ("n_multi", "<i8"), ("n_registered", "<i4"), ("n_ok_pairs", "<i4")])
assert SFM_PLAN_DTYPE.itemsize == 16 and SFM_VIEW_DTYPE.itemsize == 104 and SFM_PAIR_REG_DTYPE.itemsize == 40
assert SFM_SUMMARY_DTYPE.itemsize == 32

# gms_sfm_ba_params / gms_sfm_ba_summary (include/gms.h): bundle adjustment behind the registration; the track statuses
SFM_BA_PARAMS_DTYPE = np.dtype([("lambda0", "<f8"), ("cg_tol", "<f8"), ("ftol", "<f8"), ("huber_px", "<f8"), ("n_iters", "<i4"), ("n_cg", "<i4"),
                                ("retriangulate", "<i4"), ("reserved", "<i4")])
SFM_BA_SUMMARY_DTYPE = np.dtype([("cost0", "<f8"), ("cost", "<f8"), ("rms0_px", "<f8"), ("rms_px", "<f8"), ("lambda", "<f8"), ("n_obs", "<i8"),
                                 ("n_active", "<i8"), ("n_tracks_used", "<i8"), ("n_tracks_multi", "<i8"), ("n_frames_free", "<i4"),
                                 ("iters_run", "<i4"), ("iters_accepted", "<i4"), ("cg_iters", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
assert SFM_BA_PARAMS_DTYPE.itemsize == 48 and SFM_BA_SUMMARY_DTYPE.itemsize == 96
SFM_BA_REFINED, SFM_BA_MULTI, SFM_BA_FEW, SFM_BA_KEPT = 0, 1, 2, 3
SFM_BA_DEFAULTS = dict(n_iters=10, n_cg=50, lambda0=1e-3, cg_tol=1e-8, ftol=1e-10, huber_px=2.0, retriangulate=1)


def sfm_ba_params(**kw):
    """A one-record SFM_BA_PARAMS_DTYPE array: the definition's defaults, updated from the keywords."""
    rec = np.zeros(1, SFM_BA_PARAMS_DTYPE)
    for k, v in dict(SFM_BA_DEFAULTS, **kw).items():
        if k not in SFM_BA_DEFAULTS:
            raise TypeError(f"unknown bundle adjustment parameter {k!r}")
        rec[k] = v
    return rec


# gms_rectify_plan (include/gms.h): the rectifying rotations and the new camera of a posed pair
RECTIFY_PLAN_DTYPE = np.dtype([("R1", "<f8", (3, 3)), ("R2", "<f8", (3, 3)), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("B", "<f8"),
                               ("out_w", "<i4"), ("out_h", "<i4"), ("turn", "<i4"), ("status", "<i4")])
assert RECTIFY_PLAN_DTYPE.itemsize == 200


def rectify_plan_records(plans):
    """RECTIFY_PLAN_DTYPE records [n] from a RectifyPlan, an array of 200-byte plan records of any field layout (their bytes are
    taken as they are: numpy's cast between record types would go field by field), or a list of those."""
    if isinstance(plans, (list, tuple)):
        return np.concatenate([rectify_plan_records(p) for p in plans])
    a = np.ascontiguousarray(plans.record if isinstance(plans, RectifyPlan) else plans)
    if a.dtype.itemsize != RECTIFY_PLAN_DTYPE.itemsize:
        raise ValueError("plans: gms_rectify_plan records (200 bytes each)")
    return a.reshape(-1).view(np.uint8).view(RECTIFY_PLAN_DTYPE).copy()


class RectifyPlan:
    """A gms_rectify_plan record (`record`, one RECTIFY_PLAN_DTYPE entry; plan["R1"] etc. read it) with the source camera it was
    made for (`camera`, a CAMERA_DTYPE record), so that rectify(image, plan, which) needs nothing else."""

    def __init__(self, record, camera):
        self.record = rectify_plan_records(record).reshape(1)
        self.camera = np.ascontiguousarray(camera, dtype=CAMERA_DTYPE).reshape(1)

    def __getitem__(self, key):
        return self.record[key][0]

    @property
    def ok(self):
        return int(self.record["status"][0]) == GMS_OK

    @property
    def out_size(self):
        return int(self.record["out_w"][0]), int(self.record["out_h"][0])


# gms_dense_fuse_src (include/gms.h): one pair's output of the dense stage as the fusion reads it; the first eight fields are pointers
DENSE_FUSE_SRC_DTYPE = np.dtype([("d_disp16", "<u8"), ("d_valid", "<u8"), ("d_plan", "<u8"), ("d_xyz", "<u8"), ("d_color", "<u8"), ("d_count", "<u8"),
                                 ("d_view", "<u8"), ("d_reg", "<u8"), ("width", "<i4"), ("height", "<i4"), ("filtered16", "<i4"),
                                 ("min_disp16", "<i4"), ("cap", "<i4"), ("reserved", "<i4")])
assert DENSE_FUSE_SRC_DTYPE.itemsize == 88
DENSE_FUSE_MAX_NEIGHBORS = 32


def dense_fuse_neighbors(n_src, neighbors=None):
    """The fusion's neighbour table, int32 [n_src, n_nb] with 1 <= n_nb <= 32 (-1: an empty slot). None: every other source, which
    needs n_src - 1 <= 32; beyond that the caller chooses (ValueError otherwise). For j > i the table should list i for j whenever it
    lists j for i: source j drops its copy of a point only when it looks at source i, so a one-sided entry lets duplicates survive."""
    if neighbors is None:
        if n_src - 1 > DENSE_FUSE_MAX_NEIGHBORS:
            raise ValueError(f"{n_src} sources: more than {DENSE_FUSE_MAX_NEIGHBORS} others each, pass neighbors=")
        nb = np.full((n_src, max(n_src - 1, 1)), -1, np.int32)
        for i in range(n_src):
            nb[i, :n_src - 1] = [j for j in range(n_src) if j != i]
        return nb
    nb = np.ascontiguousarray(neighbors, dtype=np.int32)
    if nb.ndim != 2 or nb.shape[0] != n_src or not 1 <= nb.shape[1] <= DENSE_FUSE_MAX_NEIGHBORS:
        raise ValueError(f"neighbors: int32 [{n_src}, 1..{DENSE_FUSE_MAX_NEIGHBORS}]")
    return nb


def sfm_view_record(view):
    """One SFM_VIEW_DTYPE record from a record, or from (R, t) / (R, t, registered)."""
    if isinstance(view, np.ndarray) and view.dtype.itemsize == SFM_VIEW_DTYPE.itemsize and view.dtype.names:
        return np.ascontiguousarray(view).reshape(-1)[:1].view(np.uint8).view(SFM_VIEW_DTYPE).copy()
    G = np.zeros(1, SFM_VIEW_DTYPE)
    G["R"][0], G["t"][0] = np.asarray(view[0], dtype=np.float64).reshape(3, 3), np.asarray(view[1], dtype=np.float64).reshape(3)
    G["registered"], G["pair"] = (int(view[2]) if len(view) > 2 else 1), -1
    return G


def sfm_pair_reg_record(reg):
    """One SFM_PAIR_REG_DTYPE record from a record, or from (S, status)."""
    if isinstance(reg, np.ndarray) and reg.dtype.itemsize == SFM_PAIR_REG_DTYPE.itemsize and reg.dtype.names:
        return np.ascontiguousarray(reg).reshape(-1)[:1].view(np.uint8).view(SFM_PAIR_REG_DTYPE).copy()
    r = np.zeros(1, SFM_PAIR_REG_DTYPE)
    r["S"], r["status"] = float(reg[0]), int(reg[1])
    return r


# GMS_STEREO_SGM_PARAMS_DENSE: the matcher's record of the dense stage (the shared principal point makes true disparities positive)
STEREO_SGM_DENSE = dict(min_disparity=0, num_disparities=128)


def make_camera(camera, dist=None):
    """(fx, fy, cx, cy) and (k1, k2, p1, p2, k3) or None -> a CAMERA_DTYPE record (cameraMatrix / distCoeffs of SfMUtil.cpp:4)."""
    c = np.zeros(1, dtype=CAMERA_DTYPE)
    c["fx"], c["fy"], c["cx"], c["cy"] = camera
    if dist is not None:
        c["k1"], c["k2"], c["p1"], c["p2"], c["k3"] = dist
    return c


# gms_chess_candidate (include/gms.h): a chessboard corner candidate
CHESS_CANDIDATE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("response", "<u4")])
assert CHESS_CANDIDATE_DTYPE.itemsize == 12
