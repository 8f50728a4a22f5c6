"""Two-view and registration records of frame pairs from a view array, stated in numpy: the library's own definition,
which sfm_pair_pose_core.h / sfm_pair_pose_kernels.hip compute on the device and tests/cpp/sfm_pair_pose_host.cpp on the host.

A view is x_cam = R x_world + t (sfm_register_ref.py). For the pair (a, b): R_ab[r][c] = sum_k R_b[r][k] R_a[c][k], T = t_b - R_ab t_a,
S = sqrt(T0^2 + T1^2 + T2^2), t = T / S. fp64, only + - * / sqrt, every sum in index order 0, 1, 2: the bytes of the C code.

The registration builds a view as G_b = [R_i G_a.R | R_i G_a.t + S_i t_i] from pair i's two-view R_i, unit t_i and scale S_i, so that
in exact arithmetic R_ab = R_i, T = S_i t_i and S = S_i: fed the registration's own `views`, pair_poses reproduces each ok pair's
two-view R, unit t and the registration's S up to rounding (measured by tests/test_sfm_pair_pose_ref.py; the figures are in DESIGN.md
§4.10d). `reverse=True` takes every sum in the opposite order; the tests size their tolerance by the change that makes."""
import numpy as np

GMS_OK, GMS_ERR_NO_MODEL = 0, -8

PAIR_DTYPE = np.dtype([("frame_a", "<i4"), ("frame_b", "<i4"), ("m", "<i4"), ("reserved", "<i4"), ("match_off", "<i8")])
VIEW_DTYPE = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("registered", "<i4"), ("pair", "<i4")])
TWO_VIEW_DTYPE = np.dtype([("E", "<f8", (3, 3)), ("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("sum_sq_err1", "<f8"), ("sum_sq_err2", "<f8"),
                           ("n_finite", "<i8"), ("n_behind", "<i8"), ("n_points", "<i4"), ("n_ransac", "<i4"), ("ransac_iters", "<i4"),
                           ("n_pose", "<i4"), ("pose_which", "<i4"), ("n_triangulated", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
PAIR_REG_DTYPE = np.dtype([("r", "<f8"), ("S", "<f8"), ("n_links", "<i4"), ("depth", "<i4"), ("link", "<i4"), ("role", "<i4"),
                           ("status", "<i4"), ("reserved", "<i4")])
assert TWO_VIEW_DTYPE.itemsize == 232 and PAIR_REG_DTYPE.itemsize == 40 and VIEW_DTYPE.itemsize == 104 and PAIR_DTYPE.itemsize == 24


def _sum3(x0, x1, x2, reverse):
    return (x2 + x1) + x0 if reverse else (x0 + x1) + x2


def relative_pose(Ra, ta, Rb, tb, reverse=False):
    """(ok, R_ab [3, 3], t [3], S) of two views; ok False: something is not finite, or the centres coincide."""
    Ra, Rb = np.asarray(Ra, np.float64).reshape(3, 3), np.asarray(Rb, np.float64).reshape(3, 3)
    ta, tb = np.asarray(ta, np.float64).reshape(3), np.asarray(tb, np.float64).reshape(3)
    Rab, T = np.zeros((3, 3)), np.zeros(3)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                Rab[r, c] = _sum3(Rb[r, 0] * Ra[c, 0], Rb[r, 1] * Ra[c, 1], Rb[r, 2] * Ra[c, 2], reverse)
        for r in range(3):
            T[r] = tb[r] - _sum3(Rab[r, 0] * ta[0], Rab[r, 1] * ta[1], Rab[r, 2] * ta[2], reverse)
        S = np.sqrt(_sum3(T[0] * T[0], T[1] * T[1], T[2] * T[2], reverse))
        ok = bool(np.isfinite(Rab).all() and np.isfinite(T).all() and np.isfinite(S) and S > 0.0)
        t = T / S if ok else np.zeros(3)
    return ok, Rab, t, float(S)


def pair_poses(views, frame_pairs, reverse=False):
    """views: VIEW_DTYPE [n_frames]; frame_pairs [n, 2] (any integers) -> (TWO_VIEW_DTYPE [n], PAIR_REG_DTYPE [n])."""
    views = np.asarray(views)
    fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
    tv, reg = np.zeros(len(fp), TWO_VIEW_DTYPE), np.zeros(len(fp), PAIR_REG_DTYPE)
    tv["status"] = reg["status"] = GMS_ERR_NO_MODEL
    reg["link"] = -1
    n = len(views)
    for i, (a, b) in enumerate(fp):
        if not (0 <= a < n and 0 <= b < n) or a == b:
            continue
        A, B = views[a], views[b]
        if A["registered"] == 0 or B["registered"] == 0:
            continue
        ok, Rab, t, S = relative_pose(A["R"], A["t"], B["R"], B["t"], reverse)
        if not ok:
            continue
        tv[i]["R"], tv[i]["t"], tv[i]["status"] = Rab, t, GMS_OK
        reg[i]["S"], reg[i]["status"] = S, GMS_OK
    return tv, reg


def pair_table(frame_pairs):
    """PAIR_DTYPE records of frame pairs (m and match_off 0: the stage reads neither)."""
    fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(len(fp), PAIR_DTYPE)
    out["frame_a"], out["frame_b"] = fp[:, 0].astype(np.int32), fp[:, 1].astype(np.int32)
    return out


def views_of(poses, registered=None):
    """VIEW_DTYPE records of (R, t) poses; registered: flags per view (default all 1)."""
    out = np.zeros(len(poses), VIEW_DTYPE)
    for i, (R, t) in enumerate(poses):
        out[i]["R"], out[i]["t"] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    out["registered"] = 1 if registered is None else np.asarray(registered)
    out["pair"] = -1
    return out


def case_bytes(views, pairs):
    """A case as tests/cpp/sfm_pair_pose_host.cpp reads it: n_frames, n_pairs, the views, the pair table."""
    return np.array([len(views), len(pairs)], np.int32).tobytes() + np.ascontiguousarray(views).tobytes() + np.ascontiguousarray(pairs).tobytes()


def result_bytes(tv, reg):
    return np.ascontiguousarray(tv).tobytes() + np.ascontiguousarray(reg).tobytes()
