"""Hand-made inputs for the bundle adjustment tests, built on sfm_register_cases.assemble: a known scene seen by known
cameras, every pair's record written from the truth, the keypoints the scene's projections through a camera with a little
distortion plus Gaussian pixel noise (as float32, which a cv::KeyPoint is), and the registration the numpy statement
(sfm_register_ref.register) gives on them. case(name) -> dict(kp KEYPOINT records, frame_off, pairs, matches, mask, reg = the
registration's dict, camera = (fx, fy, cx, cy, k1, k2, p1, p2, k3), params = the bundle adjustment's keywords, scene)."""
import functools

import numpy as np

import sfm_register_cases as rc
import sfm_register_ref as R

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAMERA = (800.0, 790.0, 330.0, 250.0, -0.05, 0.01, 0.001, -0.0005, 0.0)


def distort(cam, x, y):
    """The forward model cv::undistortPoints inverts."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = cam
    r2 = x * x + y * y
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def keypoints(scene, cam, noise_px, seed):
    """Keypoint perm_f[s] of frame f is the projection of scene point s; the keypoints that show nothing lie anywhere."""
    rng = np.random.default_rng(seed)
    kp = np.zeros(int(scene.frame_off[-1]), KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.uniform(0, 660, len(kp)), rng.uniform(0, 500, len(kp))
    for f in range(scene.n_frames):
        Pc = scene.X @ scene.R[f].T + scene.t[f]
        u, v = distort(cam, Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2])
        at = scene.frame_off[f] + scene.perm[f]
        kp["x"][at] = u + noise_px * rng.standard_normal(len(u))
        kp["y"][at] = v + noise_px * rng.standard_normal(len(v))
    return kp


def build(scene, specs, noise_px=0.3, seed=1, cloud_cap=None, **params):
    c = rc.assemble(scene, specs)
    reg = R.register(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    if cloud_cap is not None:
        reg = dict(reg, cloud=reg["cloud"][:cloud_cap], cloud_id=reg["cloud_id"][:cloud_cap])
    kp = scene.keypoints(CAMERA, noise_px, seed) if hasattr(scene, "keypoints") else keypoints(scene, CAMERA, noise_px, seed)
    return dict(kp=kp, frame_off=c["frame_off"], pairs=c["pairs"], matches=c["matches"], mask=c["mask"],
                reg=reg, camera=CAMERA, params=params, scene=scene, points3d=c["points3d"], tv=c["tv"], root=c["root"], min_links=c["min_links"])


def _two_frames():
    """Two frames, one pair, 8 points: one free camera, and the gauge rescale is the whole story."""
    sc = rc.Scene(21, 2, 8)
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(8))])


def _three_chain():
    """Three chained frames: tracks of two keypoints (points 0..9 and 30..39) and of three (10..29); zero-mask matches in between."""
    sc = rc.Scene(22, 3, 40)
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30), junk=4), dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3)])


def _twelve_frames():
    """A chain of 12 frames: 11 free cameras, 66 unknowns -- past one wave of 64. Pair i shows points 4 i .. 4 i + 23."""
    sc = rc.Scene(23, 12, 70)
    return build(sc, [dict(a=i, b=i + 1, unit=1.0 + 0.25 * i, pts=np.arange(4 * i, 4 * i + 24)) for i in range(11)])


def _wide():
    """Three frames with 700 points each: a frame's observations take three passes of a 256-lane workgroup, and the 700 used tracks
    three workgroups of the per-track kernels."""
    sc = rc.Scene(24, 3, 700)
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 700), junk=9), dict(a=1, b=2, unit=0.5, pts=np.arange(0, 700), junk=7)])


def _multi():
    """three_chain with one wrong match more in pair (1, 2): point 12's keypoint of frame 1 to point 13's of frame 2, which chains
    the tracks of 12 and 13 into one with two keypoints in every frame."""
    sc = rc.Scene(22, 3, 40)

    def wrong(blk):
        blk["q"] = np.append(blk["q"], sc.perm[1][12])
        blk["t"] = np.append(blk["t"], sc.perm[2][13])
        blk["mask"] = np.append(blk["mask"], np.uint8(1))
        blk["P"] = np.concatenate([blk["P"], blk["P"][:1]])
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30), junk=4), dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3, edit=wrong)])


def _behind():
    """three_chain without re-triangulation, one three-keypoint track's cloud point put at z = 0.12: in front of cameras 0 and 1 (at
    z = 0 and 0.1), behind camera 2 (at 0.2): that observation is inactive."""
    c = _three_chain()
    reg = dict(c["reg"], cloud=c["reg"]["cloud"].copy())
    sc = c["scene"]
    g = int(sc.frame_off[0] + sc.perm[0][15])                   # point 15's keypoint of frame 0
    e = int(np.nonzero(reg["cloud_id"] == reg["track"][_slot_of(c, 0, g)])[0][0])
    reg["cloud"][e] = (0.01, 0.01, 0.12)
    return dict(c, reg=reg, params=dict(retriangulate=0), entry=e)


def _slot_of(c, pair, g):
    """The point slot of the match of `pair` whose query keypoint is global keypoint g."""
    p = c["pairs"][pair]
    off, m = int(p["match_off"]), int(p["m"])
    mk = c["mask"][off:off + m] != 0
    rank = np.cumsum(mk) - mk
    k = np.nonzero(mk & (c["matches"]["queryIdx"][off:off + m] + c["frame_off"][p["frame_a"]] == g))[0][0]
    return off + rank[k]


def _unregistered():
    """Four frames, pairs (0, 1) and (1, 2): frame 3 is in no pair, its zero view stays zero."""
    sc = rc.Scene(25, 4, 40)
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30)), dict(a=1, b=2, unit=3.0, pts=np.arange(10, 40))])


def _small_cap():
    """three_chain with the cloud cut to 20 entries: the tracks past them take no part."""
    sc = rc.Scene(22, 3, 40)
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30), junk=4), dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3)], cloud_cap=20)


def _outlier(huber_px):
    """three_chain with point 20's keypoint of frame 2 moved by 50 px."""
    c = _three_chain()
    kp = c["kp"].copy()
    sc = c["scene"]
    kp["x"][sc.frame_off[2] + sc.perm[2][20]] += 50.0
    return dict(c, kp=kp, params=dict(huber_px=huber_px))


class OwnScene:
    """What rc.Scene is to assemble() and build(), with a trajectory of its own: points X [n, 3], cameras R [F, 3, 3] and centres
    [F, 3] (t = -R centre), and per frame the scene points it shows (all of them when `seen` is None). A frame has a keypoint per point
    it shows and 3 + f % 4 that show nothing; perm[f][s] is -1 for a point the frame does not show."""

    def __init__(self, seed, X, R, centres, seen=None):
        rng = np.random.default_rng(seed)
        self.rng, self.n_frames, self.n_points = rng, len(R), len(X)
        self.X, self.R = np.asarray(X, dtype=np.float64), np.asarray(R, dtype=np.float64)
        self.t = np.stack([-(self.R[f] @ centres[f]) for f in range(self.n_frames)])
        self.seen = [np.arange(self.n_points) if seen is None else np.asarray(seen[f], dtype=np.int64) for f in range(self.n_frames)]
        self.counts = np.array([len(self.seen[f]) + 3 + f % 4 for f in range(self.n_frames)])
        self.perm = []
        for f in range(self.n_frames):
            pf = np.full(self.n_points, -1, np.int64)
            pf[self.seen[f]] = rng.permutation(self.counts[f])[:len(self.seen[f])]
            self.perm.append(pf)
        self.frame_off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)

    def cam(self, f, s):
        return self.X[s] @ self.R[f].T + self.t[f]

    def keypoints(self, cam, noise_px, seed):
        rng = np.random.default_rng(seed)
        kp = np.zeros(int(self.frame_off[-1]), KEYPOINT_DTYPE)
        kp["x"], kp["y"] = rng.uniform(0, 660, len(kp)), rng.uniform(0, 500, len(kp))
        for f in range(self.n_frames):
            Pc = self.cam(f, self.seen[f])
            assert (Pc[:, 2] > 0).all()                         # every point is in front of every camera that shows it
            u, v = distort(cam, Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2])
            at = self.frame_off[f] + self.perm[f][self.seen[f]]
            kp["x"][at] = u + noise_px * rng.standard_normal(len(u))
            kp["y"][at] = v + noise_px * rng.standard_normal(len(v))
        return kp


def _rot(ay, ax):
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    return Ry @ Rx


def _two_tiles():
    """Three frames with 4300 points each, all of them tracks of two or three keypoints: the cloud's 4300 entries span two tiles of
    the prefix sum (4096 entries each), with used tracks on both sides of entry 4096; junk in both pairs, so rank != k."""
    sc = rc.Scene(26, 3, 4300)
    return build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 4250), junk=11), dict(a=1, b=2, unit=1.5, pts=np.arange(50, 4300), junk=13)])


MANY_FRAMES, MANY_STEP, MANY_WINDOW = 262, 2, 12


def _many_frames(cloud_cap=None):
    """A chain of 262 frames, 261 free cameras: every lane-strided loop over the frames takes a second pass. The cameras stand 0.25
    apart along x with rotations of up to 0.02 rad; pair i shows the 12 points 2 i .. 2 i + 11, which lie around x = 0.25 i at depth
    5 to 9, so a track spans up to 7 frames and a frame has at most 14 observations. n_iters = 3 and n_cg = 10 keep the statement's
    per-frame Python solves (261 Cholesky solves per conjugate-gradient iteration) to a second or so."""
    F = MANY_FRAMES
    rng = np.random.default_rng(27)
    n_points = MANY_STEP * (F - 2) + MANY_WINDOW
    s = np.arange(n_points)
    X = np.stack([0.25 * s / MANY_STEP + rng.uniform(-1, 1, n_points), rng.uniform(-1, 1, n_points), rng.uniform(5, 9, n_points)], 1)
    f = np.arange(F)
    R = np.stack([_rot(0.02 * np.sin(0.3 * k), 0.015 * np.cos(0.5 * k)) for k in f])
    centres = np.stack([0.25 * f, 0.02 * np.sin(0.7 * f), 0.03 * np.cos(0.4 * f) - 0.03], 1)
    shows = [np.arange(MANY_STEP * i, MANY_STEP * i + MANY_WINDOW) for i in range(F - 1)]
    seen = [np.unique(np.concatenate(([shows[k - 1]] if k else []) + ([shows[k]] if k < F - 1 else []))) for k in f]
    sc = OwnScene(28, X, R, centres, seen)
    return build(sc, [dict(a=i, b=i + 1, unit=1.0 + 0.05 * (i % 7), pts=shows[i], junk=5) for i in range(F - 1)], cloud_cap=cloud_cap,
                 n_iters=3, n_cg=10)


FRAMES_PAST_CAP = 200


def _frames_past_cap():
    """many_frames with the cloud cut to its first 200 entries -- fewer than the 262 frames, so the frames size the grid of the kernel
    that takes the step -- which the first hundred or so frames observe: every free frame behind them has a zero block, no Cholesky
    factor, and z = 0 in the preconditioner."""
    return _many_frames(cloud_cap=FRAMES_PAST_CAP)


CAP_FILL = 555.0


def _cap_past_tracks():
    """three_chain with cloud and cloud_id 50 entries longer than the registration's n_tracks = 40, as a cloud_cap past the track count
    leaves them: the rows behind n_tracks hold CAP_FILL and ids that repeat the 12 lowest real ones in no order -- more of them than
    real entries, so a binary search over all 90 looks at the padding first and is sent the wrong way. They must neither be searched
    nor visited: status FEW, their bytes kept, every real entry as in three_chain."""
    c = _three_chain()
    reg, ids = c["reg"], c["reg"]["cloud_id"]
    pad = ids[(7 * np.arange(50) + 3) % 12]
    reg = dict(reg, cloud=np.concatenate([reg["cloud"], np.full((len(pad), 3), CAP_FILL)]), cloud_id=np.concatenate([ids, pad]).astype(ids.dtype))
    return dict(c, reg=reg, n_real=len(ids))


def _multi_sorted():
    """Four frames, three chained pairs. Points 10..29 are in every pair: tracks with one keypoint in each of the 4 frames (n =
    n_frames, the longest list that is still sorted). Points 30..39 are in pair (1, 2) alone; one wrong match more in that pair, from
    the frame-1 keypoint of point 42 (which no other match names) to point 35's of frame 2, gives 35's track three keypoints, two of
    them in frame 1: n = 3 <= n_frames, so only the comparison of sorted neighbours can find it."""
    sc = rc.Scene(29, 4, 45)

    def wrong(blk):
        blk["q"] = np.append(blk["q"], sc.perm[1][42])
        blk["t"] = np.append(blk["t"], sc.perm[2][35])
        blk["mask"] = np.append(blk["mask"], np.uint8(1))
        blk["P"] = np.concatenate([blk["P"], blk["P"][:1]])
    c = build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30), junk=4), dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3, edit=wrong),
                   dict(a=2, b=3, unit=0.5, pts=np.arange(10, 30), junk=5)])
    return dict(c, entry=_entry_of(c, 1, 35), whole=[_entry_of(c, 1, s) for s in (10, 29)])


def _entry_of(c, f, s):
    """The cloud entry of the track that frame f's keypoint of scene point s belongs to."""
    sc = c["scene"]
    g = int(sc.frame_off[f] + sc.perm[f][s])
    root = min(int(x) for x in _component(c, g))
    return int(np.nonzero(c["reg"]["cloud_id"] == root)[0][0])


def _component(c, g):
    """The global keypoints that the inlier matches of the case's registered pairs chain to keypoint g."""
    comp, grew = {g}, True
    edges = []
    for i, p in enumerate(c["pairs"]):
        if c["reg"]["registration"][i]["status"] != 0:
            continue
        off, n = int(p["match_off"]), int(c["tv"][i]["n_points"])
        mk = c["mask"][off:off + n] != 0
        edges += list(zip((c["frame_off"][p["frame_a"]] + c["matches"]["queryIdx"][off:off + n][mk]).tolist(),
                          (c["frame_off"][p["frame_b"]] + c["matches"]["trainIdx"][off:off + n][mk]).tolist()))
    while grew:
        grew = False
        for x, y in edges:
            if (x in comp) != (y in comp):
                comp |= {x, y}
                grew = True
    return comp


def _kept():
    """Re-triangulation refused for two reasons, with retriangulate = 1. Cameras 0 and 1 look along z without rotation, camera 1
    0.5 further along it, camera 2 to the side. (a) `behind`: point 5's keypoint of frame 1 is put half as far from the principal
    point as its keypoint of frame 0, where a camera that has moved forward sees it further out -- a wrong match whose rays meet
    about 0.5 behind camera 0. (b) `singular`: point 40 is on the optical axis
    and in pair (0, 1) alone, and both its keypoints are the principal point to the bit: both rays are (0, 0, 1) exactly, the normal
    matrix is diag(2, 2, 0), its determinant is 0 in any arithmetic and the closed-form inverse gives zeros. (A float32 keypoint holds
    (cx, cy) = (330, 250) exactly, and the undistortion's fixed point at the centre is exact.) Both stay in the problem at the
    registration's point. n_iters = 2: the rays of (a) diverge, so its point runs away along them, about three times as far with
    every step taken, and what the order of a sum is worth grows with it (4e-15 after one iteration, 2e-8 after six)."""
    rng = np.random.default_rng(30)
    n = 41
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(5, 9, n)], 1)
    X[5], X[40] = (2.0, 1.0, 6.0), (0.0, 0.0, 7.0)
    R = np.stack([np.eye(3), np.eye(3), _rot(0.05, -0.03)])
    centres = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.5], [0.7, 0.1, 0.2]])
    sc = OwnScene(31, X, R, centres)
    c = build(sc, [dict(a=0, b=1, unit=1.0, pts=np.concatenate([np.arange(0, 30), [40]]), junk=4),
                   dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3)], n_iters=2)
    kp = c["kp"].copy()
    g0, g1 = sc.frame_off[0] + sc.perm[0][5], sc.frame_off[1] + sc.perm[1][5]
    kp["x"][g1], kp["y"][g1] = CAMERA[2] + 0.5 * (kp["x"][g0] - CAMERA[2]), CAMERA[3] + 0.5 * (kp["y"][g0] - CAMERA[3])
    for f in (0, 1):
        g = sc.frame_off[f] + sc.perm[f][40]
        kp["x"][g], kp["y"][g] = CAMERA[2], CAMERA[3]
    return dict(c, kp=kp, behind=_entry_of(c, 0, 5), singular=_entry_of(c, 0, 40))


def _misfit_records():
    """three_chain plus records that do not fit the arrays and must contribute nothing. Pairs, every one with an ok registration
    record: frame_a = n_frames; frame_b = -1; a match range that ends 5 slots past the arrays (its first 5 slots, the arrays' last,
    hold inlier matches between spare keypoints of frames 1 and 2 whose track slots name real tracks); m < 0; a match_off so large
    that match_off + m does not fit 64 bits. Matches, in pair 0's spare capacity, all inliers: queryIdx = -1, queryIdx = count_a and
    trainIdx = count_b with a real track's id in their slot of `track`, and one between two keypoints of no track whose slot holds
    -1. total_m is the arrays' length."""
    sc = rc.Scene(22, 3, 40)
    c = build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30), junk=4, pad=4), dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3)])
    reg = c["reg"]
    matches, mask, track, ids = c["matches"].copy(), c["mask"].copy(), reg["track"].copy(), reg["cloud_id"]
    total_m, cnt = len(mask), sc.counts
    spare = [np.setdiff1d(np.arange(cnt[f]), sc.perm[f]) for f in range(3)]          # keypoints that show nothing (frame 0 has none)
    free0 = sc.perm[0][30:40]                                                        # frame 0's keypoints of points no pair of it shows
    p0 = c["pairs"][0]
    off, n = int(p0["match_off"]), int(c["tv"][0]["n_points"])
    rank_n = int((mask[off:off + n] != 0).sum())
    for j, (q, t, T) in enumerate([(-1, spare[1][0], ids[1]), (cnt[0], spare[1][1], ids[2]), (free0[0], cnt[1], ids[3]), (free0[1], spare[1][2], -1)]):
        matches["queryIdx"][off + n + j], matches["trainIdx"][off + n + j], mask[off + n + j] = q, t, 1
        track[off + rank_n + j] = T
    for j in range(5):                                                               # the arrays' last 5 slots
        matches["queryIdx"][total_m - 5 + j], matches["trainIdx"][total_m - 5 + j], mask[total_m - 5 + j] = spare[1][j % 3], spare[2][j], 1
        track[total_m - 5 + j] = ids[4 + j]
    more = np.zeros(5, c["pairs"].dtype)
    more[0] = (3, 1, 10, 0, off)
    more[1] = (0, -1, 10, 0, off)
    more[2] = (1, 2, 10, 0, total_m - 5)
    more[3] = (1, 2, -4, 0, off)
    more[4] = (0, 1, 10, 0, np.iinfo(np.int64).max - 4)
    rec = np.zeros(5, reg["registration"].dtype)
    rec["S"], rec["link"], rec["role"], rec["status"] = 1.0, 0, 1, 0
    reg = dict(reg, track=track, registration=np.concatenate([reg["registration"], rec]))
    return dict(c, pairs=np.concatenate([c["pairs"], more]), matches=matches, mask=mask, reg=reg, total_m=total_m, n_real_pairs=2)


def _rejected_step():
    """Steps that are dropped, then steps that are taken: three_chain's layout on a scene of its own (seed 40, found by a search over
    seeds 40..51) with six keypoints of frame 2 moved 60 px left or right, no Huber weights, no re-triangulation and lambda0 = 1e-9,
    so that the first steps are all but Gauss-Newton's and overshoot. The statement drops the first 7 -- each at 1.6 to 59 times the
    cost it started from, and with every observation still active, so the order of a sum cannot turn the decision -- and takes the
    last 3, lambda having grown to 1e-2."""
    sc = rc.Scene(40, 3, 40)
    c = build(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30), junk=4), dict(a=1, b=2, unit=2.0, pts=np.arange(10, 40), junk=3)])
    kp = c["kp"].copy()
    for j in range(6):
        kp["x"][sc.frame_off[2] + sc.perm[2][20 + j]] += 60.0 * (-1) ** j
    return dict(c, kp=kp, params=dict(huber_px=0.0, lambda0=1e-9, retriangulate=0))


def _twelve_with(**params):
    return dict(_twelve_frames(), params=params)


def _as_is():
    """n_iters = 0 and retriangulate = 0: the inputs' bytes come back."""
    return dict(_three_chain(), params=dict(n_iters=0, retriangulate=0))


def _retriangulate_only():
    return dict(_three_chain(), params=dict(n_iters=0))


CASES = {"two_frames": _two_frames, "three_chain": _three_chain, "twelve_frames": _twelve_frames, "wide": _wide, "multi": _multi, "behind": _behind,
         "unregistered": _unregistered, "small_cap": _small_cap, "outlier_huber": lambda: _outlier(2.0), "outlier_plain": lambda: _outlier(0.0),
         "as_is": _as_is, "retriangulate_only": _retriangulate_only,
         "two_tiles": _two_tiles, "many_frames": _many_frames, "frames_past_cap": _frames_past_cap, "cap_past_tracks": _cap_past_tracks,
         "multi_sorted": _multi_sorted, "kept": _kept, "misfit_records": _misfit_records, "rejected_step": _rejected_step,
         "cg_short": lambda: _twelve_with(n_cg=2), "cg_converges": lambda: _twelve_with(cg_tol=1e-2),
         "ftol_stops": lambda: _twelve_with(ftol=1e-3), "iters_run_out": lambda: _twelve_with(n_iters=3, ftol=0.0)}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def xy_of(kp):
    return np.stack([kp["x"], kp["y"]], 1)
