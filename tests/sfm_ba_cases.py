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
    return dict(kp=keypoints(scene, CAMERA, noise_px, seed), frame_off=c["frame_off"], pairs=c["pairs"], matches=c["matches"], mask=c["mask"],
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


def _as_is():
    """n_iters = 0 and retriangulate = 0: the inputs' bytes come back."""
    return dict(_three_chain(), params=dict(n_iters=0, retriangulate=0))


def _retriangulate_only():
    return dict(_three_chain(), params=dict(n_iters=0))


CASES = {"two_frames": _two_frames, "three_chain": _three_chain, "twelve_frames": _twelve_frames, "wide": _wide, "multi": _multi, "behind": _behind,
         "unregistered": _unregistered, "small_cap": _small_cap, "outlier_huber": lambda: _outlier(2.0), "outlier_plain": lambda: _outlier(0.0),
         "as_is": _as_is, "retriangulate_only": _retriangulate_only}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def xy_of(kp):
    return np.stack([kp["x"], kp["y"]], 1)
