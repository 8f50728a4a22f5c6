"""Cases for the pair records from views (tests/sfm_pair_pose_ref.py), shared by the CPU test (the host build of
sfm_pair_pose_core.h) and the GPU test (the kernel): the five-view scene's registration views, and hand-made view arrays and pair
tables for every way a pair fails. A case is (name, views VIEW_DTYPE [n_frames], frame_pairs int [n, 2])."""
import numpy as np

import sfm_pair_pose_ref as pp
from sfm_ba_cases import KEYPOINT_DTYPE
from sfm_register_cases import DMATCH_DTYPE, PAIR_DTYPE, TWO_VIEW_DTYPE

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FIVE_VIEW_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 4)]


def five_view_inputs(synth, noise_px=0.0):
    """synth.make_multi_view_scene(7, 5, n_kp=400, noise_px), the pairs (0, 1), (1, 2), (2, 3), (0, 4) with 20 % of each pair's train
    indices replaced by default_rng(1) draws (the scene and the matches of the registration's five-view test), through the CPU two-view
    chain -> dict(camera, kp, frame_off, pairs, matches, mask, points3d, tv, frame_pairs): what SfmRegister and SfmBundle load."""
    import sfm_ref
    sc = synth.make_multi_view_scene(7, 5, n_kp=400, noise_px=noise_px)
    frame_pairs, n = FIVE_VIEW_PAIRS, 400
    rng = np.random.default_rng(1)
    pairs, tv = np.zeros(4, PAIR_DTYPE), np.zeros(4, TWO_VIEW_DTYPE)
    matches, mask, points = np.zeros(4 * n, DMATCH_DTYPE), np.zeros(4 * n, np.uint8), np.zeros((4 * n, 3))
    for i, (a, b) in enumerate(frame_pairs):
        t = np.arange(n)
        bad = rng.choice(n, n // 5, replace=False)
        t[bad] = rng.integers(0, n, n // 5)
        pairs[i] = (a, b, n, 0, i * n)
        matches["queryIdx"][i * n:(i + 1) * n], matches["trainIdx"][i * n:(i + 1) * n] = np.arange(n), t
    for i, (a, b) in enumerate(frame_pairs):
        q, t = matches["queryIdx"][i * 400:(i + 1) * 400], matches["trainIdx"][i * 400:(i + 1) * 400]
        uv1 = np.stack([sc["frames"][a]["x"][q], sc["frames"][a]["y"][q]], 1)
        uv2 = np.stack([sc["frames"][b]["x"][t], sc["frames"][b]["y"][t]], 1)
        r = sfm_ref.two_view(uv1, uv2, sc["camera"], None, 0.7, 1.0, 1000)
        assert r["E"] is not None
        k = int((r["mask"] != 0).sum())
        tv[i]["R"], tv[i]["t"], tv[i]["n_points"], tv[i]["n_triangulated"] = r["R"], np.asarray(r["t"]).reshape(3), 400, k
        mask[i * 400:(i + 1) * 400] = r["mask"]
        points[i * 400:i * 400 + k] = r["points"]
    kp = np.zeros(5 * 400, KEYPOINT_DTYPE)
    kp["x"] = np.concatenate([fr["x"] for fr in sc["frames"]])
    kp["y"] = np.concatenate([fr["y"] for fr in sc["frames"]])
    return dict(camera=tuple(sc["camera"]), kp=kp, frame_off=np.arange(6, dtype=np.int64) * 400, pairs=pairs, matches=matches, mask=mask,
                points3d=points, tv=tv, frame_pairs=frame_pairs)


def five_view_registration(synth):
    """The registration statement on five_view_inputs -> (two-view records, the registration's result, its frame pairs)."""
    import sfm_register_ref as R
    c = five_view_inputs(synth)
    reg = R.register(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"])
    return c["tv"], reg, c["frame_pairs"]


def as_views(views):
    """Any view records with the fields of VIEW_DTYPE -> VIEW_DTYPE (the registration statement's dtype has the same layout)."""
    out = np.zeros(len(views), pp.VIEW_DTYPE)
    for k in ("R", "t", "registered", "pair"):
        out[k] = np.asarray(views[k]).reshape(out[k].shape)
    return out


def random_views(seed, n_frames):
    """Seeded registered views: rotations from the QR of normal draws (det +1), centres a few units apart."""
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(n_frames):
        Q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        poses.append((Q, rng.uniform(-4, 4, 3)))
    return pp.views_of(poses)


def random_case(seed, n_frames, n_pairs, bad_last=False):
    """n_pairs pairs of distinct frames of random_views; bad_last: the last pair names frame n_frames (a bad pair in the last lane of a
    partial wave, when n_pairs is no multiple of 64)."""
    rng = np.random.default_rng(seed + 1000)
    a = rng.integers(0, n_frames, n_pairs)
    b = (a + rng.integers(1, n_frames, n_pairs)) % n_frames
    fp = np.stack([a, b], 1)
    if bad_last:
        fp[-1] = (0, n_frames)
    return (f"random_{n_pairs}{'_bad_last' if bad_last else ''}", random_views(seed, n_frames), fp)


def hand_cases(views5, frame_pairs5):
    """views5: the five-view scene's registration views. One case per way a pair goes: those views (the registration's own pairs,
    their reverses and pairs the sparse stage never had), a == b, an unregistered frame (zeroed, and flagged only), frame indices -1,
    n_frames and the ends of int32, coincident centres, NaN and infinite entries and sums that overflow or underflow, no pair at all."""
    v5 = as_views(views5)
    fp5 = list(frame_pairs5)
    out = [("five_views", v5, fp5 + [(b, a) for a, b in fp5] + [(0, 2), (1, 3), (4, 2), (3, 4)])]
    out.append(("same_frame", v5, [(0, 0), (3, 3), (0, 1), (4, 4)]))
    unreg = v5.copy()
    unreg[2] = np.zeros(1, pp.VIEW_DTYPE)[0]   # zeros, as the registration leaves a frame it did not reach
    unreg["pair"][2] = -1
    flagged = v5.copy()
    flagged["registered"][3] = 0              # a pose is there, the flag says no
    out.append(("unregistered", unreg, [(0, 1), (1, 2), (2, 3), (2, 0), (3, 4)]))
    out.append(("unregistered_flag", flagged, [(2, 3), (3, 4), (0, 4), (3, 0)]))
    out.append(("bad_index", v5, [(-1, 0), (0, -1), (5, 0), (0, 5), (I32_MIN, 1), (1, I32_MAX), (I32_MAX, I32_MIN), (-1, -1), (5, 5), (0, 1),
                                  (4, 3)]))
    eye = np.eye(3)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    co = pp.views_of([(eye, (1.0, 2.0, 3.0)), (eye, (1.0, 2.0, 3.0)), (Rz, (0.0, 0.0, 0.0)), (eye, (0.0, 0.0, 0.0)), (eye, (1.0, 2.0, 3.5))])
    out.append(("coincident", co, [(0, 1), (1, 0), (2, 3), (3, 2), (0, 4), (4, 1)]))
    bad = []
    for where, k, val in (("R", 0, np.nan), ("R", 4, np.inf), ("R", 8, -np.inf), ("t", 0, np.nan), ("t", 1, np.inf), ("t", 2, -np.inf)):
        R, t = v5["R"][1].copy().reshape(9), v5["t"][1].copy()
        (R if where == "R" else t)[k] = val
        bad.append((R, t))
    nf = pp.views_of([(v5["R"][0], v5["t"][0])] + bad + [(eye, (np.inf, 0.0, 0.0)), (eye, (np.inf, 0.0, 0.0)),   # 7, 8: inf - inf
                                                         (eye, (1e300, 1e300, 0.0)),                             # 9: T0^2 overflows
                                                         (eye, (1e-200, 0.0, 0.0)),                              # 10: T0^2 underflows to 0
                                                         (eye * 1e200, (0.0, 0.0, 0.0))])                        # 11: R_ab overflows with itself
    out.append(("non_finite", nf, [(0, i) for i in range(1, 12)] + [(i, 0) for i in range(1, 12)] + [(7, 8), (3, 10), (11, 11), (11, 3)]))
    out.append(("empty", v5, []))
    return out


def statement(case):
    return pp.pair_poses(case[1], case[2])


# ---- the rendered plane of dense_fuse_cases.scene3() on records derived from views ---------------------------------------------------------
def scene_views(f=1.0):
    """The three true views of dense_fuse_cases.scene3() (camera 1 is the world); f != 1: camera 2's centre moved along the baseline of
    the pair (1, 2) to c1 + f (c2 - c1) -- what a wrong scale of that pair does to the registration's view."""
    import rectify_cases as rc
    R1, t1 = np.asarray(rc.SCENE_R), np.asarray(rc.SCENE_T, dtype=np.float64)
    R2, t2 = R1 @ R1, R1 @ t1 + t1
    c1, c2 = -(R1.T @ t1), -(R2.T @ t2)
    return pp.views_of([(np.eye(3), np.zeros(3)), (R1, t1), (R2, -(R2 @ (c1 + f * (c2 - c1))))])


def scene_chain(views, frame_pairs, images=None):
    """The numpy chain on pose records derived from `views`: pair_poses -> rectify_ref.make_plan / rectify -> stereo_sgm_ref ->
    rectify_ref.cloud in the world frame -> dense_fuse_ref.fuse. Returns dict(tv, reg, pairs = per pair dict(plan, rect1, rect2, valid,
    disp16, xyz, color, pixel), sources, fused). images: three uint8 [72, 96] (default scene3())."""
    import dense_fuse_cases as fc
    import dense_fuse_ref as fr
    import rectify_cases as rc
    import rectify_ref as rr
    import stereo_sgm_ref
    imgs = fc.scene3() if images is None else images
    tv, reg = pp.pair_poses(views, frame_pairs)
    f16 = (rc.SCENE_SGM["min_disparity"] - 1) * 16
    per_pair, sources = [], []
    for i, (a, b) in enumerate(frame_pairs):
        if tv[i]["status"] == pp.GMS_OK:
            P = rr.make_plan(rc.SCENE_CAMERA, None, tv[i]["R"], tv[i]["t"], rc.SCENE_SIZE, rc.SCENE_SIZE)
        else:
            P = rr.zero_plan()
        r1, v1 = rr.rectify(imgs[a], rc.SCENE_CAMERA, None, P, 1, rc.SCENE_SIZE)
        r2, _ = rr.rectify(imgs[b], rc.SCENE_CAMERA, None, P, 2, rc.SCENE_SIZE)
        disp, _ = stereo_sgm_ref.stereo_sgm(r1, r2, **rc.SCENE_SGM)
        G = (views[a]["R"].reshape(9), views[a]["t"], int(views[a]["registered"]))
        xyz, col, pix = rr.cloud(disp, v1, r1, P, f16, 16, float(reg[i]["S"]), (G[0], G[1]))
        if reg[i]["status"] != pp.GMS_OK:
            xyz, col, pix = xyz[:0], col[:0], pix[:0]
        per_pair.append(dict(plan=P, rect1=r1, rect2=r2, valid=v1, disp16=disp, xyz=xyz, color=col, pixel=pix))
        sources.append(fr.source(disp, v1, P, xyz, color=col.reshape(-1, 1), filtered16=f16, min_disp16=16, view=G,
                                 reg=(float(reg[i]["S"]), int(reg[i]["status"]))))
    return dict(tv=tv, reg=reg, pairs=per_pair, sources=sources, fused=fr.fuse(sources))


def agreement(chain):
    """(agreeing, overlapping, fused total) of a two-source chain: source 1's points that source 0 sees, and of those the CONSISTENT."""
    import dense_fuse_ref as fr
    s0, s1 = chain["sources"]
    l = fr.look(s0, s1["xyz"][:fr.n_points(s1)], 16)
    return int((l == fr.CONSISTENT).sum()), int((l != fr.UNSEEN).sum()), int(chain["fused"]["counts"][-1])
