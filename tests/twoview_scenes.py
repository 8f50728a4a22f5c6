"""Scenes, minimal samples and checks shared by the two-view tests (test_twoview_core.py on the host build, test_gpu_twoview_geometry.py
on the GPU): other motions than the one scene of test_gpu_twoview.py, degenerate configurations, and what makes a 3 x 3 matrix an
essential matrix. The numpy restatement is the slow part: what it returns is computed once per configuration and shared, and is also
RECORDED in tests/golden/twoview/restatement.npz (tests/golden/make_twoview_restatement.py), which the GPU tests compare with; the
host tests compute it afresh and hold the record to it."""
import functools
import os

import numpy as np

import sfm_ref

BASE_CAMERA = (1400.0, 1380.0, 960.0, 540.0)
CAMERAS = [(500.0, 520.0, 300.0, 260.0), (3000.0, 2990.0, 2016.0, 1512.0), (1400.0, 700.0, 100.0, 900.0)]
THRESHOLDS = [0.25, 0.5, 3.0, 10.0]
N_LIST = [6, 7, 11, 12, 13, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1025]
MAX_ITERS_LIST = [0, 1, 2, 11, 12, 13, 15, 16, 17, 23, 24, 25]

# The solver's validity gate (sfm_ref.VALIDITY_GATE = tv::kValidityGate) bounds the largest constraint value r of a
# unit-norm E. With singular values s1 >= s2 >= s3 (their squares sum to 1), M = 2 E E^T E - tr(E E^T) E is diag(s_i (2 s_i^2 - 1))
# in E's singular bases, and its largest entry is at least |M|_F / 3, so r >= |s_i (2 s_i^2 - 1)| / 3 for each i. For s3 <= 1/2 that is
# r >= s3 / 6; around s1 = s2 = 1 / sqrt 2 the function s (2 s^2 - 1) has slope 2, so to first order r >= 2 sqrt 2 (s1 - s2) / 2 / 3.
# Relative to s1 ~ 0.7 a model within the gate therefore has s3 / s1 <= 8.5 r and (s1 - s2) / s1 <= 3 r; the bound leaves ten times
# that (measured on the 2 x 2700 samples of the families below: at most 2e-15 for every model that passes).
SPREAD_BOUND = 100.0 * sfm_ref.VALIDITY_GATE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twoview", "restatement.npz")


def rot(a):
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


BASE_R, BASE_T = rot([0.03, np.deg2rad(6.0), -0.01]), np.array([-0.6, 0.02, 0.05])


# ---- what defines an essential matrix ------------------------------------------------------------------------------------------------------
def constraint_residual(E):
    """largest absolute value among det E and the entries of 2 E E^T E - tr(E E^T) E, of E scaled to unit Frobenius norm"""
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    G = E @ E.T
    return float(max(abs(np.linalg.det(E)), np.abs(2.0 * G @ E - np.trace(G) * E).max()))


def singular_spread(E):
    """(|s1 - s2| / s1, s3 / s1) of the singular values"""
    s = np.linalg.svd(np.asarray(E, dtype=np.float64).reshape(3, 3), compute_uv=False)
    return float((s[0] - s[1]) / s[0]), float(s[2] / s[0])


def assert_valid_model(E, where=""):
    r, (d12, d3) = constraint_residual(E), singular_spread(E)
    assert r <= sfm_ref.VALIDITY_GATE and d12 < SPREAD_BOUND and d3 < SPREAD_BOUND, (where, r, d12, d3)


# ---- minimal samples: [count, 5, 2] normalised points of both images ---------------------------------------------------------------------
GENERIC_FAMILIES = ["generic", "noisy", "unrelated", "integer_pixel"]
DEGENERATE_FAMILIES = ["collinear_1", "collinear_both", "pure_rotation", "planar", "repeated_point"]
FAMILIES = GENERIC_FAMILIES + DEGENERATE_FAMILIES


@functools.lru_cache(maxsize=None)
def minimal_samples(family, count=300, seed=11):
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    fx, fy, cx, cy = BASE_CAMERA
    x1s, x2s = np.zeros((count, 5, 2)), np.zeros((count, 5, 2))
    for s in range(count):
        R, t = rot(rng.uniform(-0.3, 0.3, 3)), rng.uniform(-1, 1, 3)
        X = np.stack([rng.uniform(-2, 2, 5), rng.uniform(-1.5, 1.5, 5), rng.uniform(3, 9, 5)], axis=1)
        if family == "planar":
            X[:, 2] = 6.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1]
        if family == "pure_rotation":
            t = np.zeros(3)
        if family == "repeated_point":
            X[4] = X[0]
        Xc = X @ R.T + t
        x1, x2 = X[:, :2] / X[:, 2:3], Xc[:, :2] / Xc[:, 2:3]
        if family == "noisy":
            x2 = x2 + rng.normal(0, 0.01, (5, 2))
        if family == "unrelated":
            x2 = rng.uniform(-0.5, 0.5, (5, 2))
        if family == "integer_pixel":
            x1 = (np.rint(x1 * [fx, fy] + [cx, cy]) - [cx, cy]) / [fx, fy]
            x2 = (np.rint(x2 * [fx, fy] + [cx, cy]) - [cx, cy]) / [fx, fy]
        if family in ("collinear_1", "collinear_both"):
            x1[:, 1] = 0.1 * x1[:, 0] + rng.uniform(-0.2, 0.2)
        if family == "collinear_both":
            x2[:, 1] = -0.3 * x2[:, 0] + rng.uniform(-0.2, 0.2)
        x1s[s], x2s[s] = x1, x2
    x1s.setflags(write=False)
    x2s.setflags(write=False)
    return x1s, x2s


@functools.lru_cache(maxsize=None)
def restatement_models(family):
    x1, x2 = minimal_samples(family)
    return [sfm_ref.five_point(a, b) for a, b in zip(x1, x2)]


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def recorded_models(family):
    """restatement_models(family) as recorded (the four well-posed families)"""
    z = _golden()
    counts, flat = z[f"models_count_{family}"], z[f"models_{family}"].reshape(-1, 3, 3)
    ends = np.cumsum(counts)
    return [list(flat[e - c:e]) for c, e in zip(counts, ends)]


def compare_solver_on_families(solve, live=False):
    """solve(family) -> per sample the list of models of the implementation under test. Every model of every family is a valid
    essential matrix; on the generic families they are sfm_ref.five_point's models within 1e-9, at most 0.3 % of the samples
    excepted. live: the restatement is run here (slow: the host test does) on all nine families, its models are held to the
    validity property too and the record to them; otherwise the recorded models stand for it. Returns the models seen per family."""
    seen, off, total = {}, 0, 0
    for fam in FAMILIES:
        got = solve(fam)
        want = restatement_models(fam) if live else recorded_models(fam) if fam in GENERIC_FAMILIES else [[]] * 300
        if live and fam in GENERIC_FAMILIES:
            rec = recorded_models(fam)
            assert [len(w) for w in want] == [len(r) for r in rec] and all(np.abs(a - b).max() < 1e-12 for w, r in zip(want, rec) for a, b in zip(w, r))
        assert len(got) == len(want) == 300
        for s, (g, w) in enumerate(zip(got, want)):
            for m in g:
                assert_valid_model(m, (fam, s, "under test"))
            for m in w:
                assert_valid_model(m, (fam, s, "restatement"))
            if fam in GENERIC_FAMILIES:
                total += 1
                off += len(g) != len(w) or any(np.abs(a - b).max() > 1e-9 for a, b in zip(g, w))
        seen[fam] = sum(len(g) for g in got)
    assert total == 1200 and off <= 0.003 * total, off
    assert all(seen[f] > 1000 for f in GENERIC_FAMILIES), seen
    return seen


# ---- two-view scenes for RANSAC --------------------------------------------------------------------------------------------------------
def scene(seed, n, outliers, R=BASE_R, t=BASE_T, camera=BASE_CAMERA, noise=0.3, planar=False, integer=False, repeat=1, line1=False,
          line2=False):
    """n correspondences (fp32 pixels) of points at depth 4-9 seen under (R, t), a fraction `outliers` of the second image's points
    replaced by uniform ones. repeat: every correspondence occurs about that many times. line1 / line2: the image's points are moved
    onto a line (which destroys the geometry: a degenerate input)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = camera
    k = max(1, -(-n // repeat))
    X = np.stack([rng.uniform(-2.2, 2.2, k), rng.uniform(-1.2, 1.2, k), rng.uniform(4, 9, k)], axis=1)
    if planar:
        X[:, 2] = 6.0 + 0.2 * X[:, 0] - 0.1 * X[:, 1]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    p1, p2 = X @ K.T, (X @ np.asarray(R).T + np.asarray(t)) @ K.T
    uv1 = p1[:, :2] / p1[:, 2:3] + rng.normal(0, noise, (k, 2))
    uv2 = p2[:, :2] / p2[:, 2:3] + rng.normal(0, noise, (k, 2))
    wrong = rng.uniform(size=k) < outliers
    uv2[wrong] = np.stack([rng.uniform(0, 2 * cx, int(wrong.sum())), rng.uniform(0, 2 * cy, int(wrong.sum()))], axis=1)
    if integer:
        uv1, uv2 = np.rint(uv1), np.rint(uv2)
    if line1:
        uv1[:, 1] = cy + 0.1 * (uv1[:, 0] - cx)
    if line2:
        uv2[:, 1] = cy - 0.3 * (uv2[:, 0] - cx)
    if repeat > 1:
        pick = rng.permutation(np.tile(np.arange(k), repeat)[:n]) if n > 0 else np.zeros(0, dtype=np.int64)
        uv1, uv2 = uv1[pick], uv2[pick]
    return np.ascontiguousarray(uv1[:n], dtype=np.float32), np.ascontiguousarray(uv2[:n], dtype=np.float32)


MOTIONS = {
    "forward": dict(R=rot([0.01, 0.02, 0.0]), t=np.array([0.02, -0.03, 0.8])),
    "backward": dict(R=np.eye(3), t=np.array([0.05, 0.0, -0.9])),
    "roll_90": dict(R=rot([0.02, 0.05, np.pi / 2]), t=np.array([0.4, 0.3, 0.1])),
    "yaw_30": dict(R=rot([0.0, np.deg2rad(30.0), 0.0]), t=np.array([-3.0, 0.0, 0.8])),
    "vertical": dict(R=rot([np.deg2rad(5.0), 0.0, 0.0]), t=np.array([0.0, 0.7, 0.0])),
    "planar": dict(planar=True),
    "integer_pixel": dict(integer=True),
    "repeated_8x": dict(repeat=8),
    "baseline_1e-3": dict(t=BASE_T * 1e-3),
    "no_translation": dict(t=np.zeros(3)),
}
# (seed, n, outliers, prob): the restatement's 50 % / 0.999 runs take seconds each -- three motions keep them, the others run at 0.99
MOTION_CONFIGS = [(1, 300, 0.3, 0.7), (2, 257, 0.5, 0.999), (3, 127, 0.1, 0.99)]
FULL_CONFIDENCE_MOTIONS = ("forward", "roll_90", "no_translation")


def ransac_cases():
    """{name: (scene keyword arguments, camera, prob, threshold, max_iters)} -- every configuration on which the host core, the
    kernels and the restatement must make the same decisions."""
    cases = {}
    for name, kw in MOTIONS.items():
        for seed, n, outl, prob in MOTION_CONFIGS:
            if prob == 0.999 and name not in FULL_CONFIDENCE_MOTIONS:
                prob = 0.99
            cases[f"{name}-{n}"] = (dict(seed=seed, n=n, outliers=outl, **kw), BASE_CAMERA, prob, 1.0, 1000)
    for n in N_LIST:
        cases[f"n-{n}"] = (dict(seed=100 + n, n=n, outliers=0.3), BASE_CAMERA, 0.7, 1.0, 1000)
    for mi in MAX_ITERS_LIST:
        cases[f"max_iters-{mi}"] = (dict(seed=200 + mi, n=200, outliers=0.6), BASE_CAMERA, 0.999, 1.0, mi)
    for th in THRESHOLDS:
        cases[f"threshold-{th}"] = (dict(seed=300, n=300, outliers=0.3), BASE_CAMERA, 0.7, th, 1000)
    for i, cam in enumerate(CAMERAS):
        cases[f"camera-{i}"] = (dict(seed=400 + i, n=300, outliers=0.3, camera=cam), cam, 0.7, 1.0, 1000)
    return cases


RANSAC_CASES = ransac_cases()

DEGENERATE_CASES = {
    "line1-300": (dict(seed=1, n=300, outliers=0.3, line1=True), BASE_CAMERA, 0.7, 1.0, 1000),
    "line1-127": (dict(seed=3, n=127, outliers=0.1, line1=True), BASE_CAMERA, 0.99, 1.0, 1000),
    "line_both-200": (dict(seed=5, n=200, outliers=0.3, line1=True, line2=True), BASE_CAMERA, 0.7, 1.0, 1000),
    "line1-5": (dict(seed=6, n=5, outliers=0.0, line1=True), BASE_CAMERA, 0.7, 1.0, 1000),
}


@functools.lru_cache(maxsize=None)
def case_scene(name):
    kw = (RANSAC_CASES.get(name) or DEGENERATE_CASES[name])[0]
    uv1, uv2 = scene(**kw)
    uv1.setflags(write=False)
    uv2.setflags(write=False)
    return uv1, uv2


@functools.lru_cache(maxsize=None)
def restatement_ransac(name):
    """(E or None, mask, iterations) of sfm_ref.find_essential_mat on the named case"""
    _, camera, prob, threshold, max_iters = RANSAC_CASES.get(name) or DEGENERATE_CASES[name]
    uv1, uv2 = case_scene(name)
    E, mask, iters = sfm_ref.find_essential_mat(uv1, uv2, camera, prob, threshold, max_iters)
    mask.setflags(write=False)
    return E, mask, iters


@functools.lru_cache(maxsize=None)
def recorded_ransac(name):
    """restatement_ransac(name) as recorded"""
    z = _golden()
    E = z[f"ransac_E_{name}"]
    return (E if E.any() else None), z[f"ransac_mask_{name}"], int(z[f"ransac_iters_{name}"])


def assert_record_is_the_restatement(name):
    (E, mask, iters), (rE, rmask, riters) = restatement_ransac(name), recorded_ransac(name)
    assert iters == riters and np.array_equal(mask, rmask) and (E is None) == (rE is None), name
    assert E is None or np.abs(E - rE).max() < 1e-12, name


def sampson_mask(E, uv1, uv2, camera, threshold):
    fx, fy, cx, cy = camera
    x1 = np.stack([(uv1[:, 0].astype(np.float64) - cx) / fx, (uv1[:, 1].astype(np.float64) - cy) / fy], axis=1)
    x2 = np.stack([(uv2[:, 0].astype(np.float64) - cx) / fx, (uv2[:, 1].astype(np.float64) - cy) / fy], axis=1)
    thr = threshold / ((fx + fy) / 2)
    return (sfm_ref.sampson_errors(np.asarray(E).reshape(3, 3), x1, x2) <= np.float32(thr * thr)).astype(np.uint8)


def assert_ransac_properties(name, E, mask, count, iters):
    """What holds of ANY implementation's answer on a degenerate input: no model, or a valid essential matrix; the mask is the Sampson
    test of the returned E (every point, for exactly five); the count is the mask's; the iteration bound is kept."""
    _, camera, _, threshold, max_iters = DEGENERATE_CASES[name]
    uv1, uv2 = case_scene(name)
    assert iters <= max(max_iters, 1) and count == int(np.asarray(mask).sum()), (name, iters, count)
    if E is None or not np.asarray(E).any():
        assert count == 0, name
        return
    assert_valid_model(E, name)
    want = np.ones(5, dtype=np.uint8) if len(uv1) == 5 else sampson_mask(E, uv1, uv2, camera, threshold)
    assert np.array_equal(np.asarray(mask), want), name
    # one image on a line, the other not: no essential matrix takes every correspondence (only a rank-one matrix does). With BOTH
    # images on lines a valid E can -- the two lines as a pair of corresponding epipolar lines -- and all points may be inliers.
    if not DEGENERATE_CASES[name][0].get("line2") and len(uv1) > 5:
        assert count < len(uv1), (name, "every point an inlier of a line-degenerate input")


# ---- recoverPose: scenes in which a chosen one of the four hypotheses is the true pose ----------------------------------------------------
def random_essential(rng):
    R, t = rot(rng.uniform(-0.4, 0.4, 3)), rng.normal(size=3)
    t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R * rng.uniform(0.2, 4.0) * rng.choice([-1.0, 1.0])


def hypothesis_scene(rng, E, h, n=600, camera=BASE_CAMERA, noise=0.3):
    """n correspondences (fp32 pixels) in front of both cameras of hypothesis h of sfm_ref.decompose_essential(E); returns
    (uv1, uv2, R, t) with (R, t) that hypothesis."""
    R1, R2, t = sfm_ref.decompose_essential(E)
    R, tt = [(R1, t), (R2, t), (R1, -t), (R2, -t)][h]
    fx, fy, cx, cy = camera
    X = np.zeros((0, 3))
    while len(X) < n:
        c = np.stack([rng.uniform(-8, 8, 2 * n), rng.uniform(-8, 8, 2 * n), rng.uniform(0.5, 12, 2 * n)], axis=1)
        X = np.concatenate([X, c[(c @ R.T + tt)[:, 2] > 0.5]])
    X = X[:n]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    p1, p2 = X @ K.T, (X @ R.T + tt) @ K.T
    uv1 = (p1[:, :2] / p1[:, 2:3] + rng.normal(0, noise, (n, 2))).astype(np.float32)
    uv2 = (p2[:, :2] / p2[:, 2:3] + rng.normal(0, noise, (n, 2))).astype(np.float32)
    return uv1, uv2, R, tt


def hypothesis_masks(E, uv1, uv2, camera=BASE_CAMERA, dist_thresh=50.0):
    """sfm_ref.recover_pose's four cheirality masks [4, n] (bool), the per-point SVDs batched: the same matrices through the same
    LAPACK routine. (R, t) of the four hypotheses are returned as well."""
    fx, fy, cx, cy = camera
    uv1, uv2 = np.asarray(uv1, dtype=np.float64), np.asarray(uv2, dtype=np.float64)
    x1 = np.stack([(uv1[:, 0] - cx) / fx, (uv1[:, 1] - cy) / fy], axis=1)
    x2 = np.stack([(uv2[:, 0] - cx) / fx, (uv2[:, 1] - cy) / fy], axis=1)
    R1, R2, t = sfm_ref.decompose_essential(E)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    poses, masks = [(R1, t), (R2, t), (R1, -t), (R2, -t)], []
    for R, tt in poses:
        P = np.hstack([R, tt.reshape(3, 1)])
        A = np.stack([x1[:, 0:1] * P0[2] - P0[0], x1[:, 1:2] * P0[2] - P0[1], x2[:, 0:1] * P[2] - P[0], x2[:, 1:2] * P[2] - P[1]], axis=1)
        Q = np.linalg.svd(A)[2][:, 3, :]
        q = Q[:, :3] / Q[:, 3:4]
        z2 = q @ P[2, :3] + P[2, 3]
        masks.append((Q[:, 2] * Q[:, 3] > 0) & (q[:, 2] < dist_thresh) & (z2 > 0) & (z2 < dist_thresh))
    return np.array(masks), poses


def recover_pose_batched(E, uv1, uv2, camera=BASE_CAMERA, in_mask=None):
    """sfm_ref.recover_pose with hypothesis_masks in place of its per-point loop: (R, t, n_good, mask uint8, winner index)"""
    masks, poses = hypothesis_masks(E, uv1, uv2, camera)
    if in_mask is not None:
        masks = masks & (np.asarray(in_mask) != 0)
    good = [int(m.sum()) for m in masks]
    w = good.index(max(good))          # recoverPose's chain of comparisons: the first hypothesis with the most points
    out = np.where(masks[w], 255 if in_mask is None else np.asarray(in_mask, dtype=np.uint8), 0).astype(np.uint8)
    return poses[w][0], poses[w][1], good[w], out, w
