"""The cases of the dense stage's tests, shared by tests/test_rectify_ref.py (CPU) and tests/test_gpu_rectify.py /
tests/test_gpu_dense.py (GPU): the poses the plan must turn, tie and refuse, the cameras, and a rendered plane of known depth.
tests/test_rectify_ref.py asserts that each case holds what it is named for. Nothing here is part of the statement: rotations come
from math.cos / math.sin and the scene uses numpy's matrix product."""
import math

import numpy as np

CAMERA_SMALL = (40.0, 41.0, 18.2, 14.1)            # for the 37 x 29 and 67 x 45 images
DIST_ALL = (0.1, -0.05, 0.01, -0.02, 0.03)         # all five coefficients non-zero
CAMERA_WIDE = (5.0, 5.0, 18.0, 14.0)               # 37 x 29 with corners 75 degrees off the axis
SIZE_SMALL = (37, 29)


def rot(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    a = a / math.sqrt(float(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]))
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


I3 = np.eye(3)
# name: (camera, R, t, expected status (0 ok, -8 refused), expected turn or None)
PLAN_CASES = {
    "t_minus_x": (CAMERA_SMALL, I3, (-1.0, 0.0, 0.0), 0, 0),
    "t_plus_x": (CAMERA_SMALL, I3, (1.0, 0.0, 0.0), 0, 1),
    "t_minus_y": (CAMERA_SMALL, I3, (0.0, -1.0, 0.0), 0, 2),
    "t_plus_y": (CAMERA_SMALL, I3, (0.0, 1.0, 0.0), 0, 3),
    "diagonal_tie": (CAMERA_SMALL, I3, (-1.0, -1.0, 0.0), 0, 0),            # |b_x| = |b_y|: x wins
    "diagonal_tie_negative": (CAMERA_SMALL, I3, (1.0, -1.0, 0.0), 0, 1),
    "rot10_x": (CAMERA_SMALL, rot((1, 0, 0), 10), (-1.0, 0.1, 0.05), 0, 0),
    "rot10_y": (CAMERA_SMALL, rot((0, 1, 0), 10), (-1.0, 0.1, 0.05), 0, 0),
    "rot10_z": (CAMERA_SMALL, rot((0, 0, 1), 10), (-1.0, 0.1, 0.05), 0, 0),
    "rot10_z_vertical": (CAMERA_SMALL, rot((0, 0, 1), 10), (0.2, 1.0, -0.3), 0, 3),
    "trace_zero": (CAMERA_SMALL, np.diag([-1.0, -1.0, 1.0]), (-1.0, 0.0, 0.0), -8, None),       # tr = -1
    "trace_negative_121": (CAMERA_SMALL, rot((0, 0, 1), 121), (-1.0, 0.0, 0.0), -8, None),      # tr = 1 + 2 cos 121 < 0
    "baseline_out_of_plane": (CAMERA_SMALL, I3, (-0.5, 0.0, -1.0), -8, None),                   # g_x = 0.5 < |g_z| = 1
    "baseline_along_axis": (CAMERA_SMALL, I3, (0.0, 0.0, 1.0), -8, None),                       # g_x = 0
    "corner_behind": (CAMERA_WIDE, rot((0, 1, 0), 40), (-1.0, 0.0, 0.0), -8, None),             # 75 + 20 degrees > 90
}
OK_PLANS = tuple(k for k, v in PLAN_CASES.items() if v[3] == 0)


def plan_inputs(name):
    cam, R, t, status, turn = PLAN_CASES[name]
    dist = None if name.startswith("t_") or cam is CAMERA_WIDE else DIST_ALL   # (the wide camera is outside the polynomial's range)
    return cam, dist, np.ascontiguousarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64), status, turn


def noise(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- a textured plane of known depth in two 96 x 72 cameras --------------------------------------------------------------------------
SCENE_SIZE = (96, 72)
SCENE_CAMERA = (90.0, 90.0, 47.5, 35.5)
SCENE_R = rot((0.3, 1.0, 0.2), 5.0)
SCENE_T = np.array([-1.0, 0.25, 0.05])
SCENE_PLANE = (np.array([-0.05, 0.02, 1.0]), 7.5)     # n . X = d in camera 1's frame: depth about 7.5 baselines, slightly tilted
SCENE_SGM = dict(num_disparities=32, min_disparity=0)
SCENE_SEED = 11
# The share of the statement's cloud points whose depth is within the equivalent of 1 px of disparity of the plane, measured on the
# numpy chain (rectify_ref.rectify -> stereo_sgm_ref.stereo_sgm -> rectify_ref.cloud) for this scene; the test asserts it less a margin
# of 0.05, which is for a later change of the texture seed (the GPU must equal the statement).
SCENE_SHARE_MEASURED = 0.9977     # 4003 of 4012 points
SCENE_SHARE_MARGIN = 0.05


def _texture(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (256, 256)).astype(np.float64)


def _tex_at(tex, X, Y, cell=0.22):
    """Bilinear lookup of the noise grid at plane coordinates (one grid cell = `cell` units, about 2.5 px at the plane's depth)."""
    gx, gy = X / cell + 128.0, Y / cell + 128.0
    x0, y0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    fx, fy = gx - x0, gy - y0
    x0, y0 = x0 % 255, y0 % 255
    return (tex[y0, x0] * (1 - fx) * (1 - fy) + tex[y0, x0 + 1] * fx * (1 - fy) + tex[y0 + 1, x0] * (1 - fx) * fy + tex[y0 + 1, x0 + 1] * fx * fy)


def scene():
    """(img1, img2) uint8 [72, 96]: the plane rendered into camera 1 ([I | 0]) and camera 2 ([R | t]); no distortion."""
    W, H = SCENE_SIZE
    f, _, cx, cy = SCENE_CAMERA
    n, d = SCENE_PLANE
    tex = _texture(SCENE_SEED)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], axis=-1)            # [H, W, 3]
    out = []
    for R, t in ((np.eye(3), np.zeros(3)), (SCENE_R, SCENE_T)):
        dirs = rays @ R                                                                # R^T r per pixel
        origin = -(R.T @ t)                                                            # the camera's centre in frame 1
        lam = (d - n @ origin) / (dirs @ n)
        X = origin + lam[..., None] * dirs
        out.append(np.clip(np.rint(_tex_at(tex, X[..., 0], X[..., 1])), 0, 255).astype(np.uint8))
    return out[0], out[1]


def scene_depth_error_share(xyz):
    """The share of points (camera 1's frame) whose depth along camera 1's axis is within the equivalent of 1 px of disparity of the
    plane's depth on their ray: |f B / Z - f B / Z_plane| <= 1."""
    n, d = SCENE_PLANE
    f = SCENE_CAMERA[0]
    B = math.sqrt(float(SCENE_T @ SCENE_T))
    xyz = np.asarray(xyz, dtype=np.float64)
    z_plane = d * xyz[:, 2] / (xyz @ n)     # the plane's point on the ray through the cloud point
    return float(np.mean(np.abs(f * B / xyz[:, 2] - f * B / z_plane) <= 1.0)) if len(xyz) else 0.0


def scene_chain():
    """The statement's chain on the scene: (plan, rect1, rect2, valid1, disp16, (xyz, colors, pixel)) in camera 1's frame."""
    import rectify_ref
    import stereo_sgm_ref
    img1, img2 = scene()
    P = rectify_ref.make_plan(SCENE_CAMERA, None, SCENE_R, SCENE_T, SCENE_SIZE)
    r1, v1 = rectify_ref.rectify(img1, SCENE_CAMERA, None, P, 1)
    r2, _ = rectify_ref.rectify(img2, SCENE_CAMERA, None, P, 2)
    disp, _ = stereo_sgm_ref.stereo_sgm(r1, r2, **SCENE_SGM)
    return P, r1, r2, v1, disp, rectify_ref.cloud(disp, v1, r1, P, (SCENE_SGM["min_disparity"] - 1) * 16, 16)
