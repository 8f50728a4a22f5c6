"""The dense stage of a posed pair as sfm-gms_amd/csrc/rectify_core.h defines it, in numpy: the rectifying plan,
the rectified image with its valid plane, and the points of a disparity map. fp64, only + - * / sqrt rint, every sum written out in
the header's order; no `@` and no np.linalg (a BLAS may fuse products into sums). The GPU, the host build of the header and this file
agree bit for bit."""
import math

import numpy as np

GMS_OK, GMS_ERR_NO_MODEL = 0, -8
PLAN_DTYPE = np.dtype([("R1", "<f8", (9,)), ("R2", "<f8", (9,)), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("B", "<f8"),
                       ("out_w", "<i4"), ("out_h", "<i4"), ("turn", "<i4"), ("status", "<i4")])
assert PLAN_DTYPE.itemsize == 200


def _mul33(A, B):
    return [A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]


def _mul3v(A, v):
    return [A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2] for r in range(3)]


def _mul3tv(A, v):
    return [A[c] * v[0] + A[3 + c] * v[1] + A[6 + c] * v[2] for c in range(3)]


def _floats(a, n):
    a = [float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1)]
    assert len(a) == n
    return a


def undistort_point(camera, dist, u, v):
    """tv::undistort_point: cv::undistortPoints' five fixed-point iterations."""
    fx, fy, cx, cy = camera
    k1, k2, p1, p2, k3 = dist
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0, y0
    if k1 != 0.0 or k2 != 0.0 or p1 != 0.0 or p2 != 0.0 or k3 != 0.0:
        for _ in range(5):
            r2 = x * x + y * y
            icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
    return x, y


def zero_plan(status=GMS_ERR_NO_MODEL):
    p = np.zeros(1, PLAN_DTYPE)
    p["status"] = status
    return p


def _corner_mean(camera, dist, Rk, W, H):
    sx = sy = 0.0
    for u, v in ((0.0, 0.0), (float(W - 1), 0.0), (float(W - 1), float(H - 1)), (0.0, float(H - 1))):
        x, y = undistort_point(camera, dist, u, v)
        p = _mul3v(Rk, [x, y, 1.0])
        if not p[2] > 0.0:
            return None
        sx += p[0] / p[2]
        sy += p[1] / p[2]
    return sx * 0.25, sy * 0.25


def make_plan(camera, dist, R, t, size, out_size=None):
    """rect::make_plan -> a one-record PLAN_DTYPE array. camera (fx, fy, cx, cy), dist (k1, k2, p1, p2, k3) or None, size (W, H)."""
    camera = _floats(camera, 4)
    dist = _floats(dist if dist is not None else np.zeros(5), 5)
    R, t = _floats(R, 9), _floats(t, 3)
    W, H = int(size[0]), int(size[1])
    P = zero_plan()
    tr = R[0] + R[4] + R[8]
    if not tr > 0.0:
        return P
    w = math.sqrt(1.0 + tr) / 2.0
    d4 = 4.0 * w
    x0, y0, z0, w0 = (R[7] - R[5]) / d4, (R[2] - R[6]) / d4, (R[3] - R[1]) / d4, 1.0 + w
    qn = math.sqrt(w0 * w0 + x0 * x0 + y0 * y0 + z0 * z0)
    qw, qx, qy, qz = w0 / qn, x0 / qn, y0 / qn, z0 / qn
    Rh = [1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy + qw * qz), 2.0 * (qx * qz - qw * qy),
          2.0 * (qx * qy - qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz + qw * qx),
          2.0 * (qx * qz + qw * qy), 2.0 * (qy * qz - qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]
    b = [-v for v in _mul3v(Rh, t)]
    if abs(b[0]) >= abs(b[1]):
        turn = 0 if b[0] > 0.0 else 1
    else:
        turn = 2 if b[1] > 0.0 else 3
    Z = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0],
         [0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]][turn]
    g = _mul3v(Z, b)
    if not g[0] > 0.0 or not g[0] >= abs(g[2]):
        return P
    B = math.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    ay, az, h = g[1] / B, g[2] / B, 1.0 + g[0] / B
    A = [1.0 - (ay * ay + az * az) / h, ay, az,
         -ay, 1.0 - (ay * ay) / h, -(ay * az) / h,
         -az, -(ay * az) / h, 1.0 - (az * az) / h]
    Wm = _mul33(A, Z)
    R2 = _mul33(Wm, Rh)
    R1 = _mul33(R2, R)
    if out_size is not None and out_size[0] > 0 and out_size[1] > 0:
        ow, oh = int(out_size[0]), int(out_size[1])
    else:
        ow, oh = (W, H) if turn < 2 else (H, W)
    f = camera[0] if camera[0] < camera[1] else camera[1]
    m1 = _corner_mean(camera, dist, R1, W, H)
    m2 = _corner_mean(camera, dist, R2, W, H) if m1 is not None else None
    if m1 is None or m2 is None:
        return P
    hx, hy = float(ow - 1) / 2.0, float(oh - 1) / 2.0
    c1x, c1y, c2x, c2y = hx - f * m1[0], hy - f * m1[1], hx - f * m2[0], hy - f * m2[1]
    P["R1"][0], P["R2"][0] = R1, R2
    P["fx"] = P["fy"] = f
    P["cx"], P["cy"], P["B"] = (c1x + c2x) * 0.5, (c1y + c2y) * 0.5, B
    P["out_w"], P["out_h"], P["turn"], P["status"] = ow, oh, turn, GMS_OK
    return P


def identity_plan(camera, size):
    """rect::identity_plan: cv::undistort as a plan."""
    P = zero_plan(GMS_OK)
    for k in ("R1", "R2"):
        P[k][0][[0, 4, 8]] = 1.0
    P["fx"], P["fy"], P["cx"], P["cy"] = [float(v) for v in camera]
    P["out_w"], P["out_h"] = size
    return P


def plan_q(plan):
    p = np.asarray(plan).reshape(-1)[0]
    Q = np.zeros((4, 4))
    Q[0, 0] = Q[1, 1] = 1.0
    Q[0, 3], Q[1, 3], Q[2, 3] = -p["cx"], -p["cy"], p["fx"]
    Q[3, 2] = 1.0 / p["B"] if p["B"] != 0.0 else 0.0
    return Q


def _round_i32(v):
    r = np.rint(v)
    with np.errstate(invalid="ignore"):
        r = np.where(~(r >= -2147483648.0), -2147483648.0, np.where(r >= 2147483647.0, 2147483647.0, r))
    return r.astype(np.int64)


def source_positions(camera, dist, plan, which, out_size):
    """Per destination pixel of out_size (W', H'): ix, iy (saturated to int16), the 5-bit fractions fx, fy and front (0: z <= 0), as
    int64 / bool arrays [H', W']. A plan that is not ok: front 0 everywhere."""
    fx, fy, cx, cy = _floats(camera, 4)
    k1, k2, p1, p2, k3 = _floats(dist if dist is not None else np.zeros(5), 5)
    p = np.asarray(plan).reshape(-1)[0]
    Rk = _floats(p["R2"] if which == 2 else p["R1"], 9)
    dw, dh = int(out_size[0]), int(out_size[1])
    with np.errstate(all="ignore"):
        xn = ((np.arange(dw, dtype=np.float64) - float(p["cx"])) / float(p["fx"]))[None, :]
        yn = ((np.arange(dh, dtype=np.float64) - float(p["cy"])) / float(p["fy"]))[:, None]
        r0 = Rk[0] * xn + (Rk[3] * yn + Rk[6])
        r1 = Rk[1] * xn + (Rk[4] * yn + Rk[7])
        r2 = Rk[2] * xn + (Rk[5] * yn + Rk[8])
        front = (r2 > 0.0) & (int(p["status"]) == GMS_OK)
        x, y = r0 / r2, r1 / r2
        rr = x * x + y * y
        kr = 1.0 + ((k3 * rr + k2) * rr + k1) * rr
        xd = x * kr + 2.0 * p1 * x * y + p2 * (rr + 2.0 * x * x)
        yd = y * kr + p1 * (rr + 2.0 * y * y) + 2.0 * p2 * x * y
        SX, SY = _round_i32((fx * xd + cx) * 32.0), _round_i32((fy * yd + cy) * 32.0)
    ix, iy = np.clip(SX >> 5, -32768, 32767), np.clip(SY >> 5, -32768, 32767)
    z = np.zeros_like(ix)
    return np.where(front, ix, z), np.where(front, iy, z), np.where(front, SX & 31, z), np.where(front, SY & 31, z), front


def rectify(image, camera, dist, plan, which, out_size=None):
    """The rectified image [H', W'(, 3)] of camera `which` (1 or 2) and its valid plane [H', W'] (1: all four taps inside)."""
    p = np.asarray(plan).reshape(-1)[0]
    if out_size is None:
        out_size = (int(p["out_w"]), int(p["out_h"]))
    image = np.asarray(image)
    assert image.dtype == np.uint8 and (image.ndim == 2 or (image.ndim == 3 and image.shape[2] == 3))
    sh, sw = image.shape[:2]
    ix, iy, fx, fy, front = source_positions(camera, dist, plan, which, out_size)
    src = image.reshape(sh, sw, -1).astype(np.int64)

    def tap(x, y):
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        v = src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]
        return np.where(inside[..., None], v, 0)

    fx_, fy_ = fx[..., None], fy[..., None]
    out = (tap(ix, iy) * (32 - fx_) * (32 - fy_) + tap(ix + 1, iy) * fx_ * (32 - fy_) + tap(ix, iy + 1) * (32 - fx_) * fy_ +
           tap(ix + 1, iy + 1) * fx_ * fy_ + 512) >> 10
    out = np.where(front[..., None], out, 0).astype(np.uint8)
    valid = (front & (ix >= 0) & (ix + 1 < sw) & (iy >= 0) & (iy + 1 < sh)).astype(np.uint8)
    return out.reshape((out_size[1], out_size[0]) + image.shape[2:]), valid


def undistort(image, camera, dist):
    image = np.asarray(image)
    return rectify(image, camera, dist, identity_plan(camera, (image.shape[1], image.shape[0])), 1)[0]


def cloud(disp16, valid, image, plan, filtered16, min_disp16=16, S=None, view=None):
    """The points of one int16 map in raster order: xyz float32 [k, 3], the bytes of `image` at them [k(, 3)] (None without an
    image), pixel int32 [k] = v W' + u. S and view = (R [9], t [3]) of frame_a: the world frame of the registration."""
    disp16, valid = np.asarray(disp16), np.asarray(valid)
    p = np.asarray(plan).reshape(-1)[0]
    H, W = disp16.shape
    d = disp16.astype(np.int64)
    is_pt = (d != filtered16) & (d >= min_disp16) & (valid != 0) & (int(p["status"]) == GMS_OK)
    v, u = np.nonzero(is_pt)
    dd = d[v, u].astype(np.float64)
    f, B, R1 = float(p["fx"]), float(p["B"]), _floats(p["R1"], 9)
    Zc = f * B * 16.0 / dd
    c = [(u.astype(np.float64) - float(p["cx"])) * Zc / f, (v.astype(np.float64) - float(p["cy"])) * Zc / f, Zc]
    pt = _mul3tv(R1, c)
    if view is not None:
        GR, Gt = _floats(view[0], 9), _floats(view[1], 3)
        q = [float(S) * pt[i] - Gt[i] for i in range(3)]
        pt = _mul3tv(GR, q)
    xyz = np.stack(pt, axis=1).astype(np.float32).reshape(-1, 3)
    colors = None if image is None else np.asarray(image)[v, u]
    return xyz, colors, (v * W + u).astype(np.int32)
