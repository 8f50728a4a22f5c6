"""Camera calibration from chessboard photographs as this library defines it, in numpy: the statement that
sfm-gms_amd/csrc/calib_core.h (host build: tests/cpp/calib_host.cpp) and calib_kernels.hip are held against. The corner finder and the
ordering are the library's OWN definition, not OpenCV's quad-based findChessboardCorners; cornerSubPix follows OpenCV 4.5.2's algorithm
as read from its source, in fp64; calibrateCamera follows its structure (closed-form start, Levenberg-Marquardt on the reprojection
error). Parity with an OpenCV build is unpinned.

  response(img)                 R, uint32 [H, W]                                   (vectorised)
  response_literal(img, x, y)   the same number for one pixel, from the definition
  peaks(R)                      bool [H, W]
  candidates(img, max_cand)     records CAND_DTYPE in descending R, then raster order
  order_board(points, nx, ny)   (found, [nx * ny, 2]) in findChessboardCorners' order
  corner_subpix(img, corners)   cornerSubPix(win (5, 5), zeroZone (-1, -1), (30, 0.1))
  calibrate_camera(obj, img, size)"""
import numpy as np

BORDER = 16          # GMS_DETECT_BORDER
D = 4                # the arm of the second differences
NMS_R = 8            # peaks: 17 x 17
MAX_CANDIDATES = 4096
CAND_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("response", "<u4")])

S_MAX = 255 * 25 * 25            # 159 375
DIFF_MAX = 2 * S_MAX             # |sxx|, |syy|, |sxy| <= 318 750
assert S_MAX == 159375 and DIFF_MAX == 318750
assert DIFF_MAX ** 2 + 4 * DIFF_MAX ** 2 < 2 ** 39 and (DIFF_MAX ** 2 + 4 * DIFF_MAX ** 2) >> 10 < 2 ** 29


def _box5(a):
    """5 x 5 box sums with zeros outside (what lies outside never reaches a pixel that is not forced to 0)."""
    p = np.pad(a, 2)
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), axis=0), axis=1)
    return c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]


def _shift(a, dx, dy):
    """a[y + dy, x + dx], zeros outside"""
    h, w = a.shape
    out = np.zeros_like(a)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def response(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    S = _box5(_box5(img.astype(np.int64)))
    assert S.max(initial=0) <= S_MAX
    sxx = _shift(S, D, 0) + _shift(S, -D, 0) - 2 * S
    syy = _shift(S, 0, D) + _shift(S, 0, -D) - 2 * S
    sxy = _shift(S, D, D) + _shift(S, -D, -D) - _shift(S, D, -D) - _shift(S, -D, D)
    assert max(np.abs(sxx).max(initial=0), np.abs(syy).max(initial=0), np.abs(sxy).max(initial=0)) <= DIFF_MAX
    R = np.maximum(0, sxy * sxy - 4 * sxx * syy) >> 10
    assert R.max(initial=0) < 2 ** 29
    out = np.zeros((h, w), np.uint32)
    if w > 2 * BORDER and h > 2 * BORDER:
        out[BORDER:h - BORDER, BORDER:w - BORDER] = R[BORDER:h - BORDER, BORDER:w - BORDER]
    return out


def response_literal(img, x, y):
    """R at one pixel, straight from the definition (python integers)."""
    h, w = img.shape
    if x < BORDER or y < BORDER or x >= w - BORDER or y >= h - BORDER:
        return 0

    def B(u, v):
        return sum(int(img[v + j, u + i]) for j in range(-2, 3) for i in range(-2, 3))

    def S(u, v):
        return sum(B(u + i, v + j) for j in range(-2, 3) for i in range(-2, 3))

    s = S(x, y)
    sxx = S(x + D, y) + S(x - D, y) - 2 * s
    syy = S(x, y + D) + S(x, y - D) - 2 * s
    sxy = S(x + D, y + D) + S(x - D, y - D) - S(x + D, y - D) - S(x - D, y + D)
    return max(0, sxy * sxy - 4 * sxx * syy) >> 10


def peaks(R):
    """R > 0, greater than every 17 x 17 neighbour earlier in raster order, not smaller than any later one."""
    R = R.astype(np.int64)
    ok = R > 0
    for dy in range(-NMS_R, NMS_R + 1):
        for dx in range(-NMS_R, NMS_R + 1):
            if dx == 0 and dy == 0:
                continue
            nb = _shift(R, dx, dy)
            ok &= (R > nb) if (dy < 0 or (dy == 0 and dx < 0)) else (R >= nb)
    return ok


def peaks_literal(R, x, y):
    h, w = R.shape
    r = int(R[y, x])
    if r <= 0:
        return False
    for dy in range(-NMS_R, NMS_R + 1):
        for dx in range(-NMS_R, NMS_R + 1):
            u, v = x + dx, y + dy
            if (dx == 0 and dy == 0) or u < 0 or v < 0 or u >= w or v >= h:
                continue
            nb = int(R[v, u])
            if (r <= nb) if (dy < 0 or (dy == 0 and dx < 0)) else (r < nb):
                return False
    return True


def peak_capacity(w, h):
    """Two peaks are more than 8 apart in x or in y, so every 9 x 9 cell of the inner region holds at most one."""
    if w <= 2 * BORDER or h <= 2 * BORDER:
        return 0
    return ((w - 2 * BORDER + 8) // 9) * ((h - 2 * BORDER + 8) // 9)


def candidates_from(R, max_candidates=256):
    assert 1 <= max_candidates <= MAX_CANDIDATES
    ys, xs = np.nonzero(peaks(R))                      # raster order
    assert len(xs) <= peak_capacity(R.shape[1], R.shape[0])
    r = R[ys, xs]
    keep = np.argsort(-r.astype(np.int64), kind="stable")[:max_candidates]
    out = np.zeros(len(keep), CAND_DTYPE)
    out["x"], out["y"], out["response"] = xs[keep], ys[keep], r[keep]
    return out


def candidates(img, max_candidates=256):
    return candidates_from(response(img), max_candidates)


# ---- ordering onto the board ---------------------------------------------------------------------------------------------------------
# integer directions (a, b) of the rotated frames, 0 .. 79 degrees; the frame's axes are (a, b) and (-b, a)
FRAMES = ((1, 0), (5, 1), (5, 2), (5, 3), (5, 4), (1, 1), (4, 5), (3, 5), (2, 5), (1, 5))
CELL_TOL = 0.25


def _fit_h(src, dst):
    """The homography src -> dst with h33 = 1, least squares on the 2n linear equations (normal equations, fp64)."""
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    z, o = np.zeros_like(x), np.ones_like(x)
    A = np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y], 1), np.stack([z, z, z, x, y, o, -v * x, -v * y], 1)])
    b = np.concatenate([u, v])
    try:
        hvec = np.linalg.solve(A.T @ A, A.T @ b)
    except np.linalg.LinAlgError:
        return None
    return np.append(hvec, 1.0).reshape(3, 3)


def _apply_h(H, p):
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ H.T
    return q[:, :2] / q[:, 2:3]


def _normalised(p):
    """points moved to their mean and divided by their mean distance from it (so that the normal equations are well scaled)"""
    c = p.mean(0)
    s = np.sqrt(((p - c) ** 2).sum(1)).mean()
    return (p - c) / (s if s > 0 else 1.0)


def extreme_quad(pi):
    """pi: integer points [n, 2] -> indices of the four extreme points of the frame whose quadrilateral is largest, in the cyclic order
    max a, max b, min a, min b; ties: the first frame, the first point. Integer arithmetic throughout."""
    best, best_area = None, -1
    x, y = pi[:, 0].astype(np.int64), pi[:, 1].astype(np.int64)
    for a, b in FRAMES:
        pa, pb = a * x + b * y, -b * x + a * y
        q = [int(np.argmax(pa)), int(np.argmax(pb)), int(np.argmin(pa)), int(np.argmin(pb))]
        area2 = sum(int(x[q[i]]) * int(y[q[(i + 1) % 4]]) - int(x[q[(i + 1) % 4]]) * int(y[q[i]]) for i in range(4))
        if abs(area2) > best_area:
            best, best_area = q, abs(area2)
    return best, best_area


def order_board(points, nx, ny):
    """points: [nx * ny, 2] (x, y) -> (found, ordered [nx * ny, 2] float64 | None). nx != ny."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = nx * ny
    assert nx != ny and nx >= 2 and ny >= 2 and len(p) == n
    q, area2 = extreme_quad(np.rint(p).astype(np.int64))
    if area2 <= 0 or len(set(q)) != 4:
        return False, None
    pn = _normalised(p)
    quad = pn[q]
    signed = sum(quad[i, 0] * quad[(i + 1) % 4, 1] - quad[(i + 1) % 4, 0] * quad[i, 1] for i in range(4))
    if signed < 0:                      # the grid's corners below run with positive signed area (x right, y down): (c) right-handed
        quad = quad[::-1]
    grid = np.array([[0, 0], [nx - 1, 0], [nx - 1, ny - 1], [0, ny - 1]], np.float64)
    found = []
    for s in range(4):
        H = _fit_h(np.roll(quad, -s, axis=0), grid)
        if H is None:
            continue
        node = np.floor(_apply_h(H, pn) + 0.5)
        if (node[:, 0] < 0).any() or (node[:, 0] > nx - 1).any() or (node[:, 1] < 0).any() or (node[:, 1] > ny - 1).any():
            continue
        idx = (node[:, 1] * nx + node[:, 0]).astype(np.int64)
        if len(np.unique(idx)) != n:    # (a) one to one
            continue
        Hall = _fit_h(pn, node)
        if Hall is None:
            continue
        if not (np.abs(_apply_h(Hall, pn) - node).max(1) <= CELL_TOL).all():   # (b) within a quarter cell, each axis
            continue
        out = np.zeros((n, 2))
        out[idx] = p
        # (c): the first cell's sides turn the way the grid's do
        e1, e2 = out[1] - out[0], out[nx] - out[0]
        if e1[0] * e2[1] - e1[1] * e2[0] <= 0:
            continue
        found.append(out)
    if not found:
        return False, None
    found.sort(key=lambda o: (o[0, 1], o[0, 0]))   # of the two half turns, the first point smaller in (y, x)
    return True, found[0]


# ---- cornerSubPix -------------------------------------------------------------------------------------------------------------------
# exp(-(i / 5)^2), i = -5 .. 5, as numbers (the header holds the same digits)
MASK11 = (0.36787944117144233, 0.52729242404304855, 0.69767632607103103, 0.85214378896621135, 0.96078943915232320, 1.0,
          0.96078943915232320, 0.85214378896621135, 0.69767632607103103, 0.52729242404304855, 0.36787944117144233)
SUBPIX_DET_MIN = np.finfo(np.float64).eps ** 2


def subpix_window_ok(w, h, x, y, win=5):
    """whether the (2 win + 3)^2 patch of bilinear samples around (x, y) reads only pixels of the image"""
    x0, y0 = x - (win + 1), y - (win + 1)
    return bool(np.floor(x0) >= 0 and np.floor(y0) >= 0 and np.floor(x0) + 2 * win + 3 <= w - 1 and np.floor(y0) + 2 * win + 3 <= h - 1)


def _patch(img, cx, cy, win):
    n = 2 * win + 3
    x0, y0 = cx - (win + 1), cy - (win + 1)
    ix, iy = int(np.floor(x0)), int(np.floor(y0))
    a, b = x0 - ix, y0 - iy
    p = img[iy:iy + n + 1, ix:ix + n + 1].astype(np.float64)
    return (p[:-1, :-1] * ((1 - a) * (1 - b)) + p[:-1, 1:] * (a * (1 - b))) + (p[1:, :-1] * ((1 - a) * b) + p[1:, 1:] * (a * b))


def corner_subpix(img, corners, win=5, max_iter=30, eps=0.1, reverse_sums=False, detail=False):
    """-> refined [n, 2] float64 (and with detail: the last squared shift and a status per corner: 0 refined, 1 start kept because the
    result moved more than win, 2 start kept because the window left the image, 3 stopped on a singular system).
    reverse_sums adds the window's terms in the opposite order: the same numbers up to rounding (how the tests size their tolerance)."""
    assert win == 5, "the committed mask is the 11-tap one"
    h, w = img.shape
    m1 = np.array(MASK11)
    mask = m1[:, None] * m1[None, :]
    py, px = np.mgrid[-win:win + 1, -win:win + 1].astype(np.float64)
    out = np.array(corners, dtype=np.float64).reshape(-1, 2).copy()
    last, status = np.zeros(len(out)), np.zeros(len(out), np.int32)
    tot = (lambda a: np.ascontiguousarray(a.ravel()[::-1]).sum()) if reverse_sums else (lambda a: a.sum())
    for k, (sx, sy) in enumerate(out.copy()):
        cx, cy, it, err = sx, sy, 0, 0.0
        while True:
            if not subpix_window_ok(w, h, cx, cy, win):
                status[k] = 2
                break
            p = _patch(img, cx, cy, win)
            gx = p[1:-1, 2:] - p[1:-1, :-2]
            gy = p[2:, 1:-1] - p[:-2, 1:-1]
            gxx, gxy, gyy = gx * gx * mask, gx * gy * mask, gy * gy * mask
            a, b, c = tot(gxx), tot(gxy), tot(gyy)
            bb1, bb2 = tot(gxx * px + gxy * py), tot(gxy * px + gyy * py)
            det = a * c - b * b
            if abs(det) <= SUBPIX_DET_MIN:
                status[k] = 3
                break
            scale = 1.0 / det
            nx_, ny_ = cx + c * scale * bb1 - b * scale * bb2, cy - b * scale * bb1 + a * scale * bb2
            err = (nx_ - cx) ** 2 + (ny_ - cy) ** 2
            cx, cy = nx_, ny_
            it += 1
            if not (it < max_iter and err > eps * eps):
                break
        last[k] = err
        if status[k] == 2:
            cx, cy = sx, sy
        elif abs(cx - sx) > win or abs(cy - sy) > win:
            cx, cy, status[k] = sx, sy, 1
        out[k] = cx, cy
    return (out, last, status) if detail else out


# ---- calibrateCamera ------------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    th = np.sqrt(r @ r)
    if th < 1e-12:
        return np.eye(3) + np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rodrigues_inv(R):
    """rotation matrix -> rotation vector by way of the unit quaternion with the largest component taken first, so that angles near pi
    (a board whose object frame is (row, column) is seen turned by about pi) lose nothing"""
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]]
    k = int(np.argmax(t))
    s = 2 * np.sqrt(1 + t[k])
    if k == 0:
        q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4]
    q = np.array(q) if q[0] >= 0 else -np.array(q)
    n = np.sqrt(q[1:] @ q[1:])
    if n < 1e-300:
        return np.zeros(3)
    return q[1:] * (2 * np.arctan2(n, q[0]) / n)


def project(obj, rvec, tvec, intr, dist):
    fx, fy, cx, cy = intr
    k1, k2, p1, p2, k3 = dist
    P = obj @ rodrigues(rvec).T + tvec
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r2 = x * x + y * y
    cd = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], 1)


def _dlt_h(src, dst):
    """plane -> image homography on normalised coordinates of both sides"""
    def norm(p):
        c = p.mean(0)
        s = np.sqrt(((p - c) ** 2).sum(1)).mean()
        s = s if s > 0 else 1.0
        return (p - c) / s, np.array([[1 / s, 0, -c[0] / s], [0, 1 / s, -c[1] / s], [0, 0, 1]])
    a, Ta = norm(src)
    b, Tb = norm(dst)
    H = np.linalg.inv(Tb) @ _fit_h(a, b) @ Ta
    return H / H[2, 2]


def initial_intrinsics(Hs, size):
    """OpenCV's initIntrinsicParams2D idea: the principal point at the image's centre, fx and fy from the orthogonality of each view's
    vanishing directions, least squares."""
    cx, cy = (size[0] - 1) * 0.5, (size[1] - 1) * 0.5
    A, b = [], []
    for H in Hs:
        H = H.copy()
        H[0] -= H[2] * cx
        H[1] -= H[2] * cy
        hh, v = H[:, 0].copy(), H[:, 1].copy()
        d1, d2 = (hh + v) * 0.5, (hh - v) * 0.5
        hh, v, d1, d2 = (t / np.sqrt(t @ t) for t in (hh, v, d1, d2))
        A += [[hh[0] * v[0], hh[1] * v[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
        b += [-hh[2] * v[2], -d1[2] * d2[2]]
    A, b = np.array(A), np.array(b)
    f = np.linalg.solve(A.T @ A, A.T @ b)
    return np.array([np.sqrt(abs(1 / f[0])), np.sqrt(abs(1 / f[1])), cx, cy])


def pose_from_h(H, intr):
    fx, fy, cx, cy = intr
    Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])
    M = Kinv @ H
    lam = 1 / np.sqrt(M[:, 0] @ M[:, 0])
    if M[2, 2] * lam < 0:
        lam = -lam
    r1, r2, t = M[:, 0] * lam, M[:, 1] * lam, M[:, 2] * lam
    r2 = r2 - (r1 @ r2) * r1
    r2 = r2 / np.sqrt(r2 @ r2)
    R = np.stack([r1, r2, np.cross(r1, r2)], 1)
    return rodrigues_inv(R), t


LM_ITERS = 30
LM_STEP = 1e-6


def calibrate_camera(object_points, image_points, image_size):
    """object_points, image_points: per view [m, 3] and [m, 2]; image_size (w, h) -> dict K [3, 3], dist [5] (k1, k2, p1, p2, k3),
    rvecs, tvecs [n, 3], rms. Levenberg-Marquardt over 9 + 6 n parameters (fx, fy, cx, cy, k1, k2, p1, p2, k3, then rvec and tvec per
    view) with central-difference derivatives (step LM_STEP * max(1, |p|)), the damping J'J + lambda diag(J'J), lambda from 1e-3,
    divided by 10 after a step that lowers the error and multiplied by 10 after one that does not; LM_ITERS steps at most, or until an
    accepted step changes the parameter vector by less than DBL_EPSILON of its length."""
    obj = [np.asarray(o, dtype=np.float64).reshape(-1, 3) for o in object_points]
    img = [np.asarray(i, dtype=np.float64).reshape(-1, 2) for i in image_points]
    nv = len(obj)
    assert nv >= 1 and len(img) == nv and all(len(o) == len(i) >= 4 for o, i in zip(obj, img))
    Hs = [_dlt_h(o[:, :2], i) for o, i in zip(obj, img)]
    intr = initial_intrinsics(Hs, image_size)
    p = np.zeros(9 + 6 * nv)
    p[:4] = intr
    for v, H in enumerate(Hs):
        r, t = pose_from_h(H, intr)
        p[9 + 6 * v:12 + 6 * v], p[12 + 6 * v:15 + 6 * v] = r, t

    def residuals(q):
        return np.concatenate([(project(obj[v], q[9 + 6 * v:12 + 6 * v], q[12 + 6 * v:15 + 6 * v], q[:4], q[4:9]) - img[v]).ravel()
                               for v in range(nv)])

    def jacobian(q):
        J = np.zeros((sum(2 * len(o) for o in obj), len(q)))
        for j in range(len(q)):
            h = LM_STEP * max(1.0, abs(q[j]))
            qa, qb = q.copy(), q.copy()
            qa[j] += h
            qb[j] -= h
            J[:, j] = (residuals(qa) - residuals(qb)) / (2 * h)
        return J

    lam, r = 1e-3, residuals(p)
    err = r @ r
    J = jacobian(p)
    for _ in range(LM_ITERS):
        JtJ, g = J.T @ J, J.T @ r
        try:
            step = np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), -g)
        except np.linalg.LinAlgError:
            lam *= 10
            continue
        r2 = residuals(p + step)
        e2 = r2 @ r2
        if np.isfinite(e2) and e2 < err:
            small = np.sqrt(step @ step) < np.finfo(np.float64).eps * np.sqrt(p @ p)
            p, r, err, lam = p + step, r2, e2, max(lam / 10, 1e-16)
            if small:
                break
            J = jacobian(p)
        else:
            lam *= 10
    total = sum(len(o) for o in obj)
    K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1]])
    return {"K": K, "dist": p[4:9].copy(), "rvecs": p[9:].reshape(nv, 6)[:, :3].copy(), "tvecs": p[9:].reshape(nv, 6)[:, 3:].copy(),
            "rms": float(np.sqrt(err / total))}


def object_points(nx, ny):
    """the reference's (CalibrationUtil.cpp:13-17): point i * nx + j is (i, j, 0)"""
    i, j = np.mgrid[0:ny, 0:nx]
    return np.stack([i.ravel(), j.ravel(), np.zeros(nx * ny)], 1).astype(np.float64)


def find_chessboard_corners(img, nx, ny, max_candidates=256):
    c = candidates(img, max_candidates)
    if len(c) < nx * ny:
        return False, None
    return order_board(np.stack([c["x"][:nx * ny], c["y"][:nx * ny]], 1), nx, ny)
