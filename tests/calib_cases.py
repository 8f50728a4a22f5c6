"""Inputs of the calibration tests, one per rule of DESIGN.md §4.12: synthetic chessboards rendered analytically through a pinhole camera
with lens distortion (4 x 4 samples per pixel), whose true corners are known, and block images for the tie rules. case(name) returns
a Case; census(case) counts, with the statement's own pieces (tests/calib_ref.py), what the case is named for:
tests/test_calib_ref.py asserts from it that every case contains its rule, on the CPU, and tests/test_gpu_calib.py holds the GPU to the
statement on the same inputs.

  rot0, rot90, rot180, rot270   the board turned about the optical axis
  perspective                   seen at 50 degrees from its normal
  edges                         the board on white paper: the half-saddles of its rim are present, and weaker than every inner corner
  covered                       one inner corner under a grey disc: must give "not found"
  flipped                       rot0 mirrored left to right: the order found must be right-handed in the image, never the mirrored one
  ties                          a block image of two grey levels in which every peak has the same R on a 2 x 2 plateau
  const                         a constant image: no candidates"""
import functools
import os
from types import SimpleNamespace

import numpy as np

import calib_ref as R

NX, NY = 6, 9
INTR = (520.0, 515.0, 171.5, 213.5)
DIST = (-0.12, 0.03, 0.001, -0.0005, 0.0)
SIZE = (344, 428)            # width, height
LEVELS = (30, 225, 128)      # dark, light (squares and paper), background
SS = 4


def _undistort(xd, yd, dist, iters=12):
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        ic = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        x, y = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) * ic, (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) * ic
    return x, y


def board_points(nx=NX, ny=NY):
    """the inner corners in the renderer's board frame: (column, row, 0), row by row"""
    i, j = np.mgrid[0:ny, 0:nx]
    return np.stack([j.ravel(), i.ravel(), np.zeros(nx * ny)], 1).astype(np.float64)


def render(rvec, tvec, size=SIZE, intr=INTR, dist=DIST, nx=NX, ny=NY, paper=0.6, cover=None):
    """-> (uint8 [h, w], true corners [nx * ny, 2]). The board's squares fill [-1, nx] x [-1, ny] of its plane, dark where
    floor(X) + floor(Y) is odd; white paper for `paper` of a square around it; background beyond. cover = (X, Y, radius): a
    background-grey disc on the board."""
    w, h = size
    fx, fy, cx, cy = intr
    o = (np.arange(SS) + 0.5) / SS - 0.5
    xs = (np.arange(w)[:, None] + o[None, :]).ravel()
    ys = (np.arange(h)[:, None] + o[None, :]).ravel()
    X, Y = np.meshgrid((xs - cx) / fx, (ys - cy) / fy)
    x, y = _undistort(X, Y, dist)
    Rm = R.rodrigues(np.asarray(rvec, dtype=np.float64))
    Hinv = np.linalg.inv(np.stack([Rm[:, 0], Rm[:, 1], np.asarray(tvec, dtype=np.float64)], 1))
    q = Hinv @ np.stack([x.ravel(), y.ravel(), np.ones(x.size)])
    bx, by = (q[0] / q[2]).reshape(x.shape), (q[1] / q[2]).reshape(x.shape)
    dark, light, back = LEVELS
    on_board = (bx >= -1) & (bx <= nx) & (by >= -1) & (by <= ny)
    on_paper = (bx >= -1 - paper) & (bx <= nx + paper) & (by >= -1 - paper) & (by <= ny + paper)
    odd = ((np.floor(bx) + np.floor(by)).astype(np.int64) & 1) == 1
    v = np.where(on_board, np.where(odd, dark, light), np.where(on_paper, light, back)).astype(np.float64)
    if cover is not None:
        v = np.where((bx - cover[0]) ** 2 + (by - cover[1]) ** 2 <= cover[2] ** 2, back, v)
    img = np.floor(v.reshape(h, SS, w, SS).mean((1, 3)) + 0.5).astype(np.uint8)
    return img, R.project(board_points(nx, ny), np.asarray(rvec, float), np.asarray(tvec, float), intr, dist)


def _pose(roll_deg, tilt=(0.0, 0.0), z=19.0):
    """the board's centre on the optical axis at depth z; tilt (about x, about y) first, then the roll about the axis"""
    a = np.deg2rad(roll_deg)
    Rz = R.rodrigues(np.array([0, 0, a]))
    Rt = R.rodrigues(np.array([tilt[0], 0, 0])) @ R.rodrigues(np.array([0, tilt[1], 0]))
    Rm = Rz @ Rt
    c = np.array([(NX - 1) / 2, (NY - 1) / 2, 0.0])
    return R.rodrigues_inv(Rm), np.array([0, 0, z]) - Rm @ c


def _ties():
    """blocks of 20 pixels in two grey levels: every crossing lies between four pixels, so R is equal on those four (a plateau), and
    equal from crossing to crossing"""
    h, w, b = 150, 190, 20
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x + 5) // b + (y + 5) // b) & 1, 200, 60).astype(np.uint8)


NAMES = ("rot0", "rot90", "rot180", "rot270", "perspective", "edges", "covered", "flipped", "ties", "const")
BOARDS = ("rot0", "rot90", "rot180", "rot270", "perspective", "edges", "flipped")   # cases whose board must be found


@functools.lru_cache(maxsize=None)
def case(name):
    """-> Case(image, true: [54, 2] true corners in the board's own order or None, found: whether the board must be found)"""
    if name in ("rot0", "rot90", "rot180", "rot270"):
        roll = int(name[3:])
        size = SIZE if roll in (0, 180) else SIZE[::-1]
        intr = INTR if roll in (0, 180) else (INTR[0], INTR[1], INTR[3], INTR[2])
        img, true = render(*_pose(roll, (0.15, -0.1)), size=size, intr=intr)
        return SimpleNamespace(image=img, true=true, found=True)
    if name == "perspective":
        img, true = render(*_pose(10, (np.deg2rad(50), 0.0), z=21.0))
        return SimpleNamespace(image=img, true=true, found=True)
    if name == "edges":
        img, true = render(*_pose(5, (0.1, 0.1)), paper=1.2)
        return SimpleNamespace(image=img, true=true, found=True)
    if name == "covered":
        img, true = render(*_pose(0, (0.15, -0.1)), cover=(2.0, 4.0, 0.55))
        return SimpleNamespace(image=img, true=true, found=False)
    if name == "flipped":
        c = case("rot0")
        img = np.ascontiguousarray(c.image[:, ::-1])
        true = np.stack([img.shape[1] - 1 - c.true[:, 0], c.true[:, 1]], 1)
        return SimpleNamespace(image=img, true=true, found=True)
    if name == "ties":
        return SimpleNamespace(image=_ties(), true=None, found=False)
    if name == "const":
        return SimpleNamespace(image=np.full((70, 90), 77, np.uint8), true=None, found=False)
    raise KeyError(name)


def admissible_orders(c, name):
    """the orders (as [54, 2] true positions) that conditions (a) to (c) admit: row by row, right-handed in the image; the two half
    turns. A mirrored image reverses every row."""
    t = c.true.reshape(NY, NX, 2)
    if name == "flipped":
        t = t[:, ::-1]
    a = t.reshape(-1, 2)
    return [a, a[::-1]]


def expected_order(c, name):
    return min(admissible_orders(c, name), key=lambda o: (round(o[0, 1]), round(o[0, 0])))


@functools.lru_cache(maxsize=None)
def statement(name, max_candidates=256):
    """the statement's response and candidates of a case, computed once"""
    Rm = R.response(case(name).image)
    return Rm, R.candidates_from(Rm, max_candidates)


def census(name):
    """what the case contains, by the statement's own pieces"""
    c = case(name)
    Rm, cand = statement(name)
    pk = R.peaks(Rm)
    out = {"peaks": int(pk.sum()), "distinct_responses": len(np.unique(Rm[pk])) if pk.any() else 0}
    # plateaus: peaks whose later neighbours hold the same R
    ys, xs = np.nonzero(pk)
    out["plateau_peaks"] = int(sum(1 for x, y in zip(xs, ys) if (Rm[y:y + 2, x:x + 2] == Rm[y, x]).sum() > 1))
    if c.true is not None:
        n = NX * NY
        pts = np.stack([cand["x"][:n], cand["y"][:n]], 1).astype(np.float64)
        d = np.sqrt(((pts[:, None, :] - c.true[None, :, :]) ** 2).sum(2))
        out["strongest_are_corners"] = bool(len(cand) >= n and (d.min(1) <= 2.0).all() and len(set(d.argmin(1))) == n)
        out["gap"] = float(cand["response"][n - 1]) / float(cand["response"][n]) if len(cand) > n and cand["response"][n] else float("inf")
        out["weaker_peaks"] = int(len(cand) - n) if len(cand) > n else 0
        e = expected_order(c, name)
        e1, e2 = e[1] - e[0], e[NX] - e[0]
        out["expected_right_handed"] = bool(e1[0] * e2[1] - e1[1] * e2[0] > 0)
    return out


# ---- what the CPU and the GPU tests share -----------------------------------------------------------------------------------------
FACTOR = 100   # a tolerance between two fp64 implementations: FACTOR x what the order of summation alone changes in the statement
N = NX * NY
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def first_points(cand):
    return np.stack([cand["x"][:N], cand["y"][:N]], 1).astype(np.float64)


def calib_vector(r):
    return np.concatenate([[r["K"][0, 0], r["K"][1, 1], r["K"][0, 2], r["K"][1, 2]], r["dist"], r["rvecs"].ravel(), r["tvecs"].ravel(), [r["rms"]]])


def fixture_images():
    return np.concatenate([np.load(os.path.join(GOLDEN, f"image_calib_{t}.npz"))["images"] for t in "abcde"])


def subpix_tolerance(img, start):
    """100 x what the order of summation alone changes. Measured on the cases and photographs: 0 to 1.1e-13 pixels -- the window's sums
    change in their last bits, which reaches a position of some hundreds of pixels only through its own rounding. So the measurement
    cannot show less than one spacing of fp64 at the position, and that spacing is its floor: 100 x max(measured, spacing)."""
    a = R.corner_subpix(img, start)
    b = R.corner_subpix(img, start, reverse_sums=True)
    measured = np.abs(a - b).max()
    assert measured < 1e-9, measured
    return FACTOR * max(measured, np.spacing(np.abs(a).max()))


