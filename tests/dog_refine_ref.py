"""A numpy statement of the DoG detector's refinement (gms_detect_dog_refined_batch_device / gms_dog_offsets_device, include/gms.h,
DESIGN.md §4.7d): a candidate of tests/dog_ref.py moved to 1/16 pixel and 1/16 layer by one integer Newton step. The header
sfm-gms_amd/csrc/dog_core.h states the same for the kernel and for the host build, and the three are compared byte for byte.

    K_SCALE                                 float32(1.2^((i - 8) / 16)), i = 0 .. 16, written out; scale_rule(i) is what the numbers are
    terms(img, contrast)                    the integer quantities of the rule at every candidate (xs, ys, nx, ny, det16, n, q)
    floor_sixteenths(n, q)                  floor((32 n + q) / (2 q)): round(16 n / q), halves up
    offsets_at(img, contrast)               (xs, ys, ox, oy, os) of the candidates in raster order, ox and oy clamped to [-8, 8]
    offsets(img, contrast)                  uint16 plane: 1 + (ox + 8) + 17 (oy + 8) + 289 (os + 8) at a candidate, else 0
    unpack(code)                            (ox, oy, os) of codes
    detect(oracle, img, ..., refine=True)   dog_ref.detect with x, y and size of every record refined; nothing else changes
    sfm_chain(oracle, left, right, camera, ..., refine=True)   dog_ref.sfm_chain behind this detector

At a candidate (x, y) of a level image, D = D_1, c = D(x, y), with the candidate rule's dxx, dyy, dxy4, det16 > 0:
    gx2 = D(x+1, y) - D(x-1, y), gy2 = D(x, y+1) - D(x, y-1)
    nx = -(8 dyy gx2 - 2 dxy4 gy2), ny = -(8 dxx gy2 - 2 dxy4 gx2)          -H^-1 g, scaled so that nx / det16 is the offset in pixels
    ox = clamp(floor((32 nx + det16) / (2 det16)), -8, 8), oy likewise       1/16 pixel, rounded half up; int64, |numerator| < 2^45
    a = D_2(x, y) - D_0(x, y), b = D_0(x, y) + D_2(x, y) - 2c                b != 0, |a| < |b|: c is a strict extremum over both
    n = a if b < 0 else -a, q = 2 |b|, os = floor((32 n + q) / (2 q))        1/16 layer; |os| <= 8 follows, asserted here
The divisions are FLOOR divisions (numpy's // on int64). SIFT re-centres and refits beyond half a pixel; this rule clamps.
The record, every operation rounded once in fp32: px = x + ox * 0.0625 (exact), X = (px + 0.5) * fx - 0.5, Y likewise,
size = (31 * fx) * K_SCALE[os + 8]. Direction, response, octave, class_id and both rows are those of the integer (x, y).
"""
import numpy as np

import dog_ref
import grad_desc_ref  # noqa: F401  (the rows of dog_ref.detect_level)
import pyramid_ref

OFFSET_MAX = 8
STEPS = 2 * OFFSET_MAX + 1
K_SCALE = np.array([0.91287094, 0.9233327, 0.9339143, 0.9446172, 0.9554428, 0.9663924, 0.97746754, 0.9886696, 1.0,
                    1.0114603, 1.0230519, 1.0347763, 1.0466352, 1.0586299, 1.070762, 1.0830332, 1.0954452], dtype=np.float32)


def scale_rule(i):
    return np.float32(1.2 ** ((i - OFFSET_MAX) / 16.0))


def floor_sixteenths(n, q):
    return (32 * n + q) // (2 * q)


def terms(img, contrast=128, cand=None):
    """The rule's integers at the candidates of an image, raster order: dict of int64 arrays xs, ys, nx, ny, det16, n, q."""
    cand = dog_ref.candidates(img, contrast) if cand is None else cand
    ys, xs = np.nonzero(cand)
    if len(xs) == 0:
        z = np.zeros(0, dtype=np.int64)
        return dict(xs=z, ys=z, nx=z, ny=z, det16=z, n=z, q=z)
    D = [d.astype(np.int64) for d in dog_ref.layers(img)]

    def at(k, dx, dy):
        return D[k][ys + dy, xs + dx]

    c = at(1, 0, 0)
    dxx = at(1, 1, 0) + at(1, -1, 0) - 2 * c
    dyy = at(1, 0, 1) + at(1, 0, -1) - 2 * c
    dxy4 = at(1, 1, 1) - at(1, -1, 1) - at(1, 1, -1) + at(1, -1, -1)
    det16 = 16 * dxx * dyy - dxy4 * dxy4
    assert (det16 > 0).all()
    gx2, gy2 = at(1, 1, 0) - at(1, -1, 0), at(1, 0, 1) - at(1, 0, -1)
    nx = -(8 * dyy * gx2 - 2 * dxy4 * gy2)
    ny = -(8 * dxx * gy2 - 2 * dxy4 * gx2)
    a, b = at(2, 0, 0) - at(0, 0, 0), at(0, 0, 0) + at(2, 0, 0) - 2 * c
    assert (b != 0).all()
    n, q = np.where(b < 0, a, -a), 2 * np.abs(b)
    assert max(np.abs(32 * nx + det16).max(), np.abs(32 * ny + det16).max()) < 1 << 45
    return dict(xs=xs.astype(np.int64), ys=ys.astype(np.int64), nx=nx, ny=ny, det16=det16, n=n, q=q)


def offsets_at(img, contrast=128, cand=None):
    """(xs, ys, ox, oy, os) of the candidates, raster order; int64."""
    t = terms(img, contrast, cand)
    ox = np.clip(floor_sixteenths(t["nx"], t["det16"]), -OFFSET_MAX, OFFSET_MAX)
    oy = np.clip(floor_sixteenths(t["ny"], t["det16"]), -OFFSET_MAX, OFFSET_MAX)
    os_ = floor_sixteenths(t["n"], t["q"])
    assert (np.abs(os_) <= OFFSET_MAX).all()                     # no clamp: the strict extremum gives it
    return t["xs"], t["ys"], ox, oy, os_


def pack(ox, oy, os_):
    return 1 + (ox + OFFSET_MAX) + STEPS * (oy + OFFSET_MAX) + STEPS * STEPS * (os_ + OFFSET_MAX)


def unpack(code):
    v = np.asarray(code).astype(np.int64) - 1
    return v % STEPS - OFFSET_MAX, v // STEPS % STEPS - OFFSET_MAX, v // (STEPS * STEPS) - OFFSET_MAX


def offsets(img, contrast=128, cand=None):
    """The code plane of an image: uint16 [h, w], 0 where there is no candidate."""
    h, w = np.shape(img)
    plane = np.zeros((h, w), dtype=np.uint16)
    xs, ys, ox, oy, os_ = offsets_at(img, contrast, cand)
    plane[ys, xs] = pack(ox, oy, os_)
    return plane


def level_offsets(img, contrast=128, n_levels=8, planes=None):
    """The code planes of the pyramid's levels; planes: dog_ref.level_candidates(img, contrast, at least n_levels), where the caller has them."""
    return [offsets(level, contrast, None if planes is None else planes[l]) for l, level in enumerate(pyramid_ref.build(img, n_levels))]


def detect(oracle, img, contrast=128, max_keypoints=10000, n_levels=8, planes=None, refine=True, codes=None):
    """dog_ref.detect's tuple (keypoints, [n, 32] rows, counts per level, [n, 128] rows); with refine, x, y and size of every record are
    the refined ones. planes / codes: the levels' candidate and code planes, where the caller has them already."""
    if not refine:
        return dog_ref.detect(oracle, img, contrast, max_keypoints, n_levels, planes)
    h, w = img.shape
    levels = pyramid_ref.build(img, n_levels)
    sizes = [(l.shape[1], l.shape[0]) for l in levels]
    kps, rows32, rows128, counts = [], [], [], np.zeros(n_levels, dtype=np.int32)
    half, step = np.float32(0.5), np.float32(0.0625)
    for l, (level, q) in enumerate(zip(levels, pyramid_ref.quotas(sizes, max_keypoints))):
        cand = dog_ref.candidates(level, contrast) if planes is None else planes[l]
        kp, r32, r128 = dog_ref.detect_level(oracle, level, contrast, q, cand)            # selection, quota and order: unchanged
        code = (offsets(level, contrast, cand) if codes is None else codes[l])[kp["y"].astype(np.int64), kp["x"].astype(np.int64)]
        assert (code > 0).all()
        ox, oy, os_ = unpack(code)
        fx, fy = np.float32(w) / np.float32(sizes[l][0]), np.float32(h) / np.float32(sizes[l][1])
        px = kp["x"].astype(np.float32) + ox.astype(np.float32) * step                   # exact
        py = kp["y"].astype(np.float32) + oy.astype(np.float32) * step
        kp["x"] = (px + half) * fx - half                                                # each operation rounds once, in fp32
        kp["y"] = (py + half) * fy - half
        kp["size"] = (np.float32(31.0) * fx) * K_SCALE[os_ + OFFSET_MAX]
        kp["octave"] = l
        kps.append(kp); rows32.append(r32); rows128.append(r128)
        counts[l] = len(kp)
    return np.concatenate(kps), np.concatenate(rows32).reshape(-1, 32), counts, np.concatenate(rows128).reshape(-1, 128).astype(np.float32)


def sfm_chain(oracle, left, right, camera, contrast=128, max_keypoints=4000, n_levels=8, factor=6.0, prob=0.7, ransac_threshold=1.0, refine=True,
              detected=None):
    """dog_ref.sfm_chain with this detector in front. detected: the two detect() tuples, where the caller has them already (the chain
    behind the detector at another RANSAC threshold)."""
    import sfm_ref
    size = (left.shape[1], left.shape[0])
    if detected is None:
        detected = [detect(oracle, img, contrast, max_keypoints, n_levels, refine=refine) for img in (left, right)]
    (kp1, r32_1, _, rows1), (kp2, r32_2, _, rows2) = detected
    matches = oracle.bf_match(rows1, rows2, False)
    rc, out, _, res = oracle.match(size, size, kp1, kp2, matches, True, True, factor)
    assert rc == 0
    _, w1, w2 = oracle.gather(kp1, kp2, out)
    tv = sfm_ref.two_view(w1, w2, camera, None, prob, ransac_threshold)
    return dict(keypoints=(kp1, kp2), rows32=(r32_1, r32_2), rows128=(rows1, rows2), matches=matches, survivors=out, result=res, two_view=tv)
