"""Constructed images that reach the ends of the value range of the keypoint source's kernels (detect_kernels.hip, grad_desc_kernels.hip,
dog_kernels.hip): FAST score 255 and ties at it, the gradient descriptor's largest and smallest accumulators, flat
patches, all 32 direction bins, and the strongest blobs the DoG rule can see. Plain numpy; tests/test_value_limit_cases.py states from
the CPU statements what each image reaches, tests/test_gpu_value_limits.py runs the kernels on them.

    mosaic()                 198 x 264: 48 patches of 33 x 33, six per row; MOSAIC_CENTRES are the patch centres, whose 16-pixel reach
                             stays inside their own patch
    dots(w, h, fg, bg)       isolated pixels of fg on bg, 7 apart: every one a FAST corner of score |fg - bg|
    dots_batch(w, h)         the four dots images of one size: bright on black, dark on white, and both again upside down
    discs()                  130 x 97: filled discs of radius 2, 3, 4, 6, bright on 0 and dark on 255
    own_contrasts(name)      the |D_1| of the weakest and of the strongest level-0 DoG candidate of mosaic() or discs(): the contrasts
                             at which the strict |c| > contrast is decided at equality
"""
import functools

import numpy as np

PATCH = 33
PER_ROW = 6
N_PATCHES = 48
MOSAIC_W, MOSAIC_H = PATCH * PER_ROW, PATCH * (N_PATCHES // PER_ROW)
MOSAIC_CENTRES = [(16 + PATCH * (i % PER_ROW), 16 + PATCH * (i // PER_ROW)) for i in range(N_PATCHES)]      # (x, y)
HALF_PLANES = range(0, 32)        # patch indices by kind
FAR_EDGES = range(32, 36)
FLAT = 36
SMALLEST_STEP = 37
CHECKERBOARDS = range(38, 41)     # periods 1, 2, 3
BRIGHT_PIXEL, DARK_PIXEL = 41, 42
NOISE = range(43, 48)
DOTS_SIZES = [(97, 65), (130, 200)]                                                                         # (width, height)
DISC_RADII = (2, 3, 4, 6)
DISC_CENTRES = [(24.25 + 26 * i, y) for y in (24.25, 71.25) for i in range(4)]                               # (x, y): bright row, dark row


def patches():
    """The 48 patches, uint8 [48, 33, 33]."""
    yy, xx = np.mgrid[0:PATCH, 0:PATCH]
    out = []
    for k in range(32):                                                    # half-planes through the centre, one per direction bin
        a = np.deg2rad(11.25 * k)
        out.append(np.where((xx - 16) * np.cos(a) + (yy - 16) * np.sin(a) > 0.25, 255, 0))
    far = np.zeros((PATCH, PATCH), dtype=np.int64)
    far[:, 28:] = 255                                                      # an edge far from the centre: few cells see a gradient
    out += [np.rot90(far, r) for r in range(4)]
    out.append(np.full((PATCH, PATCH), 77))
    step = np.full((PATCH, PATCH), 100)
    step[:, 17:] = 101                                                     # the smallest gradients
    out.append(step)
    out += [((xx // p + yy // p) & 1) * 255 for p in (1, 2, 3)]
    for fg, bg in ((255, 0), (0, 255)):
        one = np.full((PATCH, PATCH), bg)
        one[16, 16] = fg
        out.append(one)
    out += [np.random.default_rng(i).integers(0, 256, (PATCH, PATCH), dtype=np.uint8) for i in range(43, 48)]
    assert len(out) == N_PATCHES
    return np.stack([np.asarray(p).astype(np.uint8) for p in out])


@functools.lru_cache(maxsize=None)
def _mosaic():
    p = patches().reshape(N_PATCHES // PER_ROW, PER_ROW, PATCH, PATCH)
    return np.ascontiguousarray(p.transpose(0, 2, 1, 3).reshape(MOSAIC_H, MOSAIC_W))


def mosaic():
    """uint8 [264, 198], the caller's own copy: patch i at rows 33 (i // 6), columns 33 (i % 6)."""
    return _mosaic().copy()


def mosaic_batch():
    """[mosaic, mosaic upside down, 255 - mosaic]."""
    m = mosaic()
    return np.stack([m, m[::-1], 255 - m])


REFUSED = [(15, 16), (182, 247), (16.5, 16), (16, 248)]          # (x, y) on the mosaic: left of, right of, between and below the legal pixels


def centre_records(dtype):
    """The 48 patch centres as keypoint records of `dtype` (fields x, y, angle at least), angle -1."""
    kp = np.zeros(N_PATCHES, dtype=dtype)
    kp["x"], kp["y"] = [c[0] for c in MOSAIC_CENTRES], [c[1] for c in MOSAIC_CENTRES]
    kp["angle"] = -1.0
    return kp


def mixed_records(dtype):
    """(records, refused mask): the centres three at a time with one record of REFUSED among them, at position g % 4 of group g, so
    that over the 16 groups of four -- the four waves of a describe workgroup -- every position is refused four times beside three
    active ones and every kind of refusal meets every position; then a group of two, refused and active: 66 records, no multiple of 4."""
    centres = centre_records(dtype)
    out, refused = [], []
    for g in range(N_PATCHES // 3):
        group = list(centres[3 * g:3 * g + 3])
        bad = centres[0].copy()
        bad["x"], bad["y"] = REFUSED[(g + g // 4) % 4]
        group.insert(g % 4, bad)
        out += group
        refused += [j == g % 4 for j in range(4)]
    bad = centres[0].copy()
    bad["x"], bad["y"] = REFUSED[2]
    out += [bad, centres[N_PATCHES - 1]]
    refused += [True, False]
    return np.array(out, dtype=dtype), np.array(refused)


def dots(w, h, fg, bg):
    img = np.full((h, w), bg, dtype=np.uint8)
    img[18:h - 16:7, 18:w - 16:7] = fg
    return img


def dots_batch(w, h):
    a, b = dots(w, h, 255, 0), dots(w, h, 0, 255)
    return np.stack([a, b, a[::-1], b[:, ::-1]])


def discs():
    """uint8 [97, 130]: rows < 48 are 0 with discs of 255, rows >= 48 are 255 with discs of 0; the radii 2, 3, 4, 6 from left to right.
    Every centre is at least 24 pixels from the edges and from the other centres, and 23 from the row where the ground changes (the
    largest disc and the widest blur reach 6.25 + 8). A disc centred on a pixel ties its neighbours or is no extremum over the three
    layers at any of these radii, so the centres lie a quarter pixel off the grid in x and y, and a pixel belongs to a disc when its
    centre is within r + 1/4 of the disc's: radius 2 is then the 15 pixels whose |D_1| peaks on layer 1 of level 0, a quarter pixel
    from where the integer extremum is; the larger ones peak on higher levels of the pyramid."""
    h, w = 97, 130
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.where(yy < 48, 0, 255)
    for i, (cx, cy) in enumerate(DISC_CENTRES):
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= (DISC_RADII[i % 4] + 0.25) ** 2] = 255 if cy < 48 else 0
    return img.astype(np.uint8)


def discs_batch():
    d = discs()
    return np.stack([d, 255 - d])


@functools.lru_cache(maxsize=None)
def own_contrasts(name):
    """{"weakest": (c*, x, y), "strongest": (c*, x, y)} of "mosaic" or "discs": c* = |D_1| of the level-0 candidate (tests/dog_ref.py,
    contrast 0) with the smallest and with the largest |D_1|, the first in raster order among equal ones. The rule is |c| > contrast,
    so the candidate is there at contrast c* - 1 and gone at c*."""
    import dog_ref
    img = {"mosaic": mosaic, "discs": discs}[name]()
    ys, xs = np.nonzero(dog_ref.candidates(img, 0))
    a = np.abs(dog_ref.layers(img)[1][ys, xs].astype(np.int64))
    return {key: (int(a[i]), int(xs[i]), int(ys[i])) for key, i in (("weakest", int(np.argmin(a))), ("strongest", int(np.argmax(a))))}


def contrast_set(*names):
    """0, 65535 and c*, c* - 1 of both chosen candidates of every named image, ascending."""
    out = {0, 65535}
    for name in names:
        for c, _, _ in own_contrasts(name).values():
            out |= {c, c - 1}
    return sorted(out)
