"""The named cases of portrait mode's tests (tests/test_portrait_cases.py on the CPU, tests/test_gpu_portrait.py on the GPU; DESIGN.md
§4.9): constructed maps that reach what the seeded sweep of blobs does not -- ties at the cut, more than 1024 borders, 64 chosen
borders, dilations of 5 to 8, chains of tens of thousands of steps, thin and nested shapes, sides of 1 and of 8192. A case is a dict:
name, disparity (uint8 [H, W], read-only), image (uint8 [H, W, 3], read-only), params (the four parameters) and facts: what the
construction guarantees about the statement's answer (tests/portrait_ref.py), as numbers. The mask always comes out of `threshold`
and `dilate_iterations`; none is handed in. facts holds

    borders         the number of borders of the dilated mask (outer and hole)
    chosen          how many of them the statement chooses
    selected        the number of pixels of `selected` that are set
    longest_chain   the number of points of the longest border
    tied            whether the last chosen border and the first one left out have equal area (tests/portrait_ref.cut_is_tied)
    chosen_starts   (optional) the start pixels (x, y) of the chosen borders, in rank order
    areas           (optional) the doubled areas of all borders, descending
    blob            (optional) the rectangle (y0, y1, x0, x1) of the blob whose selection the tie decides

Images are seeded noise with the left half divided by 16 (windows with many equal samples); the median size is 3 unless a case is
about the median, so that the statement stays fast."""
import functools
import zlib

import numpy as np

import portrait_ref as R

FG, THRESHOLD = 200, 60      # a disparity of FG on a background of 0 at THRESHOLD and no dilation gives the mask directly


def _image(name, H, W):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    img = rng.integers(0, 256, (H, W, 3))
    img[:, : W // 2] //= 16
    return img.astype(np.uint8)


def _case(name, disparity, facts, num_contours, threshold=THRESHOLD, dilate_iterations=0, median_ksize=3):
    disparity = np.ascontiguousarray(disparity, dtype=np.uint8)
    disparity.setflags(write=False)
    image = _image(name, *disparity.shape)
    image.setflags(write=False)
    params = dict(threshold=threshold, dilate_iterations=dilate_iterations, num_contours=num_contours, median_ksize=median_ksize)
    return dict(name=name, disparity=disparity, image=image, params=params, facts=dict(facts))


def _from_mask(name, m, facts, num_contours, **kw):
    return _case(name, np.where(m, FG, 0), facts, num_contours, **kw)


# ---- a: everything tied, more keys than one stride of the selection's scan ---------------------------------------------------------------
def dots_lattice(num_contours):
    """70 x 96, a set pixel at every even x of every even y: 35 * 48 = 1680 isolated pixels, every area 0. Only the start pixel
    ranks them: the chosen ones are the first num_contours in raster order."""
    m = np.zeros((70, 96), dtype=bool)
    m[0::2, 0::2] = True
    starts = [(2 * (i % 48), 2 * (i // 48)) for i in range(num_contours)]     # 48 a row
    return _from_mask(f"dots_lattice_{num_contours}", m, dict(borders=1680, chosen=num_contours, selected=num_contours, longest_chain=1,
                                                              tied=True, chosen_starts=starts), num_contours)


# ---- b: ties between outer borders -------------------------------------------------------------------------------------------------------
SQUARE_TOPS = (20, 5, 14, 2, 11, 23, 8, 17, 26)     # the top row of square i, whose left column is 4 + 16 i


def equal_squares_staggered(num_contours):
    """Nine 7 x 7 squares (doubled area 72 each) side by side in a 40 x 150 map with their top rows staggered, so that the raster
    order of their start pixels (their top left corners) is the order of SQUARE_TOPS: neither left to right nor right to left."""
    m = np.zeros((40, 150), dtype=bool)
    for i, top in enumerate(SQUARE_TOPS):
        m[top:top + 7, 4 + 16 * i:11 + 16 * i] = True
    by_top = sorted(range(9), key=lambda i: SQUARE_TOPS[i])
    assert by_top[:5] == [3, 1, 6, 4, 2]
    starts = [(4 + 16 * i, SQUARE_TOPS[i]) for i in by_top[:num_contours]]
    return _from_mask(f"equal_squares_staggered_{num_contours}", m, dict(
        borders=9, chosen=num_contours, selected=49 * num_contours, longest_chain=24, tied=True, chosen_starts=starts,
        areas=[72] * 9), num_contours)


# ---- c: a hole border takes a slot ---------------------------------------------------------------------------------------------------------
def _ring(m, y, x, h, w=None):
    """A one-pixel-thick h x w ring with its top left corner at (y, x)."""
    w = h if w is None else w
    m[y:y + h, x:x + w] = True
    m[y + 1:y + h - 1, x + 1:x + w - 1] = False


def ring_and_blob(blob_first):
    """30 x 60: a 9 x 9 ring one pixel thick (outer border: doubled area 2 * 8 * 8 = 128; hole border: the same square with its
    four corners cut, 124) and a 3 x 32 blob (2 * 2 * 31 = 124), num_contours 2. The ring's outer border is first; the second slot
    goes to whichever of the hole border and the blob starts earlier, and both start on row 6: the hole border at the ring's left
    side, the blob at its own left end. The blob is selected only where it lies left of the ring."""
    m = np.zeros((30, 60), dtype=bool)
    ring_x, blob_x = (40, 3) if blob_first else (3, 16)
    _ring(m, 5, ring_x, 9)
    m[6:9, blob_x:blob_x + 32] = True
    second = (blob_x, 6) if blob_first else (ring_x, 6)
    return _from_mask("blob_then_ring" if blob_first else "ring_then_blob", m, dict(
        borders=3, chosen=2, selected=81 + (96 if blob_first else 0), longest_chain=66, tied=True,
        chosen_starts=[(ring_x, 5), second], areas=[128, 124, 124], blob=(6, 9, blob_x, blob_x + 32)), 2)


# ---- d: 64 chosen of more than 1024 ---------------------------------------------------------------------------------------------------------
NOISE_SEED, NOISE_THRESHOLD = 3, 157     # (254 - 157) / 256 = 38 % of the pixels are above the threshold and have a value


def noise_64():
    """131 x 259 independent noise, 38 % set: more than 1024 borders, 64 of them chosen (bit 63 of the toggle plane and lane 63 of
    the walk are used), and the seed is one at which the 64th and the 65th differ in area. The figures are the statement's."""
    rng = np.random.default_rng(NOISE_SEED)
    d = rng.integers(0, 256, (131, 259))
    return _case("noise_64", d, NOISE_FACTS, 64, threshold=NOISE_THRESHOLD)


NOISE_FACTS = dict(borders=1454, chosen=64, selected=9986, longest_chain=752, tied=False)


# ---- e: long walks, long unions -------------------------------------------------------------------------------------------------------------
def _serpentine_mask(H=131, W=259):
    """The even rows, joined alternately at the right and the left end (speckle_cases.serpentine)."""
    m = np.zeros((H, W), dtype=bool)
    m[0::2, :] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def serpentine():
    """One set component 17159 pixels long and one pixel wide: one outer border that walks it out and back, 2 * (17159 - 1) points
    less one for each of the 130 corners, which the walk cuts diagonally on one of its two ways: 34186. No hole: every zero row
    reaches the frame."""
    m = _serpentine_mask()
    assert int(m.sum()) == 66 * 259 + 65 == 17159
    return _from_mask("serpentine", m, dict(borders=1, chosen=1, selected=17159, longest_chain=34186, tied=False), 5)


def serpentine_inverse():
    """The complement: the zero pixels are one 4-connected snake that touches the frame (no hole border, and a union chain through
    the whole map), and the 65 odd rows are 65 lines of 258 pixels, one outer border of area 0 each: num_contours 5 is tied at the
    cut and takes the first five rows."""
    m = ~_serpentine_mask()
    starts = [(0 if y % 4 == 1 else 1, y) for y in (1, 3, 5, 7, 9)]
    return _from_mask("serpentine_inverse", m, dict(borders=65, chosen=5, selected=5 * 258, longest_chain=2 * 257, tied=True,
                                                    chosen_starts=starts), 5)


def comb():
    """131 x 259: row 0 and every even column. One component of 17159 pixels, one border that runs down and up each of the 130
    teeth (2 * (17159 - 1) points less the 258 diagonal steps between the back and a tooth: 34058); the zero columns between the
    teeth reach the frame at the bottom."""
    m = np.zeros((131, 259), dtype=bool)
    m[0, :] = True
    m[:, 0::2] = True
    return _from_mask("comb", m, dict(borders=1, chosen=1, selected=259 + 130 * 130, longest_chain=34058, tied=False), 5)


# ---- f: thin and nested shapes ---------------------------------------------------------------------------------------------------------------
def rings():
    """67 x 131, six shapes whose borders all differ in area (doubled areas beside each; an n x n square's border has 2 (n - 1)^2,
    the hole border around an h x w hole 2 (h + 1)(w + 1) - 4: the rectangle through the centres of the pixels around the hole with
    its four corners cut):
      * a bull's-eye of three one-pixel rings, 13, 9 and 5 pixels wide, one-pixel gaps: 288, 284, 128, 124, 32, 28
      * a one-pixel ring, 11 x 11: 200, 196
      * a 7 x 14 block with a 5 x 5 and a 5 x 6 hole, one pixel of wall between them: 156, 68, 80
      * a 9 x 10 block with a 3 x 4 and a 4 x 4 hole that touch at a corner only: zero pixels are 4-connected, so two holes: 144, 36, 46
      * an 8 x 8 ring without its top left corner pixel: the ring closes diagonally (set pixels are 8-connected), the missing corner
        is outside, and the 6 x 6 inside stays enclosed: 2 * 49 - 1 = 97, 94
      * a 10 x 10 ring without two opposite corner pixels, in the map's bottom right corner against the frame: its inside reaches the
        outside only through two diagonal gaps, that is not at all: 2 * 81 - 2 = 160, 158
    num_contours 5 cuts between 160 and 158: both borders of the bull's-eye's outer ring and of the 11 x 11 ring, and the outer
    border of the last shape: 169 + 121 + 98 pixels."""
    m = np.zeros((67, 131), dtype=bool)
    for k in (0, 2, 4):
        _ring(m, 3 + k, 2 + k, 13 - 2 * k)
    _ring(m, 30, 60, 11)
    m[20:27, 20:34] = True
    m[21:26, 21:26] = False
    m[21:26, 27:33] = False
    m[40:49, 90:100] = True
    m[41:44, 91:95] = False
    m[44:48, 95:99] = False
    _ring(m, 50, 30, 8)
    m[50, 30] = False
    _ring(m, 57, 121, 10)
    m[57, 121] = m[66, 130] = False
    areas = sorted([288, 284, 128, 124, 32, 28, 200, 196, 156, 68, 80, 144, 36, 46, 97, 94, 160, 158], reverse=True)
    return _from_mask("rings", m, dict(borders=18, chosen=5, selected=169 + 121 + 98, longest_chain=48, tied=False, areas=areas,
                                       chosen_starts=[(2, 3), (2, 4), (60, 30), (60, 31), (122, 57)]), 5)


# ---- g: dilations past 4 ---------------------------------------------------------------------------------------------------------------------
DOTS = ((2, 3), (5, 147), (67, 1), (64, 144),                 # (y, x): within 8 pixels of each corner
        (3, 75), (66, 75), (35, 4), (35, 145),                # of each edge
        (35, 75), (20, 40), (50, 110), (20, 110), (50, 40))   # and inside; any two at least 18 apart in x or in y


def dilate_n(it):
    """70 x 150, thirteen isolated pixels just above the threshold (61 and 254 on a background of 0, 60 and 255 = no value) that the
    dilation turns into (2 it + 1)^2 squares cut off at the frame. No two squares touch up to it = 8, so there are thirteen outer
    borders, all chosen, and `selected` is the mask."""
    assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 18 for a in DOTS for b in DOTS if a != b)
    H, W = 70, 150
    y, x = np.mgrid[0:H, 0:W]
    d = np.choose((x + 2 * y) % 3, [0, 60, 255])
    pixels = 0
    longest = 0
    for i, (dy, dx) in enumerate(DOTS):
        d[dy, dx] = 61 if i % 2 else 254
        h = min(dy + it, H - 1) - max(dy - it, 0) + 1
        w = min(dx + it, W - 1) - max(dx - it, 0) + 1
        pixels += h * w
        longest = max(longest, 2 * (h - 1) + 2 * (w - 1))
    return _case(f"dilate_{it}", d, dict(borders=13, chosen=13, selected=pixels, longest_chain=longest, tied=False), 64,
                 dilate_iterations=it)


# ---- h: sides of 1 and of 8192 ---------------------------------------------------------------------------------------------------------------
def line_8192(column, num_contours):
    """1 x 8192 or 8192 x 1: a run of 4901 pixels, an isolated pixel two pixels after it and a set last pixel: three borders of area
    0. num_contours 2 is tied at the cut by construction (the run and the pixel after it are chosen); 64 takes all three. The
    run's border goes out and back: 2 * 4900 points."""
    m = np.zeros(8192, dtype=bool)
    m[100:5001] = True
    m[5002] = True
    m[8191] = True
    m = m[:, None] if column else m[None, :]
    chosen = min(num_contours, 3)
    first = [(0, 100), (0, 5002), (0, 8191)] if column else [(100, 0), (5002, 0), (8191, 0)]
    return _from_mask(f"{'column' if column else 'row'}_8192_{num_contours}", m, dict(
        borders=3, chosen=chosen, selected=4901 + chosen - 1, longest_chain=9800, tied=num_contours < 3,
        chosen_starts=first[:chosen]), num_contours)


def line_3(column):
    """1 x 3 or 3 x 1, the two end pixels set, median size 31: the window is replicated border almost everywhere, and the composite's
    last three rows and columns are the whole image."""
    m = np.array([True, False, True])
    m = m[:, None] if column else m[None, :]
    return _from_mask("column_3" if column else "row_3", m, dict(borders=2, chosen=2, selected=2, longest_chain=1, tied=False), 5,
                      median_ksize=31)


# ---- i: thousands of borders in thousands of workgroups -------------------------------------------------------------------------------------
LARGE_SEED = 1


def large_blobs():
    """515 x 1030 smoothed noise (three passes, level 0.5) with 3 % of the map without value, one dilation, num_contours 5: the one
    case larger than the golden photograph (the union-find runs in some 2000 workgroups at once). The seed is one at which the cut
    is not tied; the figures are the statement's."""
    rng = np.random.default_rng(LARGE_SEED)
    H, W, smooth = 515, 1030, 3
    a = rng.random((H + 2 * smooth, W + 2 * smooth))
    for _ in range(smooth):
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0) + np.roll(a, -1, 1)) / 5
    a = a[smooth:H + smooth, smooth:W + smooth]
    d = np.where(a > np.quantile(a, 0.5), rng.integers(61, 255, (H, W)), rng.integers(0, 61, (H, W)))
    d[rng.random((H, W)) < 0.03] = 255
    return _case("large_blobs", d, LARGE_FACTS, 5, dilate_iterations=1)


LARGE_FACTS = dict(borders=6685, chosen=5, selected=527530, longest_chain=4664, tied=False)


@functools.lru_cache(maxsize=None)
def all_cases():
    return (dots_lattice(64), dots_lattice(5), equal_squares_staggered(5), equal_squares_staggered(1), ring_and_blob(False),
            ring_and_blob(True), noise_64(), serpentine(), serpentine_inverse(), comb(), rings(), dilate_n(5), dilate_n(6), dilate_n(7),
            dilate_n(8), line_8192(False, 2), line_8192(False, 64), line_8192(True, 2), line_8192(True, 64), line_3(False), line_3(True),
            large_blobs())


NAMES = ("dots_lattice_64", "dots_lattice_5", "equal_squares_staggered_5", "equal_squares_staggered_1", "ring_then_blob",
         "blob_then_ring", "noise_64", "serpentine", "serpentine_inverse", "comb", "rings", "dilate_5", "dilate_6", "dilate_7", "dilate_8",
         "row_8192_2", "row_8192_64", "column_8192_2", "column_8192_64", "row_3", "column_3", "large_blobs")


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, **override):
    """The statement's result (tests/portrait_ref.portrait) of a named case, computed once per session and shared; its arrays are
    read-only. override: parameters other than the case's own (the batch test runs several cases under one set)."""
    c = case(name)
    want = R.portrait(c["image"], c["disparity"], **dict(c["params"], **override))
    for k in ("thresh", "mask", "selected", "blurred", "out"):
        want[k].setflags(write=False)
    return want


# ---- the independent form: borders and fills from connected components ------------------------------------------------------------------
def _boxes(lab):
    """Per label of an integer map: (first pixel's raster index, y min, y max, x min, x max), as arrays indexed by label."""
    H, W = lab.shape
    flat = lab.ravel()
    n = int(flat.max()) + 1
    y, x = np.divmod(np.arange(H * W), W)
    first = np.full(n, H * W)
    np.minimum.at(first, flat, np.arange(H * W))
    lo_y, lo_x = np.full(n, H), np.full(n, W)
    hi_y, hi_x = np.full(n, -1), np.full(n, -1)
    np.minimum.at(lo_y, flat, y)
    np.maximum.at(hi_y, flat, y)
    np.minimum.at(lo_x, flat, x)
    np.maximum.at(hi_x, flat, x)
    return first, lo_y, hi_y, lo_x, hi_x


def check_mask(m, contours):
    """tests/test_portrait_ref._check_mask for maps of any size: the borders' identity, order and roots over the whole map, and every
    border's chain and fill against connected components inside the chain's own bounding box with a margin of one pixel. The
    component that the border belongs to is asserted to lie inside that box, and what lies outside the box reaches the frame, so
    the box decides what the whole map would."""
    import test_portrait_ref as T
    H, W = m.shape
    fg = m != 0
    lab8, _ = T._label(fg, True)
    bg4, _ = T._label(np.pad(~fg, 1, constant_values=True), False)
    frame = bg4[0, 0]
    bg4 = bg4[1:-1, 1:-1]
    box8, box4 = _boxes(lab8), _boxes(bg4)
    want = {(False, int(p) % W, int(p) // W) for c, p in enumerate(box8[0]) if c != 0 and p < H * W}
    want |= {(True, int(p) % W - 1, int(p) // W) for c, p in enumerate(box4[0]) if c != 0 and c != frame and p < H * W}
    assert {(h, c[0][0], c[0][1]) for h, c in contours} == want
    starts = [(c[0][1] * W + c[0][0], h) for h, c in contours]
    assert starts == sorted(starts)
    roots = np.zeros((H, W + 1), dtype=int)     # a border's root: an outer border's start pixel, the pixel right of a hole border's
    for h, c in contours:
        roots[c[0][1], c[0][0] + int(h)] += 1
    assert roots.max(initial=0) <= 1 and not (roots[:, 1:] & roots[:, :-1]).any()
    for hole, chain in contours:
        pts = np.array(chain)
        assert fg[pts[:, 1], pts[:, 0]].all()
        step = np.abs(pts - np.roll(pts, -1, axis=0)).max(axis=1)
        assert len(chain) == 1 or (step == 1).all()            # a closed 8-connected walk
        x0, y0 = chain[0]
        ya, yb, xa, xb = pts[:, 1].min(), pts[:, 1].max(), pts[:, 0].min(), pts[:, 0].max()
        c = bg4[y0, x0 + 1] if hole else lab8[y0, x0]
        _, lo_y, hi_y, lo_x, hi_x = box4 if hole else box8
        assert ya <= lo_y[c] and hi_y[c] <= yb and xa <= lo_x[c] and hi_x[c] <= xb
        ya, yb, xa, xb = max(0, ya - 1), min(H, yb + 2), max(0, xa - 1), min(W, xb + 2)
        box = (slice(ya, yb), slice(xa, xb))
        got = R.fill([(x - xa, y - ya) for x, y in chain], yb - ya, xb - xa)
        same8 = lab8[box] == lab8[y0, x0]
        if not hole:
            assert np.array_equal(got, ~T._outside(same8, False))   # the component and all that it cuts off from the frame
        else:
            b = bg4[box] == c
            on = np.zeros(b.shape, dtype=bool)
            on[pts[:, 1] - ya, pts[:, 0] - xa] = True
            near = np.zeros(b.shape, dtype=bool)                     # pixels of the component around the hole with a 4-neighbour in it
            near[1:] |= b[:-1]
            near[:-1] |= b[1:]
            near[:, 1:] |= b[:, :-1]
            near[:, :-1] |= b[:, 1:]
            assert np.array_equal(on, near & same8)
            assert np.array_equal(got, on | ~T._outside(b, True))    # the border, the hole and all that the hole cuts off
