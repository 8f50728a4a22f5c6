"""CPU: the portrait-mode statement (tests/portrait_ref.py) against independent forms -- the median against scipy's
(or a sort), the dilation against literal 3 x 3 passes, the borders and their fills against connected components, and hand-made masks
with known answers."""
import numpy as np
import pytest

import portrait_ref as R

try:
    from scipy import ndimage
except ImportError:    # the forms below then fall back to plain numpy
    ndimage = None

EIGHT = np.ones((3, 3), dtype=int)


def _label(b, eight):
    """Connected components of a boolean array: (labels from 1, count)."""
    if ndimage is not None:
        return ndimage.label(b, structure=EIGHT if eight else None)
    lab = np.zeros(b.shape, dtype=np.int64)
    n = 0
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if eight else [])
    for y, x in zip(*np.nonzero(b)):
        if lab[y, x]:
            continue
        n += 1
        lab[y, x] = n
        stack = [(y, x)]
        while stack:
            cy, cx = stack.pop()
            for dy, dx in nb:
                yy, xx = cy + dy, cx + dx
                if 0 <= yy < b.shape[0] and 0 <= xx < b.shape[1] and b[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    stack.append((yy, xx))
    return lab, n


def _outside(blocked, eight):
    """Pixels of ~blocked that reach the frame through ~blocked (4- or 8-connected), on the image with a one-pixel frame."""
    free = np.pad(~blocked, 1, constant_values=True)
    lab, _ = _label(free, eight)
    return (lab == lab[0, 0])[1:-1, 1:-1]


def _blobs(rng, H, W, level=0.5, smooth=2):
    a = rng.random((H + 2 * smooth, W + 2 * smooth))
    for _ in range(smooth):
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0) + np.roll(a, -1, 1)) / 5
    a = a[smooth:-smooth, smooth:-smooth] if smooth else a
    return np.where(a > np.quantile(a, level), 255, 0).astype(np.uint8)


def _mask(rows):
    return np.array([[255 if c == "#" else 0 for c in r] for r in rows], dtype=np.uint8)


# ---- median -----------------------------------------------------------------------------------------------------------------------------
def _median_independent(ch, k):
    if ndimage is not None:
        return ndimage.median_filter(ch, size=k, mode="nearest")
    r = k // 2
    p = np.pad(ch, r, mode="edge")
    out = np.empty_like(ch)
    for y in range(ch.shape[0]):
        for x in range(ch.shape[1]):
            out[y, x] = np.sort(p[y:y + k, x:x + k], axis=None)[k * k // 2]
    return out


@pytest.mark.parametrize("shape,k", [((23, 31, 3), 3), ((23, 31, 3), 5), ((40, 37, 3), 15), ((7, 40, 3), 15), ((40, 7, 3), 15),
                                     ((1, 1, 3), 15), ((33, 35, 1), 31), ((19, 20), 7)])
def test_median_equals_independent_form(shape, k):
    rng = np.random.default_rng(k * 100 + shape[0])
    img = rng.integers(0, 256, shape).astype(np.uint8)
    img[: shape[0] // 2] //= 8     # many equal samples in a window
    got = R.median_blur(img, k)
    assert got.shape == img.shape and got.dtype == np.uint8
    planes = img.reshape(shape[0], shape[1], -1)
    for c in range(planes.shape[2]):
        assert np.array_equal(got.reshape(planes.shape)[:, :, c], _median_independent(planes[:, :, c], k))


# ---- mask -------------------------------------------------------------------------------------------------------------------------------
def test_threshold_treats_255_as_no_value():
    d = np.array([[0, 60, 61, 254, 255]], dtype=np.uint8)
    assert R.threshold_mask(d, 60).tolist() == [[0, 0, 255, 255, 0]]
    assert R.threshold_mask(d, 0).tolist() == [[0, 255, 255, 255, 0]]
    assert R.threshold_mask(d, 255).tolist() == [[0, 0, 0, 0, 0]]
    assert d[0, 4] == 255   # the input is not written


@pytest.mark.parametrize("it", [0, 1, 2, 4, 8])
def test_dilate_equals_literal_3x3_passes(it):
    rng = np.random.default_rng(it)
    for H, W in ((1, 1), (5, 9), (17, 13), (3, 40)):
        m = np.where(rng.random((H, W)) > 0.9, 255, 0).astype(np.uint8)
        want = m.copy()
        for _ in range(it):
            p = np.pad(want, 1, mode="edge")
            want = np.max([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)
        assert np.array_equal(R.dilate(m, it), want)


# ---- borders ----------------------------------------------------------------------------------------------------------------------------
def _borders_from_components(m):
    """(hole, start x, start y) of every border, from connected components alone: one outer border per 8-connected component of the
    non-zero pixels, starting at its first pixel in raster order; one hole border per 4-connected component of the zero pixels that
    does not reach the frame, starting at the pixel left of its first pixel."""
    fg = m != 0
    out = set()
    lab, n = _label(fg, True)
    for c in range(1, n + 1):
        y, x = np.argwhere(lab == c)[0]
        out.add((False, int(x), int(y)))
    lab, n = _label(np.pad(~fg, 1, constant_values=True), False)
    for c in range(1, n + 1):
        if c == lab[0, 0]:
            continue
        y, x = np.argwhere(lab == c)[0] - 1
        out.add((True, int(x) - 1, int(y)))
    return out


def _check_mask(m):
    H, W = m.shape
    fg = m != 0
    cs = R.find_contours(m)
    assert {(h, c[0][0], c[0][1]) for h, c in cs} == _borders_from_components(m)
    starts = [(c[0][1] * W + c[0][0], h) for h, c in cs]
    assert starts == sorted(starts)
    roots = np.zeros((H, W + 1), dtype=int)     # a border's root: an outer border's start pixel, the pixel right of a hole border's
    for h, c in cs:
        roots[c[0][1], c[0][0] + int(h)] += 1
    assert roots.max(initial=0) <= 1 and not (roots[:, 1:] & roots[:, :-1]).any()    # never side by side: at most (W + 1) / 2 a row
    lab8, _ = _label(fg, True)
    bg4, _ = _label(np.pad(~fg, 1, constant_values=True), False)
    bg4 = bg4[1:-1, 1:-1]
    for hole, chain in cs:
        pts = np.array(chain)
        assert fg[pts[:, 1], pts[:, 0]].all()
        step = np.abs(pts - np.roll(pts, -1, axis=0)).max(axis=1)
        assert len(chain) == 1 or (step == 1).all()            # a closed 8-connected walk
        got = R.fill(chain, H, W)
        x0, y0 = chain[0]
        if not hole:
            comp = lab8 == lab8[y0, x0]
            assert np.array_equal(got, ~_outside(comp, False))   # the component and all that it cuts off from the frame
        else:
            b = bg4 == bg4[y0, x0 + 1]
            on = np.zeros((H, W), dtype=bool)
            on[pts[:, 1], pts[:, 0]] = True
            near = np.zeros((H, W), dtype=bool)                  # pixels of the component around the hole with a 4-neighbour in it
            near[1:] |= b[:-1]
            near[:-1] |= b[1:]
            near[:, 1:] |= b[:, :-1]
            near[:, :-1] |= b[:, 1:]
            assert np.array_equal(on, near & (lab8 == lab8[y0, x0]))
            assert np.array_equal(got, on | ~_outside(b, True))  # the border, the hole and all that the hole cuts off
    return cs


def test_one_pixel_hole_in_a_block():
    cs = _check_mask(_mask(["###", "#.#", "###"]))
    assert [(h, R.area2(c)) for h, c in cs] == [(False, 8), (True, 4)]
    hole = cs[1][1]
    assert sorted(hole) == [(0, 1), (1, 0), (1, 2), (2, 1)]
    f = R.fill(hole, 3, 3)
    assert f.tolist() == [[False, True, False], [True, True, True], [False, True, False]]


def test_spur_adds_no_area():
    # the walk leaves the block's side for the spur by diagonal steps (the triangle (3, 3), (4, 2), (3, 1): 2 more than the block's 8);
    # the spur itself, out and back over the same pixels, adds nothing however long it is
    a = _check_mask(_mask(["........", ".###....", ".####...", ".###....", "........"]))
    b = _check_mask(_mask(["........", ".###....", ".#######", ".###....", "........"]))
    assert R.area2(a[0][1]) == R.area2(b[0][1]) == 10
    assert len(b[0][1]) == len(a[0][1]) + 6    # three more pixels out and the same three back
    assert R.fill(b[0][1], 5, 8).sum() == 13
    line = _check_mask(_mask(["....", "####", "...."]))
    assert R.area2(line[0][1]) == 0 and len(line[0][1]) == 6 and R.fill(line[0][1], 3, 4).sum() == 4


def test_corner_joined_blobs_are_one_border():
    m = _mask(["##...", "##...", "..##.", "..##.", "....."])
    cs = _check_mask(m)
    assert len(cs) == 1 and not cs[0][0]
    chain = cs[0][1]
    assert chain.count((1, 1)) == 2 or chain.count((2, 2)) == 2    # through the pinch twice
    assert np.array_equal(R.fill(chain, 5, 5), m != 0)


def test_component_touching_the_frame_and_background_cut_off_by_it():
    m = _mask(["#####", "#...#", "#.#.#", "#...#", "#####"])
    cs = _check_mask(m)
    assert [(h, R.area2(c)) for h, c in cs] == [(False, 32), (True, 28), (False, 0)]   # ring, its hole (corners cut), the island in it
    assert R.fill(cs[1][1], 5, 5).sum() == 9 + 12    # hole border: the 3 x 3 inside and the ring's pixels beside it (no corners)
    sel, info = R.select(m, 1)
    assert (sel != 0).all()
    sel, info = R.select(np.flipud(_mask(["#####", "#...#", "#.#.#", "#...#", "##.##"])), 5)
    assert len(info["contours"]) == 2    # the background reaches the frame: no hole border


def test_hole_outranks_smaller_outer_border():
    m = _mask(["#######..", "#.....#..", "#.....#..", "#.....#.#", "#######.#"])
    sel, info = R.select(m, 2)
    kinds = [(info["contours"][i][0], -info["keys"][i][0]) for i in info["order"]]
    assert kinds == [(False, 48), (True, 44), (False, 0)]   # the hole border cuts the ring's four corners
    assert sel[3, 8] == 0 and sel[2, 3] == R.SELECTED


def test_fewer_borders_than_asked_for_and_empty_masks():
    m = _mask(["#..", "...", "..#"])
    sel, info = R.select(m, 5)
    assert len(info["chosen"]) == 2 and np.array_equal(sel != 0, m != 0)
    sel, info = R.select(np.zeros((4, 6), np.uint8), 5)
    assert not sel.any() and info["contours"] == []
    sel, info = R.select(np.full((4, 6), 255, np.uint8), 5)
    assert (sel == R.SELECTED).all() and len(info["contours"]) == 1 and R.area2(info["contours"][0][1]) == 2 * 3 * 5
    sel, info = R.select(np.full((1, 1), 255, np.uint8), 5)
    assert sel.tolist() == [[R.SELECTED]]


def test_tie_rule_is_start_pixel_then_outer_first():
    m = _mask(["##.##.##", "##.##.##"])
    sel, info = R.select(m, 2)
    assert info["chosen"] == [0, 1] and R.cut_is_tied(info["contours"], 8, 2) and not R.cut_is_tied(info["contours"], 8, 3)
    assert (sel[:, 6:] == 0).all() and (sel[:, :2] != 0).all()


@pytest.mark.parametrize("seed", range(12))
def test_random_blobs_against_components(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    m = _blobs(rng, H, W, level=float(rng.uniform(0.3, 0.7)), smooth=int(rng.integers(0, 3)))
    _check_mask(m)


# ---- the whole tail ---------------------------------------------------------------------------------------------------------------------
def test_composite_keeps_last_three_rows_and_columns_blurred():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (20, 24, 3)).astype(np.uint8)
    r = R.portrait(img, np.full((20, 24), 200, np.uint8))
    assert (r["selected"] == R.SELECTED).all()
    assert np.array_equal(r["out"][:17, :21], img[:17, :21])
    assert np.array_equal(r["out"][17:], r["blurred"][17:]) and np.array_equal(r["out"][:, 21:], r["blurred"][:, 21:])
    r = R.portrait(img, np.full((20, 24), 255, np.uint8))     # no value anywhere: nothing selected
    assert not r["selected"].any() and np.array_equal(r["out"], r["blurred"])
    r = R.portrait(img[:2, :3], np.full((2, 3), 200, np.uint8))
    assert np.array_equal(r["out"], r["blurred"])


def test_parameters_checked():
    img, d = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    for kw in (dict(threshold=-1), dict(threshold=256), dict(dilate_iterations=9), dict(num_contours=0), dict(num_contours=65),
               dict(median_ksize=4), dict(median_ksize=1), dict(median_ksize=33)):
        with pytest.raises(ValueError):
            R.portrait(img, d, **kw)
    with pytest.raises(TypeError):
        R.portrait(img, d, ksize=3)
