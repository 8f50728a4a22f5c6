"""CPU statement of portrait mode: the image tail of the reference's createPortraitMode (DisparityUtil.cpp:317-412).

    disparity[disparity == 255] = 0; threshold(disparity, thresh, 60, 255, THRESH_BINARY)
    dilate(thresh, img_final, Mat(), Point(-1, -1), 2, BORDER_REPLICATE)
    findContours(img_final, contours, hierarchy, RETR_LIST, CHAIN_APPROX_NONE)
    sort(contours by |contourArea| descending); drawContours(img_final, contours, i, 100, FILLED) for i < 5
    medianBlur(img_1, blurred, 15); blurred[i, j] = img_1[i, j] where img_final[i, j] is 100, i < rows - 3, j < cols - 3

Parity with OpenCV is unpinned (there is no OpenCV to run): this file is read from the reference's first-party code and from the
published algorithms (Suzuki and Abe 1985 for the borders, in OpenCV's neighbour numbering), and gms_portrait_device returns the same
arrays. Two calls of the reference have no effect on the result and are left out:
  * drawContours(img_final, contours, -1, Scalar(0, 255, 0), 2) (:364) writes 0 into a one-channel image AFTER the contours were
    extracted and BEFORE the fill; the last loop (:404) asks only "neither 0 nor 255", that is "is 100", so a pixel set to 0 there
    and then filled is 100 and a pixel set to 0 and not filled fails the test exactly as its earlier 0 or 255 did.
  * rectangle(img_final, bounding_rect, ...) (:385) gets a default-constructed, empty Rect; OpenCV 4.5.2's rectangle(Mat&, Rect, ...)
    draws only if rec.area() > 0 (from memory of the source; a stated choice).
The reference indexes five contours whether or not five exist (an OpenCV assertion otherwise); here fewer than num_contours borders
means all of them. Where the reference's order could show -- equal area between the last chosen border and the first one left out --
this statement ranks by the raster order of the border's start pixel, outer border before hole border. That is NOT the reference's
rule (MSVC's std::sort on OpenCV's contour order): the GPU tests' seeded and photographic inputs avoid such ties, and the named
cases of tests/portrait_cases.py that are tied on purpose test this rule as the project's own.
"""
import numpy as np

REFERENCE_PARAMS = dict(threshold=60, dilate_iterations=2, num_contours=5, median_ksize=15)
PARAM_NAMES = tuple(REFERENCE_PARAMS)    # the field order of gms_portrait_params
SELECTED = 255                           # the value of a chosen pixel in `selected` (the reference paints 100; only "set" matters)


def params(**kw):
    p = dict(REFERENCE_PARAMS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(f"unknown portrait parameter {k!r}")
        p[k] = int(v)
    return p


def check(p, W, H):
    """The accepted sets (include/gms.h); everything else is GMS_ERR_BAD_ARG."""
    bad = []
    if not 0 <= p["threshold"] <= 255:
        bad.append("threshold 0..255")
    if not 0 <= p["dilate_iterations"] <= 8:
        bad.append("dilate_iterations 0..8")
    if not 1 <= p["num_contours"] <= 64:
        bad.append("num_contours 1..64")
    if not (3 <= p["median_ksize"] <= 31 and p["median_ksize"] % 2 == 1):
        bad.append("median_ksize odd in 3..31")
    if not (1 <= W <= 8192 and 1 <= H <= 8192):
        bad.append("width, height 1..8192")
    if bad:
        raise ValueError("portrait: " + "; ".join(bad))


# ---- steps 1-3: the mask --------------------------------------------------------------------------------------------------------------
def threshold_mask(disparity, threshold):
    """255 where the disparity (255 = no value -> 0) is above the threshold, else 0 (:317-323, :342)."""
    d = np.array(disparity, dtype=np.uint8)
    d[d == 255] = 0
    return np.where(d > threshold, 255, 0).astype(np.uint8)


def dilate(mask, iterations):
    """`iterations` passes of a 3 x 3 maximum with replicated border = one (2 it + 1)^2 maximum over the part of the window inside the
    image (a replicated pixel adds nothing to a maximum that already holds the pixel it copies)."""
    m = np.asarray(mask, dtype=np.uint8)
    H, W = m.shape
    r = int(iterations)
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if ys < ye and xs < xe:
                np.maximum(out[ys:ye, xs:xe], m[ys + dy:ye + dy, xs + dx:xe + dx], out=out[ys:ye, xs:xe])
    return out


# ---- step 4: Suzuki-Abe border following, RETR_LIST, CHAIN_APPROX_NONE ------------------------------------------------------------------
# neighbour s of a pixel: 0 east, then counter-clockwise on the screen (1 north-east, 2 north, ..., 7 south-east)
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, -1, -1, -1, 0, 1, 1, 1)


def _follow(f, i0, j0, hole, nbd):
    """One border from its start pixel (row i0, column j0 of the framed image f, a list of lists that is marked in place)."""
    s_end = s = 0 if hole else 4           # the 0-pixel that made this a start: east for a hole border, west for an outer border
    while True:                            # clockwise from there: the first non-zero neighbour
        s = (s - 1) & 7
        if f[i0 + DY[s]][j0 + DX[s]] != 0 or s == s_end:
            break
    if s == s_end:                         # an isolated pixel
        f[i0][j0] = -nbd
        return [(j0 - 1, i0 - 1)]
    chain = []
    i1, j1 = i0 + DY[s], j0 + DX[s]
    i3, j3 = i0, j0
    while True:
        s_end = s
        while True:                        # counter-clockwise from the neighbour after the previous border pixel
            s += 1
            if f[i3 + DY[s & 7]][j3 + DX[s & 7]] != 0:
                break
        s &= 7
        if s != 0 and s - 1 < s_end:       # the east neighbour was looked at and is 0: the border's right-hand end on this row
            f[i3][j3] = -nbd
        elif f[i3][j3] == 1:
            f[i3][j3] = nbd
        chain.append((j3 - 1, i3 - 1))
        i4, j4 = i3 + DY[s], j3 + DX[s]
        if (i4, j4) == (i0, j0) and (i3, j3) == (i1, j1):
            return chain
        i3, j3 = i4, j4
        s = (s + 4) & 7


def find_contours(mask):
    """Every outer border and every hole border of the non-zero pixels (8-connected; a frame of zeros around the image), each as
    (hole, chain): chain = the border's pixels (x, y) in the order they are followed, every point kept. In the raster order of the
    start pixels, an outer border first where one pixel starts both."""
    m = np.asarray(mask)
    H, W = m.shape
    fr = np.zeros((H + 2, W + 2), dtype=np.int64)
    fr[1:-1, 1:-1] = m != 0
    f = fr.tolist()
    out = []
    nbd = 1
    for i in range(1, H + 1):
        row = f[i]
        for j in range(1, W + 1):
            v = row[j]
            if v == 0:
                continue
            if v == 1 and row[j - 1] == 0:
                hole = False
            elif v >= 1 and row[j + 1] == 0:
                hole = True
            else:
                continue
            nbd += 1
            out.append((hole, _follow(f, i, j, hole, nbd)))
    return out


# ---- steps 5-6: rank by area, fill ------------------------------------------------------------------------------------------------------
def area2(chain):
    """|contourArea| doubled: the absolute shoelace sum of the closed chain, an exact integer."""
    p = np.asarray(chain, dtype=np.int64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    return abs(int(np.sum(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1])))


def rank(contours, W):
    """Indices of the borders by doubled area descending; equal areas by the start pixel's raster index, outer before hole (this
    statement's own rule, see the module text). Returns (order, keys): keys[i] = (-area2, start index, hole) of border i."""
    keys = [(-area2(c), c[0][1] * W + c[0][0], int(h)) for h, c in contours]
    return sorted(range(len(keys)), key=lambda i: keys[i]), keys


def cut_is_tied(contours, W, num_contours):
    """True where the last chosen border and the first one left out have equal area: the one case in which the choice is this
    statement's and not the reference's."""
    order, keys = rank(contours, W)
    return len(order) > num_contours and keys[order[num_contours - 1]][0] == keys[order[num_contours]][0]


def fill(chain, H, W):
    """drawContours(FILLED) of one chain: the pixels on it and the pixels whose centre the closed lattice polygon encloses, even-odd.
    A ray from the pixel towards -x, an infinitesimal step below the pixel's row, crosses exactly the chain's edges that go between
    this row and the next one, each at the x of its end on this row (left or right of every pixel that is not on the chain, never
    on it); an edge traversed twice cancels."""
    on = np.zeros((H, W), dtype=bool)
    tog = np.zeros((H, W), dtype=np.uint8)
    n = len(chain)
    for a in range(n):
        (x0, y0), (x1, y1) = chain[a], chain[(a + 1) % n]
        on[y0, x0] = True
        if y0 != y1:
            tog[min(y0, y1), x0 if y0 < y1 else x1] ^= 1
    left = np.bitwise_xor.accumulate(tog, axis=1) ^ tog     # crossings at x < the pixel's
    return on | (left != 0)


def select(mask, num_contours):
    """Steps 4-6 on the dilated mask: `selected` (SELECTED where a chosen border's fill covers the pixel, else 0), and the contours,
    their ranking and the chosen indices for the tests."""
    m = np.asarray(mask)
    H, W = m.shape
    contours = find_contours(m)
    order, keys = rank(contours, W)
    chosen = order[:num_contours]
    sel = np.zeros((H, W), dtype=bool)
    for i in chosen:
        sel |= fill(contours[i][1], H, W)
    return np.where(sel, SELECTED, 0).astype(np.uint8), dict(contours=contours, order=order, keys=keys, chosen=chosen)


# ---- step 8: medianBlur -----------------------------------------------------------------------------------------------------------------
def median_blur(image, ksize):
    """medianBlur(image, ksize): per channel the (ksize^2 / 2)-th smallest (from 0) of the ksize^2 samples, BORDER_REPLICATE. image:
    uint8 [H, W] or [H, W, C]."""
    img = np.asarray(image, dtype=np.uint8)
    k = int(ksize)
    r = k // 2
    pad = np.pad(img, ((r, r), (r, r)) + ((0, 0),) * (img.ndim - 2), mode="edge")
    H, W = img.shape[:2]
    out = np.empty_like(img)
    rows = max(1, (1 << 25) // max(1, W * k * k * (img.shape[2] if img.ndim == 3 else 1)))   # about 32 MiB of windows at a time
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        win = np.lib.stride_tricks.sliding_window_view(pad[y0:y1 + 2 * r], (k, k), axis=(0, 1))
        flat = win.reshape(win.shape[:-2] + (k * k,))
        out[y0:y1] = np.partition(flat, k * k // 2, axis=-1)[..., k * k // 2]
    return out


# ---- the whole tail ---------------------------------------------------------------------------------------------------------------------
def portrait(image, disparity, **kw):
    """image: uint8 [H, W, 3] (BGR); disparity: uint8 [H, W], 255 = no value. Returns a dict: thresh, mask (dilated), selected,
    blurred, out (the portrait image), and info (contours, ranking, chosen)."""
    p = params(**kw)
    img = np.asarray(image, dtype=np.uint8)
    disp = np.asarray(disparity, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3 or disp.shape != img.shape[:2]:
        raise ValueError("image [H, W, 3] and disparity [H, W]")
    H, W = disp.shape
    check(p, W, H)
    thresh = threshold_mask(disp, p["threshold"])
    mask = dilate(thresh, p["dilate_iterations"])
    selected, info = select(mask, p["num_contours"])
    blurred = median_blur(img, p["median_ksize"])
    keep = selected != 0
    keep[max(H - 3, 0):, :] = False        # the reference's loop bounds (:402-403): the last three rows and columns stay blurred
    keep[:, max(W - 3, 0):] = False
    out = np.where(keep[:, :, None], img, blurred)
    return dict(thresh=thresh, mask=mask, selected=selected, blurred=blurred, out=out, info=info)
