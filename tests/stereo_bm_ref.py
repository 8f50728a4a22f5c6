"""CPU statement of the reference's block-matching baseline (DisparityUtil.cpp:22-49):

    StereoBM::create(16, 5); numDisparities 224; preFilterSize 5; preFilterCap 61; minDisparity -39; textureThreshold 507;
    uniquenessRatio 0; speckleWindowSize 0; speckleRange 8; disp12MaxDiff 1
    compute(g1, g2, disparity)                                  // CV_16S, 4 fractional bits
    normalize(disparity, disparity, 0, 255, NORM_MINMAX, CV_8U); every 0 pixel -> 255

OpenCV 4.5.2's StereoBM::compute on its integer path (findStereoCorrespondenceBM, then validateDisparity, then the fill outside
getValidDisparityROI), stated for every accepted parameter set. No OpenCV is at hand to pin it against: the statement is read from
that release's published source, not checked against it.

Two forms that must agree: stereo_bm_loop, a literal per-pixel loop for small images, and stereo_bm, a vectorised one (window sums
from cumulative sums) for the 450 x 375 fixture, made of pieces (window_costs, decisions, raw_maps, lr_sources, validate, roi_fill) that
tests/stereo_bm_cases.py counts with. Both return (disp int16 [H, W], cost int32 [H, W]); the cost of a pixel is
sad[mind] wherever the winner-take-all step gave it a disparity (before the left-right check and the ROI fill), -1 elsewhere.
gms_stereo_bm_device returns the same two arrays.
"""
import numpy as np

PREFILTER_NORMALIZED_RESPONSE = 0
PREFILTER_XSOBEL = 1

# the reference's StereoBM (DisparityUtil.cpp:24-36); preFilterType is OpenCV's default, XSOBEL
REFERENCE_PARAMS = dict(block_size=5, num_disparities=224, min_disparity=-39, pre_filter_type=PREFILTER_XSOBEL, pre_filter_size=5,
                        pre_filter_cap=61, texture_threshold=507, uniqueness_ratio=0, speckle_window_size=0, speckle_range=8,
                        disp12_max_diff=1)
PARAM_NAMES = tuple(REFERENCE_PARAMS)   # the field order of gms_stereo_bm_params
MAX_WIDTH = 8192                        # GMS_STEREO_BM_MAX_WIDTH: one row of the left-right check lives in LDS
DBL_EPSILON = float(np.finfo(np.float64).eps)


def make_params(**kw):
    p = dict(REFERENCE_PARAMS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(f"unknown StereoBM parameter {k!r}")
        p[k] = int(v)
    return p


def check_params(p, width, height):
    """What the library rejects with GMS_ERR_BAD_ARG (ValueError here)."""
    bs, nd, md = p["block_size"], p["num_disparities"], p["min_disparity"]
    bad = []
    if p["pre_filter_type"] != PREFILTER_XSOBEL:
        bad.append("only PREFILTER_XSOBEL")
    if not (5 <= p["pre_filter_size"] <= 255 and p["pre_filter_size"] % 2 == 1):
        bad.append("preFilterSize odd in 5..255")
    if not 1 <= p["pre_filter_cap"] <= 63:
        bad.append("preFilterCap in 1..63")
    if not (5 <= bs <= 51 and bs % 2 == 1):
        bad.append("blockSize odd in 5..51")
    if not (0 < nd <= 512 and nd % 16 == 0):
        bad.append("numDisparities a positive multiple of 16 up to 512")
    elif not (-2047 <= md and md + nd <= 2048):
        bad.append("every disparity and FILTERED in 16 bits: minDisparity >= -2047, minDisparity + numDisparities <= 2048")
    if not (0 <= p["texture_threshold"] and 0 <= p["uniqueness_ratio"] <= 1000):
        bad.append("textureThreshold >= 0, uniquenessRatio in 0..1000")
    if p["speckle_window_size"] != 0:
        bad.append("speckleWindowSize must be 0")
    if not (0 < width <= MAX_WIDTH and height > 0):
        bad.append(f"width in 1..{MAX_WIDTH}, height > 0")
    elif bs >= min(width, height):
        bad.append("blockSize below the width and the height")
    if bad:
        raise ValueError("StereoBM: " + "; ".join(bad))


def filtered_value(p):
    return (p["min_disparity"] - 1) * 16


def ranges(p, width):
    """(lofs, rofs, width1, nothing computed). Output column lofs + x for x in [0, width1), cut at the image's width: with
    minDisparity > 0, lofs + width1 = W + minDisparity, and OpenCV's loop writes the excess into the next row's first columns, which
    its ROI fill then overwrites."""
    nd, md = p["num_disparities"], p["min_disparity"]
    lofs = max(nd - 1 + md, 0)
    rofs = -min(nd - 1 + md, 0)
    width1 = width - rofs - nd + 1
    return lofs, rofs, width1, (width1 < 1 or lofs >= width or rofs >= width)


def c_div(a, b):
    """C's integer division (truncation toward zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def subpixel(nd, md, mind, p, n, c):
    """The 4-fractional-bit disparity of winner mind with cost c and neighbour costs p = sad[mind+1], n = sad[mind-1]."""
    den = p + n - 2 * c + abs(p - n)
    return ((nd - mind - 1 + md) * 256 + (c_div((p - n) * 256, den) if den else 0) + 15) >> 4


def winner(sad):
    """(mind, minsad): the first k with the strictly smallest cost -- equal costs go to the largest disparity."""
    minsad, mind = 2 ** 31 - 1, -1
    for k, s in enumerate(sad):
        if s < minsad:
            minsad, mind = s, k
    return mind, minsad


def decide(sad, tex, p):
    """The per-pixel decision on the costs sad[0..nd) and the texture sum: (raw disparity, cost), or None when filtered."""
    nd, md = p["num_disparities"], p["min_disparity"]
    mind, minsad = winner(sad)
    if tex < p["texture_threshold"]:
        return None
    ur = p["uniqueness_ratio"]
    if ur > 0:
        thresh = minsad + (minsad * ur) // 100
        for k in range(nd):
            if (k < mind - 1 or k > mind + 1) and sad[k] <= thresh:
                return None
    pp = sad[mind + 1] if mind + 1 < nd else sad[nd - 2]
    nn = sad[mind - 1] if mind >= 1 else sad[1]
    return subpixel(nd, md, mind, pp, nn, minsad), minsad


# ---- pre-filter ----------------------------------------------------------------------------------------------------------------------
def prefilter_xsobel_loop(img, cap):
    """prefilterXSobel, literally: rows in pairs y, y+1; an odd height's last row is all cap."""
    src = [[int(v) for v in row] for row in np.asarray(img, np.uint8)]
    H, W = len(src), len(src[0])
    dst = [[0] * W for _ in range(H)]

    def tab(v):
        return 0 if v < -cap else 2 * cap if v > cap else v + cap

    y = 0
    while y < H - 1:
        r1 = src[y]
        r0 = src[y - 1] if y > 0 else src[y + 1]
        r2 = src[y + 1]
        r3 = src[y + 2] if y < H - 2 else r1
        d0, d1 = dst[y], dst[y + 1]
        d0[0] = d0[W - 1] = d1[0] = d1[W - 1] = cap
        for x in range(1, W - 1):
            a = r0[x + 1] - r0[x - 1]
            b = r1[x + 1] - r1[x - 1]
            c = r2[x + 1] - r2[x - 1]
            d = r3[x + 1] - r3[x - 1]
            d0[x] = tab(a + 2 * b + c)
            d1[x] = tab(b + 2 * c + d)
        y += 2
    for yy in range(y, H):
        dst[yy] = [cap] * W
    return np.array(dst, np.uint8).reshape(H, W)


def prefilter_xsobel(img, cap):
    """The same, vectorised: reflect-101 rows, clamp(d(y-1) + 2 d(y) + d(y+1), -cap, cap) + cap, d(r) = I[r][x+1] - I[r][x-1]."""
    I = np.asarray(img, np.uint8).astype(np.int32)
    H, W = I.shape
    out = np.full((H, W), cap, np.uint8)
    n = H - (H % 2)
    if n == 0 or W < 3:
        return out
    ys = np.arange(n)
    up = np.where(ys > 0, ys - 1, 1)
    dn = np.where(ys + 1 < H, ys + 1, ys - 1)
    d = I[:, 2:] - I[:, :-2]
    out[:n, 1:-1] = np.clip(d[up] + 2 * d[ys] + d[dn], -cap, cap) + cap
    return out


# ---- left-right check and ROI --------------------------------------------------------------------------------------------------------
def validate_loop(disp, cost, p):
    """validateDisparity, literally, on the raw map (in place)."""
    H, W = disp.shape
    nd, md, maxdiff = p["num_disparities"], p["min_disparity"], p["disp12_max_diff"] * 16
    inv = (md - 1) * 16
    minX1, maxX1 = max(md + nd, 0), W + min(md, 0)
    for y in range(H):
        d2 = [inv] * W
        c2 = [2 ** 31 - 1] * W
        for x in range(minX1, maxX1):
            d, c = int(disp[y, x]), int(cost[y, x])
            if d == inv:
                continue
            x2 = x - ((d + 8) >> 4)
            if c2[x2] > c:
                c2[x2] = c
                d2[x2] = d
        for x in range(minX1, maxX1):
            d = int(disp[y, x])
            if d == inv:
                continue
            x0, x1 = x - (d >> 4), x - ((d + 15) >> 4)
            if (0 <= x0 < W and d2[x0] > inv and abs(d2[x0] - d) > maxdiff and
                    0 <= x1 < W and d2[x1] > inv and abs(d2[x1] - d) > maxdiff):
                disp[y, x] = inv


def lr_sources(disp, cost, p):
    """The sources of validateDisparity's first pass on the raw map: (ys, x, d, c, x2), one entry per pixel of its column range that has
    a disparity -- its row, column, disparity, cost and the target column x - ((d + 8) >> 4) it votes for. None when the range is empty."""
    W = disp.shape[1]
    nd, md = p["num_disparities"], p["min_disparity"]
    inv = (md - 1) * 16
    minX1, maxX1 = max(md + nd, 0), W + min(md, 0)
    if maxX1 <= minX1:
        return None
    sub = disp[:, minX1:maxX1].astype(np.int64)
    ys, xs = np.nonzero(sub != inv)
    d = sub[ys, xs]
    x = xs + minX1
    c = cost[ys, x].astype(np.int64)
    return ys, x, d, c, x - ((d + 8) >> 4)


def validate(disp, cost, p):
    """validateDisparity, vectorised over all rows: per target (y, x2) the strictly lowest cost, the lowest x on ties."""
    H, W = disp.shape
    md, maxdiff = p["min_disparity"], p["disp12_max_diff"] * 16
    inv = (md - 1) * 16
    src = lr_sources(disp, cost, p)
    if src is None:
        return
    ys, x, d, c, x2 = src
    g = ys * W + x2
    order = np.lexsort((x, c, g))
    first = np.ones(len(order), bool)
    first[1:] = g[order][1:] != g[order][:-1]
    win = order[first]
    disp2 = np.full(H * W, inv, np.int64)
    disp2[g[win]] = d[win]
    disp2 = disp2.reshape(H, W)

    def off(xq):
        ok = (xq >= 0) & (xq < W)
        v = disp2[ys, np.clip(xq, 0, W - 1)]
        return ok & (v > inv) & (np.abs(v - d) > maxdiff)

    kill = off(x - (d >> 4)) & off(x - ((d + 15) >> 4))
    disp[ys[kill], x[kill]] = inv


def roi_fill(disp, p, lofs):
    """FILTERED outside getValidDisparityROI of two full-image ROIs: columns [lofs + w2, W - w2), rows [w2, H - w2)."""
    H, W = disp.shape
    w2 = p["block_size"] // 2
    inv = filtered_value(p)
    disp[:, :min(lofs + w2, W)] = inv
    disp[:, max(W - w2, 0):] = inv
    disp[:w2, :] = inv
    disp[max(H - w2, 0):, :] = inv


# ---- StereoBM::compute ---------------------------------------------------------------------------------------------------------------
def _prepare(left, right, kw):
    p = make_params(**kw)
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    if left.ndim != 2 or right.shape != left.shape:
        raise ValueError("left and right: two 8-bit images of one size")
    H, W = left.shape
    check_params(p, W, H)
    return p, left, right, H, W


def stereo_bm_loop(left, right, **kw):
    """Literal per-pixel form (small images only): (disp int16, cost int32)."""
    p, left, right, H, W = _prepare(left, right, kw)
    nd, cap, w2 = p["num_disparities"], p["pre_filter_cap"], p["block_size"] // 2
    disp = np.full((H, W), filtered_value(p), np.int16)
    cost = np.full((H, W), -1, np.int32)
    lofs, rofs, width1, none = ranges(p, W)
    if none:
        return disp, cost
    L = prefilter_xsobel_loop(left, cap).astype(np.int64).tolist()
    R = prefilter_xsobel_loop(right, cap).astype(np.int64).tolist()

    def clamp(v, lo, hi):
        return lo if v < lo else hi if v > hi else v

    for y in range(w2, H - w2):
        for x in range(min(width1, W - lofs)):
            sad = [0] * nd
            tex = 0
            for dy in range(-w2, w2 + 1):
                lr, rr = L[y + dy], R[y + dy]
                for j in range(-w2, w2 + 1):
                    lv = lr[lofs + clamp(x + j, -lofs, W - 1 - lofs)]
                    rc = rofs + clamp(x + j, -rofs, W - nd - rofs)
                    tex += abs(lv - cap)
                    for k in range(nd):
                        sad[k] += abs(lv - rr[rc + k])
            r = decide(sad, tex, p)
            if r is not None:
                disp[y, lofs + x], cost[y, lofs + x] = r
    if p["disp12_max_diff"] >= 0:
        validate_loop(disp, cost, p)
    roi_fill(disp, p, lofs)
    return disp, cost


def window_costs(left, right, p):
    """The cost volume of the computed region, by cumulative sums: (sad int64 [nd, ny, wx], tex int64 [ny, wx]) for the rows
    [w2, H - w2) and the output columns lofs + [0, wx), wx = min(width1, W - lofs)."""
    H, W = left.shape
    nd, cap, bs = p["num_disparities"], p["pre_filter_cap"], p["block_size"]
    w2 = bs // 2
    lofs, rofs, width1, _ = ranges(p, W)
    wx = min(width1, W - lofs)
    L = prefilter_xsobel(left, cap).astype(np.int32)
    R = prefilter_xsobel(right, cap).astype(np.int32)
    ny = H - 2 * w2
    xs = np.arange(wx)[:, None] + np.arange(-w2, w2 + 1)[None, :]   # [wx, bs]
    cl = np.clip(xs, -lofs, W - 1 - lofs) + lofs
    cr = np.clip(xs, -rofs, W - nd - rofs) + rofs

    def vsum(h):  # per-row sums [H, wx] -> window sums for the rows [w2, H - w2)
        c = np.concatenate([np.zeros((1, h.shape[1]), np.int64), np.cumsum(h, axis=0, dtype=np.int64)])
        return c[bs:] - c[:-bs]

    Lw = L[:, cl]                                                  # [H, wx, bs]
    tex = vsum(np.abs(Lw - cap).sum(axis=2))
    sad = np.empty((nd, ny, wx), np.int64)
    for k in range(nd):
        sad[k] = vsum(np.abs(Lw - R[:, cr + k]).sum(axis=2))
    return sad, tex


def decisions(sad, tex, p):
    """decide over the whole cost volume: a dict of [ny, wx] arrays -- mind and minsad (the winner), tex_ok and uniq_ok (the two rules;
    a pixel is accepted when both hold), den (the subpixel step's denominator) and disp (the raw disparity of an accepted pixel)."""
    nd, md = p["num_disparities"], p["min_disparity"]
    ny, wx = tex.shape
    mind = np.argmin(sad, axis=0)                                  # the first strict minimum: the lowest k
    yy, xx = np.meshgrid(np.arange(ny), np.arange(wx), indexing="ij")
    minsad = sad[mind, yy, xx]
    tex_ok = tex >= p["texture_threshold"]
    uniq_ok = np.ones_like(tex_ok)
    ur = p["uniqueness_ratio"]
    if ur > 0:
        thresh = minsad + (minsad * ur) // 100
        far = np.abs(np.arange(nd)[:, None, None] - mind[None]) > 1
        uniq_ok = ~np.any(far & (sad <= thresh[None]), axis=0)
    pp = sad[np.where(mind + 1 < nd, mind + 1, nd - 2), yy, xx]
    nn = sad[np.where(mind >= 1, mind - 1, 1), yy, xx]
    den = pp + nn - 2 * minsad + np.abs(pp - nn)
    num = (pp - nn) * 256
    frac = np.where(den != 0, np.sign(num) * (np.abs(num) // np.where(den != 0, den, 1)), 0)
    dv = ((nd - mind - 1 + md) * 256 + frac + 15) >> 4
    return dict(mind=mind, minsad=minsad, tex_ok=tex_ok, uniq_ok=uniq_ok, den=den, disp=dv)


def raw_maps(left, right, p):
    """findStereoCorrespondenceBM's output before the left-right check and the ROI fill: (disp int16, cost int32, the decisions; None
    when nothing is computed)."""
    H, W = left.shape
    w2 = p["block_size"] // 2
    disp = np.full((H, W), filtered_value(p), np.int16)
    cost = np.full((H, W), -1, np.int32)
    lofs, _, _, none = ranges(p, W)
    if none:
        return disp, cost, None
    sad, tex = window_costs(left, right, p)
    dec = decisions(sad, tex, p)
    dec["sad"] = sad
    ok = dec["tex_ok"] & dec["uniq_ok"]
    wx = tex.shape[1]
    disp[w2:H - w2, lofs:lofs + wx] = np.where(ok, dec["disp"], filtered_value(p))
    cost[w2:H - w2, lofs:lofs + wx] = np.where(ok, dec["minsad"], -1)
    return disp, cost, dec


def stereo_bm(left, right, **kw):
    """Vectorised form: (disp int16, cost int32), equal to stereo_bm_loop."""
    p, left, right, H, W = _prepare(left, right, kw)
    disp, cost, dec = raw_maps(left, right, p)
    if dec is None:
        return disp, cost
    if p["disp12_max_diff"] >= 0:
        validate(disp, cost, p)
    roi_fill(disp, p, ranges(p, W)[0])
    return disp, cost


# ---- the reference's stereo_match ----------------------------------------------------------------------------------------------------
def normalize_u8(disp):
    """normalize(disp, disp, 0, 255, NORM_MINMAX, CV_8U) over the whole int16 map, then every 0 -> 255. OpenCV's arithmetic:
    scale = 255 * (1 / (max - min)) (0 when max == min) and shift = 0 - min * scale in double, both cast to float; each value is
    v * scale + shift in float32, not fused, rounded half to even and saturated to 0..255."""
    d = np.asarray(disp, np.int16)
    mn, mx = float(d.min()), float(d.max())
    scale = 255.0 * (1.0 / (mx - mn) if mx - mn > DBL_EPSILON else 0.0)
    shift = 0.0 - mn * scale
    v = d.astype(np.float32) * np.float32(scale)
    v = v + np.float32(shift)
    out = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    out[out == 0] = 255
    return out


def stereo_match(left, right, **kw):
    """DisparityUtil.cpp:22-49: the reference's 8-bit map."""
    return normalize_u8(stereo_bm(left, right, **kw)[0])
