"""CPU statement of the library's semi-global matching (gms_stereo_sgm_device; Hirschmueller 2008 for the idea). It is
the library's own definition, NOT cv::StereoSGBM: the matching cost is StereoBM's window SAD, not Birchfield-Tomasi, and no OpenCV source
is restated here. Everything but the path aggregation is a piece of tests/stereo_bm_ref.py.

    C[y, x, k]   stereo_bm_ref.window_costs: StereoBM's SAD after its XSOBEL pre-filter, for the rows [w2, H - w2) and the output columns
                 lofs + [0, wx); k in [0, nd) means disparity nd - 1 + md - k. tex is its texture sum. The region is empty exactly where
                 StereoBM computes nothing.
    paths        (dy, dx) = (0,1), (0,-1), (1,0), (-1,0), then (1,1), (1,-1), (-1,1), (-1,-1); n_paths = 4 uses the first four. A pixel
                 whose predecessor (y - dy, x - dx) lies outside the region has L = C; every other pixel
                 L[k] = C[k] + min(Lp[k], Lp[k - 1] + p1, Lp[k + 1] + p1, m + p2) - m,  m = min_k Lp[k],
                 terms with k +- 1 outside [0, nd) left out. S is the sum of L over the paths.
    decision     stereo_bm_ref.decisions / validate / roi_fill on S in place of the SADs: the lowest k among equal S wins, the texture
                 rule runs on tex, the uniqueness rule on S, the subpixel step mirrors at the ends, the cost of a pixel is S[winner].

Parameters: StereoBM's, p1 (default 8 block_size^2), p2 (default 32 block_size^2) and n_paths (default 8). Accepted: what StereoBM
accepts, 0 <= p1 <= p2, n_paths 4 or 8, and n_paths (block_size^2 2 pre_filter_cap + p2) <= 65535, which keeps every L and S within 16
unsigned bits: 0 <= L <= C + p2 by induction (min(...) - m lies in [0, p2]).

Two forms that must agree: stereo_sgm_loop, a literal per-pixel loop for small images, and stereo_sgm, vectorised along the lines of
each direction. Both return (disp int16 [H, W], cost int32 [H, W]) in gms_stereo_bm_device's formats."""
import numpy as np

import stereo_bm_ref as B

DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
PARAM_NAMES = B.PARAM_NAMES + ("p1", "p2", "n_paths")   # the field order of gms_stereo_sgm_params
LIMIT = 65535


def make_params(p1=None, p2=None, n_paths=8, **bm):
    p = B.make_params(**bm)
    bs2 = p["block_size"] ** 2
    p["p1"] = 8 * bs2 if p1 is None else int(p1)
    p["p2"] = 32 * bs2 if p2 is None else int(p2)
    p["n_paths"] = int(n_paths)
    return p


def check_params(p, width, height):
    """What the library rejects with GMS_ERR_BAD_ARG (ValueError here)."""
    B.check_params(p, width, height)
    bad = []
    if not 0 <= p["p1"] <= p["p2"]:
        bad.append("0 <= p1 <= p2")
    if p["n_paths"] not in (4, 8):
        bad.append("n_paths 4 or 8")
    elif p["n_paths"] * (p["block_size"] ** 2 * 2 * p["pre_filter_cap"] + p["p2"]) > LIMIT:
        bad.append(f"n_paths * (block_size^2 * 2 * pre_filter_cap + p2) <= {LIMIT}")
    if bad:
        raise ValueError("StereoSGM: " + "; ".join(bad))


def _prepare(left, right, kw):
    p = make_params(**kw)
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    if left.ndim != 2 or right.shape != left.shape:
        raise ValueError("left and right: two 8-bit images of one size")
    H, W = left.shape
    check_params(p, W, H)
    return p, left, right, H, W


def cost_volume(left, right, p):
    """(C int32 [ny, wx, nd], tex int64 [ny, wx]) of the computed region: stereo_bm_ref.window_costs, k last."""
    sad, tex = B.window_costs(left, right, p)
    return np.ascontiguousarray(sad.transpose(1, 2, 0)).astype(np.int32), tex


# ---- the literal form ----------------------------------------------------------------------------------------------------------------
def path_costs_loop(C, dy, dx, p1, p2):
    """L of one direction, pixel by pixel along each line. C: nested lists [ny][wx][nd]."""
    ny, wx, nd = len(C), len(C[0]), len(C[0][0])
    L = [[None] * wx for _ in range(ny)]
    ys = range(ny) if dy >= 0 else range(ny - 1, -1, -1)     # an order in which the predecessor comes first
    xs = range(wx) if dx >= 0 else range(wx - 1, -1, -1)
    for y in ys:
        for x in xs:
            yp, xp = y - dy, x - dx
            c = C[y][x]
            if not (0 <= yp < ny and 0 <= xp < wx):
                L[y][x] = list(c)
                continue
            Lp = L[yp][xp]
            m = min(Lp)
            out = []
            for k in range(nd):
                t = min(Lp[k], m + p2)
                if k >= 1:
                    t = min(t, Lp[k - 1] + p1)
                if k + 1 < nd:
                    t = min(t, Lp[k + 1] + p1)
                out.append(c[k] + t - m)
            L[y][x] = out
    return L


def cost_volume_loop(left, right, p):
    """C and tex, literally (stereo_bm_ref.stereo_bm_loop's sums): nested lists [ny][wx][nd] and [ny][wx]."""
    H, W = left.shape
    nd, cap, w2 = p["num_disparities"], p["pre_filter_cap"], p["block_size"] // 2
    lofs, rofs, width1, _ = B.ranges(p, W)
    Lf = B.prefilter_xsobel_loop(left, cap).astype(np.int64).tolist()
    Rf = B.prefilter_xsobel_loop(right, cap).astype(np.int64).tolist()

    def clamp(v, lo, hi):
        return lo if v < lo else hi if v > hi else v

    C, T = [], []
    for y in range(w2, H - w2):
        crow, trow = [], []
        for x in range(min(width1, W - lofs)):
            sad, tex = [0] * nd, 0
            for dy in range(-w2, w2 + 1):
                lr, rr = Lf[y + dy], Rf[y + dy]
                for j in range(-w2, w2 + 1):
                    lv = lr[lofs + clamp(x + j, -lofs, W - 1 - lofs)]
                    rc = rofs + clamp(x + j, -rofs, W - nd - rofs)
                    tex += abs(lv - cap)
                    for k in range(nd):
                        sad[k] += abs(lv - rr[rc + k])
            crow.append(sad)
            trow.append(tex)
        C.append(crow)
        T.append(trow)
    return C, T


def stereo_sgm_loop(left, right, **kw):
    """Literal per-pixel form (small images only): (disp int16, cost int32)."""
    p, left, right, H, W = _prepare(left, right, kw)
    nd, w2 = p["num_disparities"], p["block_size"] // 2
    disp = np.full((H, W), B.filtered_value(p), np.int16)
    cost = np.full((H, W), -1, np.int32)
    lofs, _, _, none = B.ranges(p, W)
    if none:
        return disp, cost
    C, T = cost_volume_loop(left, right, p)
    ny, wx = len(C), len(C[0])
    S = [[[0] * nd for _ in range(wx)] for _ in range(ny)]
    for dy, dx in DIRECTIONS[:p["n_paths"]]:
        L = path_costs_loop(C, dy, dx, p["p1"], p["p2"])
        for y in range(ny):
            for x in range(wx):
                for k in range(nd):
                    S[y][x][k] += L[y][x][k]
    for y in range(ny):
        for x in range(wx):
            r = B.decide(S[y][x], T[y][x], p)
            if r is not None:
                disp[w2 + y, lofs + x], cost[w2 + y, lofs + x] = r
    if p["disp12_max_diff"] >= 0:
        B.validate_loop(disp, cost, p)
    B.roi_fill(disp, p, lofs)
    return disp, cost


# ---- the vectorised form -------------------------------------------------------------------------------------------------------------
def _step(Lp, p1, p2):
    """min(Lp[k], Lp[k - 1] + p1, Lp[k + 1] + p1, m + p2) - m over the last axis."""
    m = Lp.min(axis=-1, keepdims=True)
    t = np.minimum(Lp, m + p2)
    t[..., 1:] = np.minimum(t[..., 1:], Lp[..., :-1] + p1)
    t[..., :-1] = np.minimum(t[..., :-1], Lp[..., 1:] + p1)
    return t - m


def path_costs(C, dy, dx, p1, p2):
    """L [ny, wx, nd] of one direction: all lines of the direction advance together, one row (dy != 0) or one column at a time."""
    ny, wx, _ = C.shape
    L = C.copy()
    if dy == 0:
        xs = range(1, wx) if dx > 0 else range(wx - 2, -1, -1)
        for x in xs:
            L[:, x] += _step(L[:, x - dx], p1, p2)
        return L
    ys = range(1, ny) if dy > 0 else range(ny - 2, -1, -1)
    for y in ys:
        Lp = L[y - dy]
        if dx == 0:
            L[y] += _step(Lp, p1, p2)
        elif dx > 0:
            L[y, 1:] += _step(Lp[:-1], p1, p2)     # column 0 has no predecessor: L = C
        else:
            L[y, :-1] += _step(Lp[1:], p1, p2)     # nor has column wx - 1
    return L


def aggregate(C, p):
    """S [ny, wx, nd] int32: the sum of the path costs."""
    S = np.zeros_like(C)
    for dy, dx in DIRECTIONS[:p["n_paths"]]:
        S += path_costs(C, dy, dx, p["p1"], p["p2"])
    return S


def raw_maps(left, right, p):
    """The maps before the left-right check and the ROI fill: (disp int16, cost int32, the decisions with C, S and tex; None when
    nothing is computed)."""
    H, W = left.shape
    w2 = p["block_size"] // 2
    disp = np.full((H, W), B.filtered_value(p), np.int16)
    cost = np.full((H, W), -1, np.int32)
    lofs, _, _, none = B.ranges(p, W)
    if none:
        return disp, cost, None
    C, tex = cost_volume(left, right, p)
    S = aggregate(C, p)
    dec = B.decisions(S.transpose(2, 0, 1).astype(np.int64), tex, p)
    dec.update(C=C, S=S, tex=tex, sad=S.transpose(2, 0, 1))
    ok = dec["tex_ok"] & dec["uniq_ok"]
    wx = tex.shape[1]
    disp[w2:H - w2, lofs:lofs + wx] = np.where(ok, dec["disp"], B.filtered_value(p))
    cost[w2:H - w2, lofs:lofs + wx] = np.where(ok, dec["minsad"], -1)
    return disp, cost, dec


def stereo_sgm(left, right, **kw):
    """Vectorised form: (disp int16, cost int32), equal to stereo_sgm_loop."""
    p, left, right, H, W = _prepare(left, right, kw)
    disp, cost, dec = raw_maps(left, right, p)
    if dec is None:
        return disp, cost
    if p["disp12_max_diff"] >= 0:
        B.validate(disp, cost, p)
    B.roi_fill(disp, p, B.ranges(p, W)[0])
    return disp, cost


def stereo_match_sgm(left, right, **kw):
    """The reference's 8-bit form of the map: normalize(NORM_MINMAX, 0..255, CV_8U), then every 0 -> 255."""
    return B.normalize_u8(stereo_sgm(left, right, **kw)[0])
