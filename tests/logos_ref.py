"""An independent numpy restatement of cv::xfeatures2d::matchLOGOS, as the reference DLL computes it (LOGOS).

Everything is float32 arithmetic in the DLL's order, with the DLL's float <-> double round trips spelled out. The two
elementary functions it takes from the CRT, logf and acosf, are evaluated in float64 and rounded to float32.

matchLOGOS(kp1, kp2, nn1, nn2) -> int32 array (m, 2) of (queryIdx, trainIdx); the DLL's DMatch records carry imgIdx -1 and
distance 0 besides.
"""
import numpy as np

F = np.float32
PI = np.pi                      # the double constant of the DLL
TWO_PI = 2.0 * np.pi
THRESH = F(0.1)                 # intra / inter orientation and scale thresholds, GLOBALORITHRESH
NUM = 5                         # NUM1 == NUM2
LB = F(-np.pi)                  # float(-pi)
BINSIZE = F(THRESH / F(3.0))
BINNUMBER = int(np.ceil(TWO_PI / float(BINSIZE)))   # 189


def _logf(x):
    return np.log(np.asarray(x, np.float64)).astype(F)


def _acosf(x):
    return np.arccos(np.asarray(x, np.float64)).astype(F)


def points(kp, nn):
    """(x, y, orientation, log scale input, label) per keypoint, orientation = (float)(angle * pi / 180.0) in double."""
    kp = np.asarray(kp, np.float32).reshape(-1, 4)   # x, y, size, angle
    ori = ((kp[:, 3].astype(np.float64) * PI) / 180.0).astype(F)
    return kp[:, 0].copy(), kp[:, 1].copy(), ori, kp[:, 2].copy(), np.asarray(nn, np.int32)


# ---- Point::nearestNeighbours: squared distances in index order (self left out), std::sort by distance alone, first NUM ----
# The DLL sorts with MSVC's std::sort (RVA 0x52d60, predicate RVA 0x53540: a.d < b.d). It is not stable, so which of several
# points at the same distance make the first NUM is the order that sort leaves them in. That order is restated below as the
# DLL runs it: introsort with ranges of at most 32 finished by insertion sort, a median of three (of nine above 40 elements)
# and a three-way partition around it, 1.5 log2 n partition levels before heap sort. Only the ranges that reach into the first
# NUM places are worked on: the others cannot move an element into them.
_ISORT_MAX = 32


def _insertion(d, ix, f, l):
    for nx in range(f + 1, l):
        vd, vi = d[nx], ix[nx]
        if vd < d[f]:
            d[f + 1:nx + 1] = d[f:nx]; ix[f + 1:nx + 1] = ix[f:nx]
            d[f], ix[f] = vd, vi
        else:
            h = nx
            while vd < d[h - 1]:
                d[h], ix[h] = d[h - 1], ix[h - 1]
                h -= 1
            d[h], ix[h] = vd, vi


def _swap(d, ix, a, b):
    d[a], d[b] = d[b], d[a]
    ix[a], ix[b] = ix[b], ix[a]


def _med3(d, ix, f, m, l):
    if d[m] < d[f]: _swap(d, ix, m, f)
    if d[l] < d[m]:
        _swap(d, ix, l, m)
        if d[m] < d[f]: _swap(d, ix, m, f)


def _partition(d, ix, f, l):
    m = f + ((l - f) >> 1)
    last = l - 1
    cnt = last - f
    if 40 < cnt:
        st = (cnt + 1) >> 3
        tw = st << 1
        _med3(d, ix, f, f + st, f + tw)
        _med3(d, ix, m - st, m, m + st)
        _med3(d, ix, last - tw, last - st, last)
        _med3(d, ix, f + st, m, last - st)
    else:
        _med3(d, ix, f, m, last)
    pf, pl = m, m + 1
    while f < pf and not (d[pf - 1] < d[pf]) and not (d[pf] < d[pf - 1]):
        pf -= 1
    while pl < l and not (d[pl] < d[pf]) and not (d[pf] < d[pl]):
        pl += 1
    gf, gl = pl, pf
    while True:
        while gf < l:
            if d[pf] < d[gf]:
                pass
            elif d[gf] < d[pf]:
                break
            elif pl != gf:
                _swap(d, ix, pl, gf); pl += 1
            else:
                pl += 1
            gf += 1
        while f < gl:
            if d[gl - 1] < d[pf]:
                pass
            elif d[pf] < d[gl - 1]:
                break
            else:
                pf -= 1
                if pf != gl - 1:
                    _swap(d, ix, pf, gl - 1)
            gl -= 1
        if gl == f and gf == l:
            return pf, pl
        if gl == f:
            if pl != gf:
                _swap(d, ix, pf, pl)
            pl += 1
            _swap(d, ix, pf, gf)
            pf += 1
            gf += 1
        elif gf == l:
            gl -= 1; pf -= 1
            if gl != pf:
                _swap(d, ix, gl, pf)
            pl -= 1
            _swap(d, ix, pf, pl)
        else:
            gl -= 1
            _swap(d, ix, gf, gl)
            gf += 1


def _sift_down(d, ix, f, hole, bottom, vd, vi):
    # _Pop_heap_hole_by_index + _Push_heap_by_index (max-heap under a.d < b.d)
    top = hole
    idx = hole
    max_seq_non_leaf = (bottom - 1) >> 1
    while idx < max_seq_non_leaf:
        idx = 2 * idx + 2
        if d[f + idx] < d[f + idx - 1]:
            idx -= 1
        d[f + hole], ix[f + hole] = d[f + idx], ix[f + idx]
        hole = idx
    if idx == max_seq_non_leaf and bottom % 2 == 0:
        d[f + hole], ix[f + hole] = d[f + bottom - 1], ix[f + bottom - 1]
        hole = bottom - 1
    idx = (hole - 1) >> 1
    while top < hole and d[f + idx] < vd:
        d[f + hole], ix[f + hole] = d[f + idx], ix[f + idx]
        hole = idx
        idx = (hole - 1) >> 1
    d[f + hole], ix[f + hole] = vd, vi


def _heap_sort(d, ix, f, l):
    n = l - f
    for hole in range((n >> 1) - 1, -1, -1):
        _sift_down(d, ix, f, hole, n, d[f + hole], ix[f + hole])
    for last in range(n - 1, 0, -1):
        vd, vi = d[f + last], ix[f + last]
        d[f + last], ix[f + last] = d[f], ix[f]
        _sift_down(d, ix, f, 0, last, vd, vi)


def msvc_sort_head(d, ix, k):
    """MSVC std::sort on (d, ix) by d alone, as far as its first k places (k <= 32); ranges that lie wholly at or beyond
    position k are left unsorted."""
    f, l, ideal = 0, len(d), len(d)
    while True:
        if f >= k:
            return
        if l - f <= _ISORT_MAX:
            _insertion(d, ix, f, l)
            return
        if ideal <= 0:
            _heap_sort(d, ix, f, l)
            return
        pf, pl = _partition(d, ix, f, l)
        ideal = (ideal >> 1) + (ideal >> 2)
        if pl < k:       # both outer parts can reach below k: the lower one then lies inside [0, k), k <= 32
            _insertion(d, ix, f, pf)
            f = pl
        else:
            l = pf


def neighbours(x, y, k=NUM, chunk=1024):
    """The k nearest other points of each point in the DLL's order (msvc_sort_head where distances tie across the k-th
    place); -1 pads when the frame has fewer than k + 1 points (the DLL reads past its list there)."""
    n = len(x)
    out = np.full((n, k), -1, np.int32)
    kk = min(k, n - 1)
    if kk <= 0:
        return out
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        dx = x[s:e, None] - x[None, :]
        dy = y[s:e, None] - y[None, :]
        d = (dx * dx + dy * dy).astype(F)
        d[np.arange(e - s), np.arange(s, e)] = np.inf
        order = np.argsort(d, axis=1, kind="stable")
        dk = np.take_along_axis(d, order[:, kk - 1:kk], 1)
        out[s:e, :kk] = order[:, :kk]
        tie = (d <= dk).sum(1) > kk
        for r in np.nonzero(tie)[0]:
            i = s + r
            others = np.concatenate((np.arange(i), np.arange(i + 1, n)))
            dl = [float(v) for v in d[r, others]]
            il = [int(v) for v in others]
            msvc_sort_head(dl, il, kk)
            out[i, :kk] = il[:kk]
    return out


MAX_ANGLE_DEG = F(3600.0)


def kp_ok(x, y, angle):
    """The keypoint domain of every LOGOS entry point (include/gms.h; logos_core.h kp_ok): x, y and angle finite and
    |angle| <= 3600. Elementwise on float32 arrays."""
    x, y, angle = (np.asarray(v, F) for v in (x, y, angle))
    return np.isfinite(x) & np.isfinite(y) & np.isfinite(angle) & (np.abs(angle) <= MAX_ANGLE_DEG)


def _wrap_pair(d):
    """relOri of a pair: d = o1 - o2 in float, brought into [-pi, pi] through double the way the DLL does. match() admits only
    keypoints inside kp_ok, which bounds either loop to 21 rounds: beyond 2^27 rad a float no longer changes when 2 pi is taken
    off it, and the DLL's loop -- and this one -- would never end."""
    d = d.astype(F)
    fin = np.isfinite(d)           # inf / NaN: outside the domain; left as they are
    while True:
        m = (d.astype(np.float64) > PI) & fin
        if not m.any():
            break
        d[m] = (d[m].astype(np.float64) - TWO_PI).astype(F)
    while True:
        m = (-PI > d.astype(np.float64)) & fin
        if not m.any():
            break
        d[m] = (d[m].astype(np.float64) + TWO_PI).astype(F)
    return d


def _angle_dist(a, b):
    """min(|2 pi - t|, t) with t = |a - b| reduced below 2 pi (float, through double)."""
    t = np.abs((a - b).astype(F))
    fin = np.isfinite(t)
    while True:
        m = (t.astype(np.float64) > TWO_PI) & fin
        if not m.any():
            break
        t[m] = (t[m].astype(np.float64) - TWO_PI).astype(F)
    t = np.abs(t)
    u = np.abs((TWO_PI - t.astype(np.float64)).astype(F))
    return np.where(u < t, u, t)


def local_support(P1, P2, nb1, nb2, ci, cj):
    """Support count of each candidate (ci[c], cj[c]): neighbour pairs (a, b), a among ci's neighbours and b among cj's with
    equal labels, consistent with the candidate in all four measures."""
    x1, y1, o1, s1, l1 = P1
    x2, y2, o2, s2, l2 = P2
    ls1, ls2 = _logf(s1), _logf(s2)
    rel_o = _wrap_pair(o1[ci] - o2[cj])
    rel_s = (ls1[ci] - ls2[cj]).astype(F)
    support = np.zeros(len(ci), np.int32)
    for u in range(nb1.shape[1]):
        a = nb1[ci, u]
        for v in range(nb2.shape[1]):
            b = nb2[cj, v]
            ok = (a >= 0) & (b >= 0)
            ok[ok] = l1[a[ok]] == l2[b[ok]]
            if not ok.any():
                continue
            c = np.nonzero(ok)[0]
            pa, pb, qi, qj = a[c], b[c], ci[c], cj[c]
            nrel_o = _wrap_pair(o1[pa] - o2[pb])
            nrel_s = (ls1[pa] - ls2[pb]).astype(F)
            intra_o = _angle_dist(rel_o[c], nrel_o)
            intra_s = np.abs((rel_s[c] - nrel_s).astype(F))
            dx1 = (x1[qi] - x1[pa]).astype(F)
            dy1 = (y1[qi] - y1[pa]).astype(F)
            dx2 = (x2[qj] - x2[pb]).astype(F)
            dy2 = (y2[qj] - y2[pb]).astype(F)
            cross = (dy2 * dx1 - dy1 * dx2).astype(F)
            n1 = np.sqrt((dy1 * dy1 + dx1 * dx1).astype(F))
            n2 = np.sqrt((dy2 * dy2 + dx2 * dx2).astype(F))
            with np.errstate(invalid="ignore", divide="ignore"):
                dot = ((dy2 * dy1 + dx2 * dx1).astype(F) / (n2 * n1).astype(F)).astype(F)
                cl = np.where(F(-1.0) > dot, F(-1.0), dot)
                cl = np.where(cl > F(1.0), F(1.0), cl)
                sign = ((cross > 0).astype(np.int32) - (F(0) > cross).astype(np.int32)).astype(F)
                ang = (_acosf(cl) * sign).astype(F)
                lsc = (_logf(n1) - _logf(n2)).astype(F)
            inter_o = _angle_dist(rel_o[c], ang)
            inter_s = np.abs((rel_s[c] - lsc).astype(F))
            good = (THRESH > intra_o) & (THRESH > intra_s) & (THRESH > inter_o) & (THRESH > inter_s)
            np.add.at(support, c[good], 1)
    return support, rel_o


def peak_orientation(rel_o):
    """Histogram of the supported candidates' relOri, smoothed over three circular bins, first maximum; the bin's centre."""
    t = ((rel_o - LB).astype(F) / BINSIZE).astype(F)
    b = np.trunc(t).astype(np.int64)
    b = b - (b.astype(F) > t)
    b = np.where((b < 0) | (b >= BINNUMBER), BINNUMBER - 1, b)
    bins = np.bincount(b, minlength=BINNUMBER).astype(np.int64)
    sm = bins + np.roll(bins, 1) + np.roll(bins, -1)
    peak = int(np.argmax(sm))
    return peak, F(F(F(peak) * BINSIZE) + LB) + F(BINSIZE * F(0.5))


def candidates(l1, l2):
    """Every (i, j) with equal labels, i ascending, then j ascending."""
    order = np.argsort(l2, kind="stable")
    sl = l2[order]
    lo = np.searchsorted(sl, l1, "left")
    hi = np.searchsorted(sl, l1, "right")
    cnt = hi - lo
    ci = np.repeat(np.arange(len(l1)), cnt)
    start = np.repeat(lo - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt)
    cj = order[start + np.arange(len(ci))] if len(ci) else np.zeros(0, np.int64)
    return ci.astype(np.int64), np.asarray(cj, np.int64)


def match(kp1, kp2, nn1, nn2, detail=False):
    """matchLOGOS: (m, 2) int32 (queryIdx, trainIdx). With detail, also (n candidates, n supported, peak bin). ValueError for a
    keypoint outside the domain (kp_ok), where the DLL does not terminate."""
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 4)
    kp2 = np.asarray(kp2, np.float32).reshape(-1, 4)
    for kp in (kp1, kp2):
        if not kp_ok(kp[:, 0], kp[:, 1], kp[:, 3]).all():
            raise ValueError("matchLOGOS: a keypoint outside the domain (x, y, angle finite, |angle| <= 3600)")
    empty = np.zeros((0, 2), np.int32)
    if len(kp1) == 0 or len(kp2) == 0:
        return (empty, (0, 0, -1)) if detail else empty
    P1, P2 = points(kp1, nn1), points(kp2, nn2)
    nb1, nb2 = neighbours(P1[0], P1[1]), neighbours(P2[0], P2[1])
    ci, cj = candidates(P1[4], P2[4])
    support, rel_o = local_support(P1, P2, nb1, nb2, ci, cj)
    keep = support > 0
    ci, cj, rel_o = ci[keep], cj[keep], rel_o[keep]
    if len(ci) == 0:
        res = empty
        peak = -1          # include/gms.h: no candidate had support (the DLL's histogram is empty then; nothing survives)
    else:
        peak, g = peak_orientation(rel_o)
        glob = THRESH.astype(np.float64) > np.abs(rel_o.astype(np.float64) - np.float64(g))
        res = np.stack([ci[glob], cj[glob]], 1).astype(np.int32)
    return (res, (int(len(support)), int(keep.sum()), peak)) if detail else res
