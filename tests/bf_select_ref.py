"""numpy restatement of the reference's bruteForceMatch (FeatureMatchUtil.cpp:20-31): OpenCV's one-sided
cross-check (batchDistance with K = 1, crosscheck = true), MSVC std::sort by distance (logos_ref's restated introsort, carried to any
prefix length) and the ratio / size prune. What sfm-gms_amd/csrc/bf_select_kernels.hip must reproduce byte for byte."""
import os
import sys

import numpy as np

import logos_ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import gms_oracle  # noqa: E402

DMATCH_DTYPE = gms_oracle.DMATCH_DTYPE


def msvc_sort_prefix(d, ix, k):
    """MSVC std::sort on (d, ix) by d alone, as far as its first k places (any k); ranges that lie wholly at or beyond position k are
    left unsorted. The two sides of a partition are sorted with the same ideal, independently, so working the lower one first and
    the upper one later (if it reaches below k) gives std::sort's permutation."""
    stack = [(0, len(d), len(d))]
    while stack:
        f, l, ideal = stack.pop()
        while f < k:
            if l - f <= logos_ref._ISORT_MAX:
                logos_ref._insertion(d, ix, f, l)
                break
            if ideal <= 0:
                logos_ref._heap_sort(d, ix, f, l)
                break
            pf, pl = logos_ref._partition(d, ix, f, l)
            ideal = (ideal >> 1) + (ideal >> 2)
            if pl < k and l - pl > 1:
                stack.append((pl, l, ideal))
            l = pf


def cross_check(tidx, tdist, n_query):
    """OpenCV's merge of the backward matches: for train row i in order, `if (tdist[i] < dist[tidx[i]])` take it. Returns
    (q, t, d) of every query row that got one, q ascending."""
    dist = np.full(n_query, np.inf, np.float32)
    nidx = np.full(n_query, -1, np.int64)
    for i in range(len(tidx)):
        q = int(tidx[i])
        if tdist[i] < dist[q]:
            dist[q] = tdist[i]
            nidx[q] = i
    q = np.nonzero(nidx >= 0)[0]
    return q, nidx[q], dist[q]


def prune_count(d, coef, max_size):
    """K = min(max_size, #{d : !((double)d_min * coef < (double)d)}); d non-empty."""
    dm = float(np.min(d))
    n_ratio = int(np.count_nonzero(~(dm * float(coef) < d.astype(np.float64))))
    return min(int(max_size), n_ratio), n_ratio, np.float32(dm)


def select(q, t, d, coef=4.0, max_size=500):
    """candidates (q, t, d) in the cross-check's order -> (survivors as DMATCH_DTYPE, n_ratio, d_min)."""
    if len(d) == 0:
        return np.zeros(0, DMATCH_DTYPE), 0, np.float32(0)
    k, n_ratio, dm = prune_count(d, coef, max_size)
    dd = [np.float32(x) for x in d]
    ix = list(range(len(d)))
    msvc_sort_prefix(dd, ix, k)
    out = np.zeros(k, DMATCH_DTYPE)
    sel = np.asarray(ix[:k], np.int64)
    out["queryIdx"], out["trainIdx"], out["imgIdx"] = q[sel], t[sel], 0
    out["distance"] = np.asarray(dd[:k], np.float32)
    return out, n_ratio, dm


def candidates(desc1, desc2, hamming, cross=True):
    """The matcher stage: (q, t, d) in query order. desc1: query rows (frame_a), desc2: train rows (frame_b)."""
    if cross:
        back = gms_oracle.bf_match(desc2, desc1, hamming)  # every row of frame_b against frame_a: the backward direction only
        return cross_check(back["trainIdx"], back["distance"], len(desc1))
    fwd = gms_oracle.bf_match(desc1, desc2, hamming)
    return np.arange(len(desc1)), fwd["trainIdx"].astype(np.int64), fwd["distance"].astype(np.float32)


def bf_match_select(desc1, desc2, hamming, cross=True, coef=4.0, max_size=500):
    """(survivors, n_candidates, n_ratio, d_min); None survivors for an empty frame (GMS_ERR_DOMAIN)."""
    if len(desc1) == 0 or len(desc2) == 0:
        return None, 0, 0, np.float32(0)
    q, t, d = candidates(desc1, desc2, hamming, cross)
    out, n_ratio, dm = select(q, t, d, coef, max_size)
    return out, len(d), n_ratio, dm
