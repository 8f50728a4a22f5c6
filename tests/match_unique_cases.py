"""Hand-made match lists for the one-to-one rule (tests/match_unique_ref.py). case(name) -> dict(frame_off, pairs,
matches, mask, tv, total_m, expect = {pair: the k that are kept} where the case states them). A row is (queryIdx, trainIdx, distance)
or (queryIdx, trainIdx, distance, mask byte). Slots that no pair owns hold indices outside every frame and a mask byte of 255."""
import functools

import numpy as np

from sfm_register_cases import DMATCH_DTYPE, PAIR_DTYPE, TWO_VIEW_DTYPE

GMS_OK, NO_MODEL = 0, -8
NAN, INF = float("nan"), float("inf")


def build(counts, specs, gap=3, first_off=2, with_mask=True, with_tv=True):
    """counts: keypoints per frame; specs: per pair dict(a, b, rows, and optionally pad = slots behind the rows inside m (default 0),
    status, n_points (default: the rows), off = the match_off to write instead of the next free one)."""
    frame_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pairs, tv = np.zeros(len(specs), PAIR_DTYPE), np.zeros(len(specs), TWO_VIEW_DTYPE)
    off, blocks = first_off, []
    for i, sp in enumerate(specs):
        n, pad = len(sp["rows"]), sp.get("pad", 0)
        pairs[i] = (sp["a"], sp["b"], n + pad, 0, off)
        tv[i]["status"], tv[i]["n_points"], tv[i]["n_triangulated"] = sp.get("status", GMS_OK), sp.get("n_points", n), n
        blocks.append(off)
        off += n + pad + gap
    total = off
    matches = np.zeros(total, DMATCH_DTYPE)
    matches["queryIdx"], matches["trainIdx"], matches["distance"] = -5, 10 ** 6, 0.5
    mask = np.full(total, 255, np.uint8)
    for o, sp in zip(blocks, specs):
        for k, row in enumerate(sp["rows"]):
            matches[o + k] = (row[0], row[1], 0, row[2])
            mask[o + k] = row[3] if len(row) > 3 else 1 + 100 * (k % 3)
        for k in range(len(sp["rows"]), len(sp["rows"]) + sp.get("pad", 0)):   # pad slots: a best match, were it read as one
            matches[o + k] = (0, 0, 0, 0.0)
    return dict(frame_off=frame_off, pairs=pairs, matches=matches, mask=mask if with_mask else None, tv=tv if with_tv else None, total_m=total)


def _equal_distances():
    """Three rivals for train 4 at one distance (the lowest k wins), two for query 2 likewise, and one match nobody disputes."""
    c = build([8, 9], [dict(a=0, b=1, rows=[(5, 7, 2.0), (1, 4, 1.5), (2, 4, 1.5), (3, 4, 1.5), (6, 1, 1.0), (6, 2, 1.0), (0, 0, 9.0)])])
    c["expect"] = {0: [0, 1, 4, 6]}
    return c


def _signed_zero():
    """+0 beside -0 on one train keypoint: both are ord 0, the lowest k wins -- once with -0 first, once with +0 first; and a
    denormal distance, which is more than either."""
    c = build([6, 6], [dict(a=0, b=1, rows=[(0, 1, -0.0), (1, 1, 0.0), (2, 3, 0.0), (3, 3, -0.0), (4, 5, 1e-45), (5, 5, -0.0)])])
    c["expect"] = {0: [0, 2, 5]}
    return c


def _unordered_last():
    """NaN, -1, +inf and -inf come behind every finite distance and are ordered by k among themselves."""
    rows = [(0, 0, NAN), (1, 0, 3.0e38),              # the huge finite distance wins over the NaN before it
            (2, 1, INF), (3, 1, -1.0), (4, 1, NAN),   # all last: k = 2 wins
            (5, 2, -INF), (6, 2, -1.0),                # k = 5
            (7, 3, -1.0), (8, 3, 0.0)]                 # +0 beats the negative before it
    c = build([9, 4], [dict(a=0, b=1, rows=rows)])
    c["expect"] = {0: [1, 2, 5, 8]}
    return c


def _best_not_live():
    """The best match of train 2 is masked out, that of train 3 names a query keypoint outside frame_a, that of train 4 a negative one,
    and the best of query 6 names a train keypoint at the frame's count: none of them competes."""
    rows = [(0, 2, 0.1, 0), (1, 2, 0.7), (2, 3, 0.1), (10, 3, 0.05), (3, 4, 0.9), (-1, 4, 0.2), (6, 7, 0.1), (6, 5, 0.4)]
    c = build([10, 7], [dict(a=0, b=1, rows=rows)])
    c["expect"] = {0: [1, 2, 4, 7]}
    return c


def _not_a_matching():
    """k = 0 (q0, t0, 2.0) loses train 0 to k = 1 (q1, t0, 1.0), which loses query 1 to k = 2 (q1, t1, 0.5): k = 0 is not kept although
    nothing kept touches q0 or t0. A maximum matching would keep two; the rule keeps one."""
    c = build([3, 3], [dict(a=0, b=1, rows=[(0, 0, 2.0), (1, 0, 1.0), (1, 1, 0.5)])])
    c["expect"] = {0: [2]}
    return c


def _two_view_cuts():
    """Pair 0 has no two-view model: nothing is live. Pair 1 has n_points = 3 of 5 rows: its best match for train 1, at k = 4, is past
    the count. Pair 2 has a negative n_points. Pair 3 has one past m, clamped to m: its two pad slots (0, 0, distance 0) are live, and
    the first of them wins query 0 and train 0."""
    specs = [dict(a=0, b=1, rows=[(0, 0, 1.0), (1, 1, 1.0)], status=NO_MODEL),
             dict(a=0, b=1, rows=[(0, 0, 1.0), (1, 1, 2.0), (2, 2, 1.0), (3, 2, 0.5), (4, 1, 0.1)], n_points=3),
             dict(a=1, b=0, rows=[(0, 0, 1.0)], n_points=-4),
             dict(a=1, b=0, rows=[(0, 0, 1.0), (1, 0, 0.5), (2, 2, 3.0)], n_points=99, pad=2)]
    c = build([5, 5], specs)
    c["expect"] = {0: [], 1: [0, 1, 2], 2: [], 3: [2, 3]}
    return c


def _no_mask_no_tv():
    """The same lists without a mask and without two-view records: every slot below m counts, the pad slots (0, 0, distance 0)
    included -- the first of them wins query 0 and train 0."""
    specs = [dict(a=0, b=1, rows=[(0, 0, 1.0, 0), (1, 1, 2.0, 0), (2, 1, 1.0, 0)], status=NO_MODEL, pad=2)]
    c = build([5, 5], specs, with_mask=False, with_tv=False)
    c["expect"] = {0: [2, 3]}
    return c


def _misfits():
    """Records that do not fit the arrays beside one that does: frame_a = n_frames, frame_b = -1, m = -3, match_off = -1, a range that
    ends past total_m, a match_off whose sum with m does not fit 64 bits. keep 0, counts {0, 0}, nothing read outside."""
    rows = [(0, 0, 1.0), (1, 0, 0.5), (2, 2, 3.0)]
    c = build([4, 4], [dict(a=0, b=1, rows=rows) for _ in range(7)])
    p = c["pairs"]
    p["frame_a"][1] = 2
    p["frame_b"][2] = -1
    p["m"][3] = -3
    p["match_off"][4] = -1
    p["match_off"][5] = c["total_m"] - 2
    p["match_off"][6], p["m"][6] = 2 ** 63 - 2, 5
    c["expect"] = {0: [1, 2]}
    c["host_refuses"] = True   # the one-shot refuses these records, as gms_sfm_register does
    return c


def _two_chunks():
    """One pair of 600 matches -- more than two chunks of 256 --, the rivals for train 7 at k = 0 and k = 599 with equal distances; every
    other match has a train keypoint of its own."""
    rows = [(k, 7 if k in (0, 599) else 8 + k, 1.0 if k in (0, 599) else 0.25 + (k % 7)) for k in range(600)]
    c = build([600, 700], [dict(a=0, b=1, rows=rows)])
    c["expect"] = {0: list(range(599))}
    return c


def _one_train_300():
    """300 live matches of one pair all name train keypoint 11: the contended word. The least distance sits at k = 217, and k = 40
    and k = 260 tie for second."""
    d = 5.0 + (np.arange(300) * 37 % 101)
    d[217], d[40], d[260] = 0.5, 1.0, 1.0
    c = build([300, 20], [dict(a=0, b=1, rows=[(k, 11, float(d[k])) for k in range(300)])])
    c["expect"] = {0: [217]}
    return c


def _star():
    """(0, 1), (0, 2), (0, 3): the same query keypoints of frame 0 in all three pairs, each pair with two rivals per query and a
    different winner. A query table shared between the pairs keeps one winner per keypoint instead of one per pair."""
    def rows(first_wins):
        out = []
        for q in range(40):
            d = (1.0, 2.0) if (q % 3 == first_wins) else (2.0, 1.0)
            out += [(q, 2 * q, d[0]), (q, 2 * q + 1, d[1])]
        return out
    c = build([40, 80, 80, 80], [dict(a=0, b=f + 1, rows=rows(f)) for f in range(3)])
    c["expect"] = {f: [2 * q + (0 if q % 3 == f else 1) for q in range(40)] for f in range(3)}
    return c


def _shared_trains():
    """(0, 1) twice and (0, 2), (1, 2), with different lists: per pair, two rivals for every train keypoint and a winner that differs
    from pair to pair. A train table shared by frame_b keeps one winner per keypoint of frame 1 and of frame 2."""
    def rows(shift):
        out = []
        for t in range(30):
            d = (1.0, 2.0) if ((t + shift) % 2 == 0) else (2.0, 1.0)
            out += [(2 * t, t, d[0]), (2 * t + 1, t, d[1])]
        return out
    specs = [dict(a=0, b=1, rows=rows(0)), dict(a=0, b=1, rows=rows(1)), dict(a=0, b=2, rows=rows(0)), dict(a=1, b=2, rows=rows(1))]
    c = build([60, 60, 30], specs)
    c["expect"] = {i: [2 * t + (0 if (t + s) % 2 == 0 else 1) for t in range(30)] for i, s in enumerate((0, 1, 0, 1))}
    return c


def _chain_roles_of_frame_1():
    """(0, 1) then (1, 2): frame 1 is train in one pair and query in the next, with rivals on it in both roles."""
    p0 = [(q, q // 2, 1.0 + (q % 2)) for q in range(40)]                 # two queries per keypoint of frame 1; the even one wins
    p1 = [(k // 2, k, 2.0 - (k % 2)) for k in range(40)]                 # two trains per keypoint of frame 1; the odd one wins
    c = build([40, 20, 40], [dict(a=0, b=1, rows=p0), dict(a=1, b=2, rows=p1)])
    c["expect"] = {0: list(range(0, 40, 2)), 1: list(range(1, 40, 2))}
    return c


def _empty_pair():
    """A pair with m = 0 between two others."""
    c = build([4, 4], [dict(a=0, b=1, rows=[(0, 0, 1.0), (1, 0, 0.5)]), dict(a=0, b=1, rows=[]), dict(a=1, b=0, rows=[(2, 2, 1.0)])])
    c["expect"] = {0: [1], 1: [], 2: [0]}
    return c


def _no_pairs():
    c = build([4, 4], [])
    c["expect"] = {}
    return c


RULE_CASES = {"equal_distances": _equal_distances, "signed_zero": _signed_zero, "unordered_last": _unordered_last,
              "best_not_live": _best_not_live, "not_a_matching": _not_a_matching, "two_view_cuts": _two_view_cuts,
              "no_mask_no_tv": _no_mask_no_tv, "misfits": _misfits}
SHAPE_CASES = {"two_chunks": _two_chunks, "one_train_300": _one_train_300, "star": _star, "shared_trains": _shared_trains,
               "chain_roles_of_frame_1": _chain_roles_of_frame_1, "empty_pair": _empty_pair, "no_pairs": _no_pairs}
CASES = {**RULE_CASES, **SHAPE_CASES}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
