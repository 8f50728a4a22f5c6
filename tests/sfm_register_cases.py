"""Hand-made two-view records for the registration tests (no RANSAC): a known rigid scene seen by known cameras, every pair's record
and points written from the truth in a unit of its own. Pair i's points are the scene in camera frame_a divided by unit_i and its
translation is the true one divided by unit_i, so the cumulative scale is S_i = unit_i / unit_first analytically (unit_first: the unit
of the pair without a link that starts i's chain), whatever the median picks among equal ratios.

Keypoint perm_f[s] of frame f shows scene point s (a different permutation per frame, and frame f has 3 f keypoints that show
nothing), so that queryIdx and trainIdx cannot be mixed up unnoticed. case(name) -> dict(frame_off, pairs, matches, mask, points3d,
tv, root, min_links, expect = {pair: (status, n_links or None, S or None)}, truth = (R [n, 3, 3], t [n, 3]))."""
import functools

import numpy as np

GMS_OK, SKIPPED, NO_MODEL = 0, 1, -8
FILL = 777.0   # what the point slots behind a pair's points hold: read by mistake, it shows

PAIR_DTYPE = np.dtype([("frame_a", "<i4"), ("frame_b", "<i4"), ("m", "<i4"), ("reserved", "<i4"), ("match_off", "<i8")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
TWO_VIEW_DTYPE = np.dtype([("E", "<f8", (3, 3)), ("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("sum_sq_err1", "<f8"), ("sum_sq_err2", "<f8"),
                           ("n_finite", "<i8"), ("n_behind", "<i8"), ("n_points", "<i4"), ("n_ransac", "<i4"), ("ransac_iters", "<i4"),
                           ("n_pose", "<i4"), ("pose_which", "<i4"), ("n_triangulated", "<i4"), ("status", "<i4"), ("reserved", "<i4")])


class Scene:
    def __init__(self, seed, n_frames, n_points):
        rng = np.random.default_rng(seed)
        self.rng, self.n_frames, self.n_points = rng, n_frames, n_points
        self.X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(5, 9, n_points)], 1)
        self.R, self.t = np.zeros((n_frames, 3, 3)), np.zeros((n_frames, 3))
        for f in range(n_frames):
            a, b = 0.03 * f, -0.02 * f
            Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
            self.R[f] = Ry @ Rx
            self.t[f] = -self.R[f] @ np.array([0.4 * f, 0.05 * f * f, 0.1 * f])
        self.counts = np.array([n_points + 3 * f for f in range(n_frames)])
        self.perm = [rng.permutation(self.counts[f])[:n_points] for f in range(n_frames)]
        self.frame_off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)

    def cam(self, f, s):
        return self.X[s] @ self.R[f].T + self.t[f]


def assemble(scene, specs, root=0, min_links=8, gap=5, first_off=3):
    """specs: per pair dict(a, b, unit, pts = scene point indices, and optionally junk = every how many matches a zero-mask match is put in
    front, status, pad = spare capacity, edit = f(block) applied to the pair's dict of arrays before it is laid out)."""
    rng = scene.rng
    blocks = []
    for sp in specs:
        a, b, unit, pts = sp["a"], sp["b"], sp["unit"], np.asarray(sp["pts"], dtype=np.int64)
        q, t, mk, P = [], [], [], []
        for n, s in enumerate(pts):
            if sp.get("junk") and n % sp["junk"] == 0:
                q.append(int(rng.integers(scene.counts[a])))
                t.append(int(rng.integers(scene.counts[b])))
                mk.append(0)
            q.append(int(scene.perm[a][s]))
            t.append(int(scene.perm[b][s]))
            mk.append(1 + (n % 3) * 100)   # any non-zero byte is set
            P.append(scene.cam(a, s) / unit)
        Rrel = scene.R[b] @ scene.R[a].T
        blk = dict(a=a, b=b, q=np.array(q, np.int64), t=np.array(t, np.int64), mask=np.array(mk, np.uint8),
                   P=np.array(P, np.float64).reshape(-1, 3), R=Rrel, tr=(scene.t[b] - Rrel @ scene.t[a]) / unit,
                   status=sp.get("status", GMS_OK), pad=sp.get("pad", 2))
        if sp.get("edit"):
            sp["edit"](blk)
        blocks.append(blk)
    pairs = np.zeros(len(blocks), PAIR_DTYPE)
    tv = np.zeros(len(blocks), TWO_VIEW_DTYPE)
    off = first_off
    for i, blk in enumerate(blocks):
        n = len(blk["q"])
        pairs[i] = (blk["a"], blk["b"], n + blk["pad"], 0, off)
        tv[i]["R"], tv[i]["t"], tv[i]["status"] = blk["R"], blk["tr"], blk["status"]
        tv[i]["n_points"], tv[i]["n_triangulated"] = n, int((blk["mask"] != 0).sum())
        off += n + blk["pad"] + gap
    total = off
    matches = np.zeros(total, DMATCH_DTYPE)
    matches["queryIdx"], matches["trainIdx"] = -5, 10 ** 6   # slots no pair owns
    mask = np.full(total, 255, np.uint8)
    points = np.full((total, 3), FILL)
    for i, blk in enumerate(blocks):
        o, n = int(pairs[i]["match_off"]), len(blk["q"])
        matches["queryIdx"][o:o + n], matches["trainIdx"][o:o + n] = blk["q"], blk["t"]
        mask[o:o + n] = blk["mask"]
        points[o:o + len(blk["P"])] = blk["P"]
    return dict(frame_off=scene.frame_off, pairs=pairs, matches=matches, mask=mask, points3d=points, tv=tv, root=root, min_links=min_links,
                truth=(scene.R, scene.t))


def _scale_points(blk, rows, factor):
    blk["P"][rows] *= factor


def _chain_roles():
    """Both roles, an even number of links with two ratio values (the lower median is the smaller), zero mask bytes in between
    (rank != k), gapped offsets, and a reverse, a loop and a disconnected pair."""
    sc = Scene(11, 7, 60)

    def half_other(blk):   # pair 1's own points from row 20 on are 1.5 times nearer: 20 of its 40 links have 1.5 times the true ratio
        _scale_points(blk, np.arange(20, len(blk["P"])), 1 / 1.5)
    specs = [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 50), junk=3),
             dict(a=1, b=2, unit=2.5, pts=np.arange(10, 60), junk=4, edit=half_other),   # 40 links with pair 0, even
             dict(a=0, b=3, unit=0.7, pts=np.arange(5, 46), junk=2),                     # role 0: 41 links
             dict(a=2, b=1, unit=1.0, pts=np.arange(0, 30)),                             # reverse
             dict(a=1, b=3, unit=1.0, pts=np.arange(0, 30)),                             # both registered: a loop
             dict(a=5, b=6, unit=1.0, pts=np.arange(0, 30)),                             # neither registered
             dict(a=3, b=4, unit=3.0, pts=np.arange(0, 40), junk=5)]                     # hangs on the role-0 pair: 35 links
    c = assemble(sc, specs)
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 40, 2.5), 2: (GMS_OK, 41, 0.7), 3: (SKIPPED, 0, 0.0), 4: (SKIPPED, 0, 0.0),
                   5: (SKIPPED, 0, 0.0), 6: (GMS_OK, 35, 3.0)}
    return c


def _lowest_k_wins():
    """Every trainIdx of the link pair is named by two more inlier matches further down its list, whose points are three and five times
    too far: the slot is the lowest k, so every ratio is the true one; any other choice triples it or worse."""
    sc = Scene(12, 3, 40)

    def add_dups(blk):
        n = len(blk["q"])
        other = sc.rng.permutation(sc.counts[0])[:n]   # queried from other keypoints of frame 0
        blk["q"] = np.concatenate([blk["q"], other, other[::-1]])
        blk["t"] = np.concatenate([blk["t"], blk["t"], blk["t"]])
        blk["mask"] = np.concatenate([blk["mask"], np.full(2 * n, 1, np.uint8)])
        blk["P"] = np.concatenate([blk["P"], 3 * blk["P"], 5 * blk["P"]])
    specs = [dict(a=0, b=1, unit=1.0, pts=np.arange(40), edit=add_dups), dict(a=1, b=2, unit=0.4, pts=np.arange(4, 36), junk=3)]
    c = assemble(sc, specs)
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 32, 0.4)}
    return c


def _invalid_links_and_min_links():
    """Links with a non-finite point or z <= 0 on either side do not count; a pair with exactly min_links - 1 valid links fails and
    takes its two descendants with it; one with exactly min_links passes."""
    sc = Scene(13, 8, 40)

    def spoil_own(blk):   # pair (1, 2): of its 14 shared points, 6 of its own are spoilt: 8 valid links = min_links
        P = blk["P"]
        P[0, 0], P[1, 1], P[2, 2] = np.nan, np.inf, -np.inf
        P[3, 2], P[4, 2], P[5] = 0.0, -P[4, 2], -P[5]

    def spoil_linked(blk):   # pair (0, 3): of its 12 points, all shared with pair 0, 5 are spoilt: 7 valid links = min_links - 1
        P = blk["P"]
        P[0, 2], P[1, 0], P[2, 1], P[3, 2], P[4, 2] = np.nan, np.inf, -np.inf, 0.0, -1.0
    specs = [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 30)),
             dict(a=1, b=2, unit=2.0, pts=np.arange(16, 40), edit=spoil_own),      # shares 16..29 with pair 0
             dict(a=0, b=3, unit=1.5, pts=np.arange(0, 12), edit=spoil_linked),    # role 0 with pair 0: 7 valid links, fails
             dict(a=3, b=4, unit=0.5, pts=np.arange(0, 20)),                       # hangs on the failed pair
             dict(a=4, b=5, unit=1.0, pts=np.arange(0, 20)),                       # and has two descendants of its own,
             dict(a=4, b=6, unit=1.0, pts=np.arange(0, 20)),                       # which fail with it
             dict(a=2, b=7, unit=4.0, pts=np.arange(16, 40))]                      # hangs on the pair with exactly min_links: ok
    c = assemble(sc, specs)
    # (None: the count is not stated here -- spoilt points of the linked pair may or may not land in front of the camera)
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 8, 2.0), 2: (NO_MODEL, 7, 0.0), 3: (NO_MODEL, None, 0.0), 4: (NO_MODEL, None, 0.0),
                   5: (NO_MODEL, None, 0.0), 6: (GMS_OK, None, 4.0)}
    return c


def _upstream_failures():
    """A pair whose two-view status is GMS_ERR_NO_MODEL, an empty pair, and what hangs on them; root = 2."""
    sc = Scene(14, 8, 30)
    specs = [dict(a=2, b=0, unit=1.0, pts=np.arange(30), junk=4),
             dict(a=0, b=1, unit=0.25, pts=np.arange(30), junk=7),
             dict(a=1, b=3, unit=1.0, pts=np.arange(30), status=NO_MODEL),
             dict(a=3, b=4, unit=1.0, pts=np.arange(30)),
             dict(a=2, b=5, unit=2.0, pts=np.arange(0)),       # empty: nothing triangulated
             dict(a=5, b=6, unit=1.0, pts=np.arange(30)),
             dict(a=2, b=7, unit=8.0, pts=np.arange(3, 30))]   # role 0
    c = assemble(sc, specs, root=2)
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 30, 0.25), 2: (NO_MODEL, 0, 0.0), 3: (NO_MODEL, 0, 0.0), 4: (NO_MODEL, 0, 0.0),
                   5: (NO_MODEL, 0, 0.0), 6: (GMS_OK, 27, 8.0)}
    return c


def _many_links():
    """One pair with 5000 links: past one pass of any 1024-lane gather, and past one tile of the ordered compaction."""
    sc = Scene(15, 3, 5200)
    specs = [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 5100), junk=11), dict(a=1, b=2, unit=1.75, pts=np.arange(100, 5200), junk=13)]
    c = assemble(sc, specs)
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 5000, 1.75)}
    return c


CASES = {"chain_roles": _chain_roles, "lowest_k_wins": _lowest_k_wins, "invalid_links_and_min_links": _invalid_links_and_min_links,
         "upstream_failures": _upstream_failures, "many_links": _many_links}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def truth_views(c):
    """The true views in the root's frame and the first pair's unit (unit 1 in every case): R_f R_root^T, t_f - R t_root."""
    R, t = c["truth"]
    r = c["root"]
    out = []
    for f in range(len(R)):
        Rf = R[f] @ R[r].T
        out.append((Rf, t[f] - Rf @ t[r]))
    return out
