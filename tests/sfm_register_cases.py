"""Hand-made two-view records for the registration tests (no RANSAC): a known rigid scene seen by known cameras, every pair's record
and points written from the truth in a unit of its own. Pair i's points are the scene in camera frame_a divided by unit_i and its
translation is the true one divided by unit_i, so the cumulative scale is S_i = unit_i / unit_first analytically (unit_first: the unit
of the pair without a link that starts i's chain), whatever the median picks among equal ratios.

Keypoint perm_f[s] of frame f shows scene point s (a different permutation per frame, and frame f has 3 f keypoints that show
nothing), so that queryIdx and trainIdx cannot be mixed up unnoticed. case(name) -> dict(frame_off, pairs, matches, mask, points3d,
tv, root, min_links, expect = {pair: (status, n_links or None, S or None)}, truth = (R [n, 3, 3], t [n, 3])). A case may add
cloud_cap (the capacity to run it with), and -- the cases named in UNFIT -- plan (the plan to walk instead of the pair list's own),
host_pairs (the sane records the host sizes its buffers by, where `pairs` are what the device reads) and total_m (the arrays'
length)."""
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
    """gentle: 0.002 rad and (0.01, 0.002, 0.003) of motion per frame instead of 0.03 rad and 0.4 -- the scene stays in front of
    hundreds of cameras, where the default motion puts it behind them after about 60. spare: per frame the number of keypoints that
    show nothing (default 3 f)."""

    def __init__(self, seed, n_frames, n_points, gentle=False, spare=None):
        rng = np.random.default_rng(seed)
        self.rng, self.n_frames, self.n_points = rng, n_frames, n_points
        self.X = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(5, 9, n_points)], 1)
        self.R, self.t = np.zeros((n_frames, 3, 3)), np.zeros((n_frames, 3))
        for f in range(n_frames):
            a, b = (0.002 * f, -0.001 * f) if gentle else (0.03 * f, -0.02 * f)
            Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
            self.R[f] = Ry @ Rx
            self.t[f] = -self.R[f] @ (np.array([0.01 * f, 0.002 * f, 0.003 * f]) if gentle else np.array([0.4 * f, 0.05 * f * f, 0.1 * f]))
        self.counts = np.array([n_points + (3 * f if spare is None else int(spare[f])) for f in range(n_frames)])
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


def _unit(f):
    return 1.0 + 0.25 * (f % 5)


def _chain_300():
    """301 frames, pair f = (f, f + 1): every link is the previous pair and every frame_a the frame it registered, so the walk of
    sfr_compose_kernel takes all of it from its registers, across the boundary of its 256 staged pairs. 24 tracks of 301 keypoints."""
    sc = Scene(31, 301, 24, gentle=True)
    c = assemble(sc, [dict(a=f, b=f + 1, unit=_unit(f), pts=np.arange(24)) for f in range(300)])
    c["expect"] = {f: (GMS_OK, 24 if f else 0, _unit(f)) for f in range(300)}
    return c


def _star_300():
    """The same frames, pair f = (0, f + 1): every link is pair 0 in role 0, so from pair 2 on its outcome and scale are read from
    global memory, and the view of frame_a is the root's."""
    sc = Scene(32, 301, 24, gentle=True)
    c = assemble(sc, [dict(a=0, b=f + 1, unit=_unit(f), pts=np.arange(24)) for f in range(300)])
    c["expect"] = {f: (GMS_OK, 24 if f else 0, _unit(f)) for f in range(300)}
    return c


def _two_branches_300():
    """Two chains out of frame 0, taken in turn: pairs (0, 1), (0, 2), then pair i = (i - 1, i + 1). The link of pair i is pair i - 2
    and frame_a is never the frame registered last: outcome, scale and view all come from global memory. Pair 256 -- the first of
    the second staging pass -- has no two-view model: its branch fails from there on, the other goes on."""
    sc = Scene(33, 301, 24, gentle=True)
    specs = [dict(a=0 if i < 2 else i - 1, b=i + 1, unit=_unit(i), pts=np.arange(24)) for i in range(300)]
    specs[256]["status"] = NO_MODEL
    c = assemble(sc, specs)
    # (pairs 256 and 258 measure no link: one side has no two-view result; from 260 on both sides have one)
    c["expect"] = {i: (GMS_OK, 24 if i else 0, _unit(i)) if i < 256 or i % 2 else (NO_MODEL, 0 if i < 260 else 24, 0.0) for i in range(300)}
    return c


def _tiles_past_256():
    """Three frames, the root with 1,100,000 spare keypoints: 1,100,185 keypoints are 269 tiles of the ordered compaction, past one
    pass of sfr_scan_kernel. The track ids are keypoints of frame 0, scattered over its tiles by the permutation, and -- for the
    points only pair 1 shows -- of frame 1, in the last tile. cloud_cap: what the device call is given (the default would be half the
    keypoints)."""
    sc = Scene(34, 3, 60, spare=(1100000, 2, 3))

    def half_other(blk):
        _scale_points(blk, np.arange(20, len(blk["P"])), 1 / 1.5)
    c = assemble(sc, [dict(a=0, b=1, unit=1.0, pts=np.arange(0, 50), junk=3), dict(a=1, b=2, unit=2.5, pts=np.arange(10, 60), junk=4, edit=half_other)])
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 40, 2.5)}
    c["cloud_cap"] = 64
    return c


def _ratio_spread():
    """Ratios that differ in every byte, so that each of the eight passes of the radix select has more than one bin to walk. Every
    pair but the first hangs on pair 0 and nothing hangs on them, so their scaled points reach no other pair.
    pair 1 (role 1): 41 links, its own point e scaled by 2^(-24 e), e = -20 .. 20 shuffled -- ratios 2^-480 .. 2^480 times the true one,
    which is the median. pair 2 (role 0): 40 links, 19 ratios below the true one and 20 above in steps of 2^20: the lower median is
    the true one, the upper is not. pair 3 (role 0): 257 links -- past one trip of the 256 lanes over the ratios --, 200 of them one
    match repeated (one ratio, bit for bit: more than the target in one bin, in every pass), 28 within 2^-3 .. 2^-48 of it on either
    side, four to a byte, and 29 whole powers of 2^16 away. pair 4 (role 0): 63 links, the true ratio and 31 on either side of it at
    random factors within 2, so that the mantissas differ from the first byte on: from pass 5 down the median is alone behind its
    prefix, and a ratio counted without the prefix compare falls into a lower bin."""
    sc = Scene(35, 6, 300)
    rng = np.random.default_rng(350)

    def wide(blk):
        blk["P"] *= np.exp2(-24.0 * rng.permutation(np.arange(-20, 21)))[:, None]

    def even(blk):
        blk["P"] *= np.exp2(-20.0 * rng.permutation(np.arange(-19, 21)))[:, None]

    def bunch(blk):
        f = [1.0]                                             # row 0: the match that is repeated
        for s in (3, 8, 16, 24, 32, 40, 48):                  # a relative step of 2^-s lands in byte 6, 5, .. 0 of the ratio
            f += [1 - 2.0 ** -s, 1 + 2.0 ** -s, 1 - 3 * 2.0 ** -s, 1 + 3 * 2.0 ** -s]
        f += [2.0 ** (16 * e) for e in range(-14, 16) if e]
        assert len(f) == len(blk["P"]) == 58
        blk["P"] *= np.array(f)[:, None]
        for k in ("q", "t", "mask"):
            blk[k] = np.concatenate([blk[k], np.repeat(blk[k][:1], 199)])
        blk["P"] = np.concatenate([blk["P"], np.repeat(blk["P"][:1], 199, 0)])

    def scatter(blk):
        blk["P"] *= rng.permutation(np.concatenate([rng.uniform(0.5, 1.0, 31), [1.0], rng.uniform(1.0, 2.0, 31)]))[:, None]
    specs = [dict(a=0, b=1, unit=1.0, pts=np.arange(300), junk=7),
             dict(a=1, b=2, unit=2.5, pts=np.arange(100, 141), edit=wide),
             dict(a=0, b=3, unit=0.7, pts=np.arange(30, 70), junk=3, edit=even),
             dict(a=0, b=4, unit=0.3, pts=np.arange(200, 258), edit=bunch),
             dict(a=0, b=5, unit=1.7, pts=np.arange(120, 183), junk=5, edit=scatter)]
    c = assemble(sc, specs)
    c["expect"] = {0: (GMS_OK, 0, 1.0), 1: (GMS_OK, 41, 2.5), 2: (GMS_OK, 40, 0.7), 3: (GMS_OK, 257, 0.3), 4: (GMS_OK, 63, 1.7)}
    return c


def _first_root_pair_fails():
    """upstream_failures' shape with the first registering pair out of the root without a two-view model: the two role-0 pairs behind
    it have no link table to measure against (n_links 0, r 0) and fail, and so does everything further down; nothing registers but
    the root. The reverse pair stays skipped."""
    sc = Scene(36, 8, 30)
    specs = [dict(a=2, b=0, unit=1.0, pts=np.arange(30), junk=4, status=NO_MODEL),
             dict(a=0, b=1, unit=0.25, pts=np.arange(30), junk=7),
             dict(a=1, b=3, unit=1.0, pts=np.arange(30)),      # both this pair and its link have a two-view result: 30 links, and no model
             dict(a=2, b=5, unit=2.0, pts=np.arange(30)),      # role 0
             dict(a=5, b=6, unit=1.0, pts=np.arange(5, 30)),
             dict(a=1, b=0, unit=1.0, pts=np.arange(30)),      # both frames are registered by the plan: skipped
             dict(a=2, b=7, unit=8.0, pts=np.arange(3, 30))]   # role 0
    c = assemble(sc, specs, root=2)
    c["expect"] = {0: (NO_MODEL, 0, 0.0), 1: (NO_MODEL, 0, 0.0), 2: (NO_MODEL, 30, 0.0), 3: (NO_MODEL, 0, 0.0), 4: (NO_MODEL, 25, 0.0),
                   5: (SKIPPED, 0, 0.0), 6: (NO_MODEL, 0, 0.0)}
    return c


def _misfit_records():
    """chain_roles plus seven pairs over seven more frames of 60 keypoints each. `host_pairs` -- what makes the plan, total_m and max_m --
    holds sane records: pairs 7 .. 12 each register a frame of their own (7 .. 12) out of a registered one, with ten inlier matches
    between keypoints that their link saw, real points and a pose, so that each would register if it were read; pair 13 = (11, 13)
    hangs on pair 11. `pairs` -- what the device and the statement read -- differs in pairs 7 .. 12: frame_a = n_frames; frame_b = -1;
    m = -3; match_off = -1; a range of 10 that ends 5 slots past total_m (its first 5 slots, the arrays' last, hold pair 13's inlier
    matches and points); match_off = 2^63 - 2 with m = 5, whose sum does not fit 64 bits. Each of them ends skipped, pair 13 without
    a model, and everything else is chain_roles' own."""
    import sfm_register_ref
    base, sc = _chain_roles(), Scene(11, 7, 60)
    n0, f0, m0 = len(base["pairs"]), len(base["frame_off"]) - 1, len(base["mask"])
    frame_off = np.concatenate([base["frame_off"], base["frame_off"][-1] + 60 * np.arange(1, 8)]).astype(np.int64)
    from_frame = [1, 2, 3, 4, 1, 2, 11]
    host = np.zeros(7, PAIR_DTYPE)
    tv = np.zeros(7, TWO_VIEW_DTYPE)
    total_m = m0 + 6 * 12 + 10                                # the arrays end with pair 13's last match
    matches, mask, points = np.zeros(total_m, DMATCH_DTYPE), np.full(total_m, 255, np.uint8), np.full((total_m, 3), FILL)
    matches[:m0], mask[:m0], points[:m0] = base["matches"], base["mask"], base["points3d"]
    matches["queryIdx"][m0:], matches["trainIdx"][m0:] = -5, 10 ** 6
    s = np.arange(10, 20)                                     # scene points that every registering pair of chain_roles shows
    for k, a in enumerate(from_frame):
        off = m0 + 12 * k
        host[k] = (a, f0 + k, 10, 0, off)
        matches["queryIdx"][off:off + 10], matches["trainIdx"][off:off + 10] = (sc.perm[a][s] if a < f0 else s), s
        mask[off:off + 10] = 1
        points[off:off + 10] = sc.cam(min(a, f0 - 1), s)
        tv[k]["R"], tv[k]["t"], tv[k]["n_points"], tv[k]["n_triangulated"] = np.eye(3), (1.0, 0.0, 0.0), 10, 10
    dev = host.copy()
    dev["frame_a"][0] = f0 + 7
    dev["frame_b"][1] = -1
    dev["m"][2] = -3
    dev["match_off"][3] = -1
    dev["match_off"][4] = total_m - 5
    dev["match_off"][5], dev["m"][5] = 2 ** 63 - 2, 5
    host_pairs = np.concatenate([base["pairs"], host])
    R, t = base["truth"]
    c = dict(base, frame_off=frame_off, pairs=np.concatenate([base["pairs"], dev]), host_pairs=host_pairs, matches=matches, mask=mask,
             points3d=points, tv=np.concatenate([base["tv"], tv]), total_m=total_m, n_base_pairs=n0, n_base_frames=f0,
             plan=sfm_register_ref.plan(np.stack([host_pairs["frame_a"], host_pairs["frame_b"]], 1), f0 + 7, base["root"]),
             truth=(np.concatenate([R, np.zeros((7, 3, 3))]), np.concatenate([t, np.zeros((7, 3))])))
    c["expect"] = {**base["expect"], **{n0 + k: (SKIPPED, 0, 0.0) for k in range(6)}, n0 + 6: (NO_MODEL, 0, 0.0)}
    return c


def _bad_plan_links():
    """chain_roles with plan entries that the walk cannot follow. `plan` (what the device and the statement are given in place of the
    pair list's own): pair 1 links to itself and pair 2 forward, to pair 4 -- both are skipped, and pair 6, which hangs on pair 2,
    has no model. `more_plans`: pair 1 with link -2 and pair 6 with link n_pairs + 5 (both skipped, the rest as planned); and pair 0
    with link -2, which takes every registering pair with it. Each with the (status, n_links, S) it must end in."""
    import sfm_register_ref
    c = _chain_roles()
    n = len(c["pairs"])
    own = sfm_register_ref.plan(np.stack([c["pairs"]["frame_a"], c["pairs"]["frame_b"]], 1), len(c["frame_off"]) - 1, c["root"])

    def with_links(links):
        p = own.copy()
        for i, link in links.items():
            assert p[i]["registers"]
            p[i]["link"] = link
        return p
    skipped, failed = (SKIPPED, 0, 0.0), (NO_MODEL, 0, 0.0)
    c["plan"] = with_links({1: 1, 2: 4})
    c["expect"] = {**c["expect"], 1: skipped, 2: skipped, 6: failed}
    c["more_plans"] = [(with_links({1: -2, 6: n + 5}), {**c["expect"], 1: skipped, 2: (GMS_OK, 41, 0.7), 6: skipped}),
                       # (pair 6 and its link, pair 2, both have a two-view result: their 35 links are measured)
                       (with_links({0: -2}), {**c["expect"], 0: skipped, 1: failed, 2: failed, 6: (NO_MODEL, 35, 0.0)})]
    return c


CASES = {"chain_roles": _chain_roles, "lowest_k_wins": _lowest_k_wins, "invalid_links_and_min_links": _invalid_links_and_min_links,
         "upstream_failures": _upstream_failures, "many_links": _many_links, "chain_300": _chain_300, "star_300": _star_300,
         "two_branches_300": _two_branches_300, "tiles_past_256": _tiles_past_256, "ratio_spread": _ratio_spread,
         "first_root_pair_fails": _first_root_pair_fails, "misfit_records": _misfit_records, "bad_plan_links": _bad_plan_links}
UNFIT = ("misfit_records", "bad_plan_links")   # cases whose records or plan differ from what the pair list alone gives


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
