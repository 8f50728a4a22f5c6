"""The registration of many two-view results into one frame, stated in numpy: the library's own definition, which
sfm_register_core.h / sfm_register_kernels.hip compute on the device and tests/cpp/sfm_register_host.cpp on the host.

Inputs are what gms_two_view_batch_device leaves: frame_off [n_frames + 1], pairs (PAIR_DTYPE), the survivors `matches` (DMATCH_DTYPE),
`mask` (uint8) and `points3d` ([.., 3] float64) laid out by the pairs' match_off, and `tv` (TWO_VIEW_DTYPE per pair). Pair i has
n_i = clamp(tv.n_points, 0, m) matches when tv.status is GMS_OK, none otherwise; rank(k) = non-zero mask bytes before k; its points
are points3d[match_off + rank]. A match whose queryIdx / trainIdx lies outside its frame is ignored everywhere, and so is a pair
whose record does not fit the arrays or whose plan entry the walk cannot follow (pair_fits, plan_entry_fits: the kernels' rule)."""
import numpy as np

GMS_OK, GMS_SFM_SKIPPED, GMS_ERR_NO_MODEL = 0, 1, -8
NO_SLOT = np.iinfo(np.int32).max

PLAN_DTYPE = np.dtype([("registers", "<i4"), ("link", "<i4"), ("role", "<i4"), ("depth", "<i4")])
VIEW_DTYPE = np.dtype([("R", "<f8", (3, 3)), ("t", "<f8", (3,)), ("registered", "<i4"), ("pair", "<i4")])
PAIR_REG_DTYPE = np.dtype([("r", "<f8"), ("S", "<f8"), ("n_links", "<i4"), ("depth", "<i4"), ("link", "<i4"), ("role", "<i4"),
                           ("status", "<i4"), ("reserved", "<i4")])
SUMMARY_DTYPE = np.dtype([("n_tracks", "<i8"), ("n_points", "<i8"), ("n_multi", "<i8"), ("n_registered", "<i4"), ("n_ok_pairs", "<i4")])


def plan(frame_pairs, n_frames, root=0):
    """The plan from the pair list alone: frame_pairs [n, 2] -> PLAN_DTYPE [n]. Raises ValueError on a frame index out of range."""
    fp = np.asarray(frame_pairs, dtype=np.int64).reshape(-1, 2)
    if not 0 <= root < n_frames or ((fp < 0) | (fp >= n_frames)).any():
        raise ValueError("frame index out of range")
    out = np.zeros(len(fp), PLAN_DTYPE)
    out["link"] = -1
    reg_by = np.full(n_frames, -2, np.int64)   # -2: not registered; -1: the root; else the pair that registered the frame
    reg_by[root] = -1
    first_root = -1
    for i, (a, b) in enumerate(fp):
        if reg_by[a] == -2 or reg_by[b] != -2:
            continue
        out[i]["registers"] = 1
        if a == root:
            if first_root < 0:
                first_root = i
            else:
                out[i]["link"], out[i]["role"] = first_root, 0
        else:
            out[i]["link"], out[i]["role"] = reg_by[a], 1
        if out[i]["link"] >= 0:
            out[i]["depth"] = out[out[i]["link"]]["depth"] + 1
        reg_by[b] = i
    return out


plan_of_pairs = plan   # (register() has an argument of the name)


def rows_times(V, M):
    """V @ M for rows V [n, 3], as three products summed in order -- what the C code does, also on non-finite values."""
    return V[:, 0:1] * M[0] + V[:, 1:2] * M[1] + V[:, 2:3] * M[2]


def lower_median(v):
    return float(np.sort(np.asarray(v, dtype=np.float64))[(len(v) - 1) // 2])


def _pair_view(i, pairs, matches, mask, tv, counts):
    """(k of the pair's matches with a non-zero mask byte and both indices inside their frames, their q, t, rank) -- and the number
    of non-zero mask bytes."""
    p = pairs[i]
    n = int(np.clip(tv[i]["n_points"], 0, p["m"])) if tv[i]["status"] == GMS_OK else 0
    off = int(p["match_off"])
    mk = mask[off:off + n] != 0
    rank = np.cumsum(mk) - mk
    q, t = matches["queryIdx"][off:off + n].astype(np.int64), matches["trainIdx"][off:off + n].astype(np.int64)
    inside = (q >= 0) & (q < counts[p["frame_a"]]) & (t >= 0) & (t < counts[p["frame_b"]])
    k = np.nonzero(mk & inside)[0]
    return k, q[k], t[k], rank[k], int(mk.sum())


def pair_fits(pair, frame_off, total_m):
    """sfr::pair_fits of sfm_register_core.h in Python's integers: both frame indices in [0, n_frames), m >= 0, the match range inside
    [0, total_m] and both frames' keypoint ranges inside [0, total_kp]."""
    n_frames, total_kp = len(frame_off) - 1, int(frame_off[-1])
    a, b, m, off = int(pair["frame_a"]), int(pair["frame_b"]), int(pair["m"]), int(pair["match_off"])
    if not (0 <= a < n_frames and 0 <= b < n_frames) or m < 0 or off < 0 or off + m > total_m:
        return False
    return all(0 <= int(frame_off[f]) <= int(frame_off[f + 1]) <= total_kp for f in (a, b))


def plan_entry_fits(entry, i):
    """sfr::plan_entry_fits: an entry that registers links to an earlier pair or to none."""
    return not entry["registers"] or -1 <= int(entry["link"]) < i


_NO_MATCHES = (np.zeros(0, np.int64),) * 4 + (0,)


def register(frame_off, pairs, matches, mask, points3d, tv, root=0, min_links=8, plan=None, total_m=None):
    """-> dict(plan, views VIEW_DTYPE [n_frames], registration PAIR_REG_DTYPE [n_pairs], points_world [len(points3d), 3], track int32
    [len(points3d)], cloud [n_tracks, 3], cloud_id, cloud_obs, cloud_est (int32), cloud_spread (float64), summary SUMMARY_DTYPE [1]).
    points_world / track entries that belong to no point are 0 / -1.

    plan: PLAN_DTYPE entries to walk instead of the pair list's own (returned as given); total_m: the length of the match arrays
    (default: the mask's). A pair that does not fit -- pair_fits, or a plan entry that is not plan_entry_fits -- has no matches and
    the plan entry {0, -1, 0, 0}, as in the kernels: it ends GMS_SFM_SKIPPED with link -1 and zeros, and what hangs on it by the plan
    fails by the ordinary rule. The pair list's own plan is made only where none is given: it refuses a frame index out of range."""
    frame_off = np.asarray(frame_off, dtype=np.int64)
    n_frames, n_pairs = len(frame_off) - 1, len(pairs)
    counts = np.diff(frame_off)
    P = np.asarray(points3d, dtype=np.float64).reshape(-1, 3)
    given = plan
    if given is None:
        given = plan_of_pairs(np.stack([pairs["frame_a"], pairs["frame_b"]], 1) if n_pairs else np.zeros((0, 2)), n_frames, root)
    given = np.asarray(given, dtype=PLAN_DTYPE)
    total_m = len(mask) if total_m is None else int(total_m)
    fits = [pair_fits(pairs[i], frame_off, total_m) and plan_entry_fits(given[i], i) for i in range(n_pairs)]
    pl = given.copy()
    for i in range(n_pairs):
        if not fits[i]:
            pl[i] = (0, -1, 0, 0)
    views = np.zeros(n_frames, VIEW_DTYPE)
    views["pair"] = -1
    views[root]["R"], views[root]["registered"] = np.eye(3), 1
    reg = np.zeros(n_pairs, PAIR_REG_DTYPE)
    reg["link"], reg["status"] = -1, GMS_SFM_SKIPPED
    world = np.zeros_like(P)
    track = np.full(len(P), -1, np.int32)
    pv = [_pair_view(i, pairs, matches, mask, tv, counts) if fits[i] else _NO_MATCHES for i in range(n_pairs)]
    base_ok = [bool(pl[i]["registers"]) and tv[i]["status"] == GMS_OK and tv[i]["n_triangulated"] > 0 for i in range(n_pairs)]
    ok = np.zeros(n_pairs, bool)
    for i in range(n_pairs):
        if not pl[i]["registers"]:
            continue
        a, b, off = int(pairs[i]["frame_a"]), int(pairs[i]["frame_b"]), int(pairs[i]["match_off"])
        j, role = int(pl[i]["link"]), int(pl[i]["role"])
        reg[i]["depth"], reg[i]["link"], reg[i]["role"] = pl[i]["depth"], j, role
        S = 1.0
        good = base_ok[i]
        if j >= 0:
            n_links, r = 0, 0.0
            if base_ok[i] and base_ok[j]:
                kj, qj, tj, rankj, _ = pv[j]
                slot = np.full(counts[a], NO_SLOT, np.int64)
                np.minimum.at(slot, tj if role == 1 else qj, kj)
                rank_of_k = dict(zip(kj.tolist(), rankj.tolist()))
                k, q, _, rank, _ = pv[i]
                has = slot[q] != NO_SLOT
                joff = int(pairs[j]["match_off"])
                X = P[joff + np.array([rank_of_k[s] for s in slot[q[has]].tolist()], dtype=np.int64)]
                with np.errstate(all="ignore"):
                    if role == 1:
                        X = rows_times(X, tv[j]["R"].T) + tv[j]["t"]
                    Y = P[off + rank[has]]
                    valid = np.isfinite(X).all(1) & np.isfinite(Y).all(1) & (X[:, 2] > 0) & (Y[:, 2] > 0)
                    rho = np.sqrt((X[valid] ** 2).sum(1)) / np.sqrt((Y[valid] ** 2).sum(1))
                n_links = int(valid.sum())
                r = lower_median(rho) if n_links else 0.0
            reg[i]["n_links"], reg[i]["r"] = n_links, r
            good = good and ok[j] and n_links >= min_links
            if good:
                S = reg[j]["S"] * r
        if not good:
            reg[i]["status"] = GMS_ERR_NO_MODEL
            continue
        ok[i] = True
        reg[i]["status"], reg[i]["S"] = GMS_OK, S
        Ga = views[a]
        Ri, ta = tv[i]["R"], Ga["t"]
        views[b]["R"] = rows_times(Ri, Ga["R"])
        views[b]["t"] = Ri[:, 0] * ta[0] + Ri[:, 1] * ta[1] + Ri[:, 2] * ta[2] + S * tv[i]["t"]
        views[b]["registered"], views[b]["pair"] = 1, i
        n_pts = pv[i][4]
        with np.errstate(all="ignore"):
            world[off:off + n_pts] = rows_times(S * P[off:off + n_pts] - Ga["t"], Ga["R"])
    # tracks: connected components of the ok pairs' edges; the id is the least global keypoint index
    total_kp = int(frame_off[-1])
    parent = np.arange(total_kp)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    member = np.zeros(total_kp, bool)
    est = []   # (pair, rank, global keypoint of frame_a)
    for i in np.nonzero(ok)[0]:
        k, q, t, rank, _ = pv[i]
        u, v = frame_off[pairs[i]["frame_a"]] + q, frame_off[pairs[i]["frame_b"]] + t
        member[u], member[v] = True, True
        for x, y in zip(u.tolist(), v.tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
        est += [(int(i), int(rk), int(x)) for rk, x in zip(rank, u)]
    root_of = np.arange(total_kp, dtype=np.int64)             # (a keypoint of no edge is its own root, and nothing below reads it)
    for g in np.nonzero(member)[0].tolist():
        root_of[g] = find(g)
    ids = np.unique(root_of[member])
    index_of = {int(g): c for c, g in enumerate(ids)}
    n_tracks = len(ids)
    cloud, spread = np.zeros((n_tracks, 3)), np.zeros(n_tracks)
    cloud_obs = np.bincount([index_of[int(r)] for r in root_of[member]], minlength=n_tracks).astype(np.int32)
    cloud_est = np.zeros(n_tracks, np.int32)
    rep = {}
    for i, rk, g in est:   # est is in ascending (pair, rank)
        c = index_of[int(root_of[g])]
        track[int(pairs[i]["match_off"]) + rk] = ids[c]
        cloud_est[c] += 1
        rep.setdefault(c, (i, rk))
    for c, (i, rk) in rep.items():
        cloud[c] = world[int(pairs[i]["match_off"]) + rk]
    for i, rk, g in est:
        c = index_of[int(root_of[g])]
        with np.errstate(all="ignore"):
            d = np.sqrt(((world[int(pairs[i]["match_off"]) + rk] - cloud[c]) ** 2).sum())
        if not np.isnan(d):   # (a distance that is not a number -- an estimate with a non-finite coordinate -- does not count)
            spread[c] = max(spread[c], d)
    frame_of = np.searchsorted(frame_off, np.arange(total_kp), side="right") - 1
    keys = np.unique(np.stack([root_of[member], frame_of[member]], 1), axis=0) if member.any() else np.zeros((0, 2), np.int64)
    frames_in = np.bincount([index_of[int(r)] for r in keys[:, 0]], minlength=n_tracks)
    summary = np.zeros(1, SUMMARY_DTYPE)
    summary["n_tracks"], summary["n_points"], summary["n_multi"] = n_tracks, len(est), int((frames_in < cloud_obs).sum())
    summary["n_registered"], summary["n_ok_pairs"] = int(views["registered"].sum()), int(ok.sum())
    return dict(plan=given, views=views, registration=reg, points_world=world, track=track, cloud=cloud, cloud_id=ids.astype(np.int32),
                cloud_obs=cloud_obs, cloud_est=cloud_est, cloud_spread=spread, summary=summary)


def camera_centres(views):
    """The camera centres -R^T t of the registered views (rows of the others are NaN)."""
    c = np.full((len(views), 3), np.nan)
    for f, v in enumerate(views):
        if v["registered"]:
            c[f] = -v["R"].T @ v["t"]
    return c
