"""One-to-one matches per pair and the registration on them, stated in numpy: the library's own definition, which
match_unique_core.h / match_unique_kernels.hip compute on the device and tests/cpp/match_unique_host.cpp on the host.

Match k of pair i is live when k < n_i (n_i = clamp(tv.n_points, 0, m) when tv.status is GMS_OK, else 0; m without tv), its mask byte
is non-zero (no mask: every byte counts as set) and both indices lie inside their frames. key(k) = (ord(distance) << 32) | k, with
ord(d) the bit pattern of a finite d > 0, 0 for +0 and -0, 0xFFFFFFFF for anything else. A live match is kept when its key is the
least among the live matches of its pair that share its trainIdx and the least among those that share its queryIdx. Not a maximum
matching: a match may lose on one side to a match that loses on the other, and then neither is kept."""
import numpy as np

import sfm_register_ref as R

GMS_OK = R.GMS_OK


def ord_of(distance):
    """ord(d) of float32 distances -> uint64, from the bit patterns alone."""
    u = np.ascontiguousarray(distance, dtype=np.float32).view(np.uint32).astype(np.uint64)
    out = u.copy()
    out[(u & np.uint64(0x7FFFFFFF)) == 0] = 0
    out[(u >= np.uint64(0x7F800000)) & ((u & np.uint64(0x7FFFFFFF)) != 0)] = 0xFFFFFFFF
    return out


def keys_of(distance):
    return (ord_of(distance) << np.uint64(32)) | np.arange(len(distance), dtype=np.uint64)


def live_of(i, frame_off, pairs, matches, mask=None, tv=None):
    """bool [m] of a fitting pair: which of its slots hold a live match."""
    p = pairs[i]
    m, off = int(p["m"]), int(p["match_off"])
    n = m if tv is None else (int(np.clip(tv[i]["n_points"], 0, m)) if tv[i]["status"] == GMS_OK else 0)
    counts = np.diff(np.asarray(frame_off, dtype=np.int64))
    q, t = matches["queryIdx"][off:off + m].astype(np.int64), matches["trainIdx"][off:off + m].astype(np.int64)
    live = (np.arange(m) < n) & (q >= 0) & (q < counts[p["frame_a"]]) & (t >= 0) & (t < counts[p["frame_b"]])
    if mask is not None:
        live &= np.asarray(mask)[off:off + m] != 0
    return live


def unique(frame_off, pairs, matches, mask=None, tv=None, total_m=None):
    """-> (keep uint8 [total_m], counts int32 [n_pairs, 2] = live, kept). total_m: the length of the match arrays (default: the
    matches'). Slots of no fitting pair (R.pair_fits) are 0."""
    frame_off = np.asarray(frame_off, dtype=np.int64)
    total_m = len(matches) if total_m is None else int(total_m)
    keep, counts = np.zeros(total_m, np.uint8), np.zeros((len(pairs), 2), np.int32)
    for i in range(len(pairs)):
        if not R.pair_fits(pairs[i], frame_off, total_m):
            continue
        m, off = int(pairs[i]["m"]), int(pairs[i]["match_off"])
        live = live_of(i, frame_off, pairs, matches, mask, tv)
        key = keys_of(matches["distance"][off:off + m])
        q, t = matches["queryIdx"][off:off + m], matches["trainIdx"][off:off + m]
        best_q, best_t = {}, {}
        for k in np.nonzero(live)[0].tolist():
            best_q[int(q[k])] = min(best_q.get(int(q[k]), key[k]), key[k])
            best_t[int(t[k])] = min(best_t.get(int(t[k]), key[k]), key[k])
        kept = np.array([bool(live[k]) and best_q[int(q[k])] == key[k] and best_t[int(t[k])] == key[k] for k in range(m)], dtype=bool)
        keep[off:off + m] = kept
        counts[i] = (int(live.sum()), int(kept.sum()))
    return keep, counts


def register_keep(frame_off, pairs, matches, mask, points3d, tv, root=0, min_links=8, plan=None, total_m=None, keep=None):
    """R.register on a keep plane (uint8 per match slot; None: R.register itself). views, registration, points_world and the links do
    not read the plane; a match whose byte is 0 is no edge and no estimate, its track slot stays -1, and track, cloud* and the
    summary's n_tracks, n_points, n_multi follow the kept matches."""
    base = R.register(frame_off, pairs, matches, mask, points3d, tv, root, min_links, plan, total_m)
    if keep is None:
        return base
    frame_off = np.asarray(frame_off, dtype=np.int64)
    keep = np.asarray(keep)
    counts = np.diff(frame_off)
    total_kp = int(frame_off[-1])
    total_m = len(mask) if total_m is None else int(total_m)
    world = base["points_world"]
    ok = base["registration"]["status"] == GMS_OK
    parent = np.arange(total_kp)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    member = np.zeros(total_kp, bool)
    est = []   # (pair, rank, global keypoint of frame_a), in ascending (pair, rank)
    for i in np.nonzero(ok)[0]:   # (an ok pair fits)
        off = int(pairs[i]["match_off"])
        k, q, t, rank, _ = R._pair_view(i, pairs, matches, mask, tv, counts)
        on = keep[off + k] != 0
        q, t, rank = q[on], t[on], rank[on]
        u, v = frame_off[pairs[i]["frame_a"]] + q, frame_off[pairs[i]["frame_b"]] + t
        member[u], member[v] = True, True
        for x, y in zip(u.tolist(), v.tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
        est += [(int(i), int(rk), int(x)) for rk, x in zip(rank, u)]
    root_of = np.arange(total_kp, dtype=np.int64)
    for g in np.nonzero(member)[0].tolist():
        root_of[g] = find(g)
    ids = np.unique(root_of[member])
    index_of = {int(g): c for c, g in enumerate(ids)}
    n_tracks = len(ids)
    track = np.full(len(world), -1, np.int32)
    cloud, spread = np.zeros((n_tracks, 3)), np.zeros(n_tracks)
    cloud_obs = np.bincount([index_of[int(r)] for r in root_of[member]], minlength=n_tracks).astype(np.int32)
    cloud_est = np.zeros(n_tracks, np.int32)
    rep = {}
    for i, rk, g in est:
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
        if not np.isnan(d):
            spread[c] = max(spread[c], d)
    frame_of = np.searchsorted(frame_off, np.arange(total_kp), side="right") - 1
    keys = np.unique(np.stack([root_of[member], frame_of[member]], 1), axis=0) if member.any() else np.zeros((0, 2), np.int64)
    frames_in = np.bincount([index_of[int(r)] for r in keys[:, 0]], minlength=n_tracks)
    summary = base["summary"].copy()
    summary["n_tracks"], summary["n_points"], summary["n_multi"] = n_tracks, len(est), int((frames_in < cloud_obs).sum())
    return dict(base, track=track, cloud=cloud, cloud_id=ids.astype(np.int32), cloud_obs=cloud_obs, cloud_est=cloud_est,
                cloud_spread=spread, summary=summary)


def redirect_trains(c, fraction, seed, max_distance=5):
    """A copy of a registration case (sfm_register_cases) in which `fraction` of every pair's train indices name the train index of
    another match of the pair, and the distances are drawn from 0 .. max_distance: what a nearest-neighbour matcher leaves."""
    rng = np.random.default_rng(seed)
    m = c["matches"].copy()
    for p in c["pairs"]:
        off, n = int(p["match_off"]), int(p["m"])
        if n < 2 or off < 0 or off + n > len(m):   # (a record that does not fit the arrays has no matches to change)
            continue
        t = m["trainIdx"][off:off + n].copy()
        hit = np.nonzero(rng.random(n) < fraction)[0]
        t[hit] = t[rng.integers(0, n, len(hit))]
        m["trainIdx"][off:off + n] = t
        m["distance"][off:off + n] = rng.integers(0, max_distance + 1, n).astype(np.float32)
    return dict(c, matches=m)
