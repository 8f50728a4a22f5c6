"""The cases of the dense fusion's tests, shared by tests/test_dense_fuse_ref.py (CPU) and
tests/test_gpu_dense_fuse.py (GPU): hand-made sources on a plan whose arithmetic is exact, the wild inputs, and the rendered plane of
tests/rectify_cases.py seen by a third camera. A case is a dict: sources (dense_fuse_ref.source dicts), neighbors int32 [n_src, n_nb],
tol16, min_support, fused_cap (None: room for all), channels; `expect` holds what the case is named for, per source the
(support, conflict, kept) of its points, which tests/test_dense_fuse_ref.py asserts of the statement. Nothing here is part of the
statement."""
import numpy as np

import dense_fuse_ref as fr
import rectify_cases as rc
import rectify_ref as rr

W, H = 20, 12
F16, MIN16 = -16, 16          # the matcher's FILTERED code and the least disparity of a point
NO_MODEL, SKIPPED = -8, 1


def hand_plan(w=W, h=H, fx=40.0, cx=8.0, cy=6.0, B=1.0, status=0):
    """R1 = R2 = I, fx' = fy' = 40, integer principal point, B = 1: a pixel with d16 = 64 is the point at depth 10, and e = 640 / z."""
    P = rr.zero_plan(status)
    if status == 0:
        for k in ("R1", "R2"):
            P[k][0][[0, 4, 8]] = 1.0
        P["fx"], P["fy"], P["cx"], P["cy"], P["B"] = fx, fx, cx, cy, B
        P["out_w"], P["out_h"] = w, h
    return P


def empty_map(w=W, h=H):
    return np.full((h, w), F16, np.int16), np.ones((h, w), np.uint8)


def map_source(disp, valid=None, plan=None, color_seed=None, channels=1, view=None, reg=None):
    """A source whose points are its own map's (rectify_ref.cloud with the source's view and scale; a source that is not live gets the
    points it would have had, which the fusion must not count)."""
    disp = np.asarray(disp, dtype=np.int16)
    valid = np.ones(disp.shape, np.uint8) if valid is None else valid
    plan = hand_plan(disp.shape[1], disp.shape[0]) if plan is None else plan
    ok_plan = plan if int(plan["status"][0]) == 0 else hand_plan(disp.shape[1], disp.shape[0])
    S = float(reg[0]) if reg is not None and reg[0] > 0 else 1.0
    with np.errstate(all="ignore"):
        xyz, _, _ = rr.cloud(disp, valid, None, ok_plan, F16, MIN16, S, None if view is None else (view[0], view[1]))
    color = None if color_seed is None else rc.noise(color_seed, len(xyz), channels)
    return fr.source(disp, valid, plan, xyz, color=color, filtered16=F16, min_disp16=MIN16, view=view, reg=reg)


def pixel_point(u, v, d16=64, fx=40.0, cx=8.0, cy=6.0):
    z = fx * 16.0 / d16
    return ((u - cx) * z / fx, (v - cy) * z / fx, z)


def _case(name, sources, neighbors=None, tol16=16, min_support=1, fused_cap=None, channels=1, expect=None):
    nb = fr.default_neighbors(len(sources)) if neighbors is None else np.asarray(neighbors, dtype=np.int32).reshape(len(sources), -1)
    return dict(name=name, sources=sources, neighbors=nb, tol16=tol16, min_support=min_support, fused_cap=fused_cap, channels=channels,
                expect=expect)


def probe_case(tol16):
    """Source 0 holds hand-made points, source 1 the map they are looked up in. Per point: what look() must say."""
    t = tol16
    disp, valid = empty_map()
    pts, want = [], []

    def add(p, verdict):
        pts.append(p)
        want.append(verdict)

    for u, d, verdict in ((2, 64 + t, fr.CONSISTENT), (3, 64 - t, fr.CONSISTENT), (4, 64 + t + 1, fr.CONFLICT), (5, 64 - t - 1, fr.CONFLICT)):
        disp[3, u] = d
        add(pixel_point(u, 3), verdict)
    add(pixel_point(-1, 3), fr.UNSEEN)          # ui = -1
    add(pixel_point(W, 3), fr.UNSEEN)           # ui = width
    add(pixel_point(2, -1), fr.UNSEEN)          # vi = -1
    add(pixel_point(2, H), fr.UNSEEN)           # vi = height
    disp[6, 10], disp[6, 16] = 40, 40           # the even neighbours of 10.5 and 15.5; 11 and 15 stay filtered
    add((1.0, 0.0, 16.0), fr.CONSISTENT)        # u = 40 / 16 + 8 = 10.5 -> 10; e = 640 / 16 = 40
    add((3.0, 0.0, 16.0), fr.CONSISTENT)        # u = 15.5 -> 16
    disp[3, 6], valid[3, 6] = 64, 0
    add(pixel_point(6, 3), fr.UNSEEN)           # valid = 0
    add(pixel_point(7, 3), fr.UNSEEN)           # the filtered value
    disp[3, 8] = MIN16 - 8
    add(pixel_point(8, 3, d16=8), fr.UNSEEN)    # below min_disp16
    add((0.0, 0.0, 0.0), fr.UNSEEN)             # r.z = 0
    x, y, z = pixel_point(2, 3)
    add((-x, -y, -z), fr.UNSEEN)                # r.z < 0, the same pixel
    e_disp, e_valid = empty_map()
    s0 = fr.source(e_disp, e_valid, hand_plan(), np.asarray(pts, dtype=np.float32), color=rc.noise(3, len(pts), 3), filtered16=F16, min_disp16=MIN16)
    s1 = map_source(disp, valid, color_seed=4, channels=3)
    want = np.asarray(want)
    exp0 = ((1 + (want == fr.CONSISTENT)).astype(np.uint8), (want == fr.CONFLICT).astype(np.uint8), np.ones(len(want), bool))
    return _case(f"probe_tol{tol16}", [s0, s1], tol16=tol16, channels=3, expect={0: exp0})


def owner_case(min_support):
    """Three sources see patch A; only 1 and 2 see patch B; only 2 sees patch C."""
    maps = [empty_map()[0] for _ in range(3)]
    for m in maps:
        m[2:5, 3:7] = 64            # A: 12 pixels
    for m in maps[1:]:
        m[7:9, 10:15] = 128         # B: 10 pixels, depth 5
    maps[2][10, 1:4] = 32           # C: 3 pixels, depth 20
    srcs = [map_source(m, color_seed=20 + i) for i, m in enumerate(maps)]
    nA, nB, nC = 12, 10, 3
    lone = min_support <= 1
    exp = {0: (np.full(nA, 3, np.uint8), np.zeros(nA, np.uint8), np.ones(nA, bool)),
           1: (np.r_[np.full(nA, 3), np.full(nB, 2)].astype(np.uint8), np.zeros(nA + nB, np.uint8), np.r_[np.zeros(nA, bool), np.ones(nB, bool)]),
           2: (np.r_[np.full(nA, 3), np.full(nB, 2), np.full(nC, 1)].astype(np.uint8), np.zeros(nA + nB + nC, np.uint8),
               np.r_[np.zeros(nA + nB, bool), np.full(nC, lone)])}
    return _case(f"owner_min{min_support}", srcs, min_support=min_support, expect=exp)


def skipped_slots_case():
    """Slots holding -1, the source itself, an index >= n_src and the three forms of a source that is not live are all skipped."""
    m = empty_map()[0]
    m[2:5, 3:7] = 64
    view = (np.eye(3).reshape(9), np.zeros(3), 1)
    srcs = [map_source(m), map_source(m), map_source(m, plan=hand_plan(status=NO_MODEL)), map_source(m, view=view, reg=(1.0, SKIPPED)),
            map_source(m, view=view, reg=(0.0, 0)), map_source(m, view=(np.eye(3).reshape(9), np.zeros(3), 0), reg=(1.0, 0))]
    nb = np.array([[-1, 0, 99, 2, 3, 4, 5, 1]] + [[0, 1, 2, 3, 4, 5, -1, -1]] * 5, np.int32)
    n = 12
    exp = {0: (np.full(n, 2, np.uint8), np.zeros(n, np.uint8), np.ones(n, bool)),
           1: (np.full(n, 2, np.uint8), np.zeros(n, np.uint8), np.zeros(n, bool))}
    for i in (2, 3, 4, 5):
        exp[i] = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, bool))
    return _case("skipped_slots", srcs, neighbors=nb, expect=exp)


def count_and_cap_case():
    """count > cap (the first cap points count), count < cap, and a fused_cap below the total."""
    m = empty_map()[0]
    m[2:5, 3:7] = 64
    a, b, c = map_source(m, color_seed=30), map_source(empty_map()[0]), map_source(m, color_seed=31)
    a["count"] = 40                       # cap 12
    c["count"] = 5                        # cap 12
    nb = np.array([[-1], [-1], [-1]], np.int32)
    exp = {0: (np.ones(12, np.uint8), np.zeros(12, np.uint8), np.ones(12, bool)), 1: (np.zeros(0, np.uint8),) * 2 + (np.zeros(0, bool),),
           2: (np.ones(5, np.uint8), np.zeros(5, np.uint8), np.ones(5, bool))}
    return _case("count_and_cap", [a, b, c], neighbors=nb, fused_cap=14, expect=exp)


def view_and_scale_case():
    """A view that is not the identity and S != 1, against points made by rectify_ref.cloud(..., S, view): two sources of one map."""
    m = empty_map()[0]
    m[1:11, 2:18] = 64
    m[4:6, 5:9] = 96
    G = (rc.rot((0.2, 1.0, -0.3), 10.0).reshape(9), np.array([0.3, -0.2, 0.5]), 1)
    srcs = [map_source(m, view=G, reg=(1.5, 0)), map_source(m, view=G, reg=(1.5, 0))]
    n = int((m != F16).sum())
    exp = {0: (np.full(n, 2, np.uint8), np.zeros(n, np.uint8), np.ones(n, bool)), 1: (np.full(n, 2, np.uint8), np.zeros(n, np.uint8), np.zeros(n, bool))}
    return _case("view_and_scale", srcs, expect=exp)


def quarter_turn_case():
    """Sources of 37 x 29 and 29 x 37: the plans of a horizontal and a vertical baseline from one camera 1; both maps a plane at depth 10."""
    srcs = []
    for name in ("t_minus_x", "t_minus_y"):
        cam, dist, R, t, _, _ = rc.plan_inputs(name)
        P = rr.make_plan(cam, dist, R, t, rc.SIZE_SMALL)
        m = np.full((int(P["out_h"][0]), int(P["out_w"][0])), 64, np.int16)
        srcs.append(map_source(m, plan=P, color_seed=40 + len(srcs)))
    return _case("quarter_turn", srcs)


def wild_case():
    """NaN and +-inf coordinates, float32's largest, a zeroed plan that says ok, fx' = 1e300, a view with a huge t: everything UNSEEN or a
    verdict, never a load outside a map."""
    m = empty_map()[0]
    m[:] = 64
    big = np.finfo(np.float32).max
    vals = [np.nan, np.inf, -np.inf, big, -big, 0.0, 1e-30, 1.0]
    pts = [(a, b, c) for a in vals for b in (np.nan, -np.inf, big, 0.5) for c in (np.nan, np.inf, -big, 0.0, 10.0, 1e-38)]
    e_disp, e_valid = empty_map()
    s0 = fr.source(e_disp, e_valid, hand_plan(), np.asarray(pts, dtype=np.float32), filtered16=F16, min_disp16=MIN16)
    zero = rr.zero_plan(0)
    huge_f = hand_plan(fx=1e300)
    huge_t = (np.eye(3).reshape(9), np.array([1e300, -1e300, 1e300]), 1)
    nan_view = (np.full(9, np.nan), np.array([np.inf, 0.0, -np.inf]), 1)
    tiny_S = (5e-324, 0)
    srcs = [s0, map_source(m), fr.source(m, np.ones_like(m, dtype=np.uint8), zero, np.zeros((0, 3), np.float32), filtered16=F16, min_disp16=MIN16),
            fr.source(m, np.ones_like(m, dtype=np.uint8), huge_f, np.zeros((0, 3), np.float32), filtered16=F16, min_disp16=MIN16),
            map_source(m, view=huge_t, reg=(1.0, 0)), map_source(m, view=nan_view, reg=(1.0, 0)), map_source(m, view=huge_t[:2] + (1,), reg=tiny_S)]
    return _case("wild", srcs)


def hand_cases():
    return [probe_case(16), probe_case(0), owner_case(1), owner_case(2), skipped_slots_case(), count_and_cap_case(), view_and_scale_case(),
            quarter_turn_case(), wild_case()]


# ---- the rendered plane of rectify_cases.scene() in three cameras ---------------------------------------------------------------------
# Camera 3 = (R R, R t + t): camera 2 is to camera 3 what camera 1 is to camera 2, so the pairs (0, 1) and (1, 2) share one plan.
# Measured on the numpy chain (rectify_ref.rectify -> stereo_sgm_ref.stereo_sgm -> rectify_ref.cloud -> dense_fuse_ref.fuse, tol16 16,
# min_support 1, the true poses); the test asserts (a) and (c) less the margin and (b) plus it, which is for a later change of the
# texture seed (the GPU must equal the statement).
SCENE_CONSISTENT_SHARE_MEASURED = 0.9979  # 3782 of 3790: (a) source-1 points seen by source 0 that are CONSISTENT
SCENE_FUSED_RATIO_MEASURED = 0.5290       # 4248 of 4012 + 4018: (b) the fused total over the sum of the parts
SCENE_SUPPORTED_SHARE_MEASURED = 1.0      # 3692 of 3692: (c) rectify_cases.scene_depth_error_share of the kept points with support >= 2
SCENE_ORPHANS_MEASURED = 0              # (d) dropped duplicates whose pixel in the lower source holds no kept point (reported only)
SCENE_MARGIN = rc.SCENE_SHARE_MARGIN


def scene3():
    """(img1, img2, img3) uint8 [72, 96]: rectify_cases.scene() and the same plane in the third camera."""
    img1, img2 = rc.scene()
    Wd, Hd = rc.SCENE_SIZE
    f, _, cx, cy = rc.SCENE_CAMERA
    n, d = rc.SCENE_PLANE
    R, t = rc.SCENE_R @ rc.SCENE_R, rc.SCENE_R @ rc.SCENE_T + rc.SCENE_T
    tex = rc._texture(rc.SCENE_SEED)
    u, v = np.meshgrid(np.arange(Wd, dtype=np.float64), np.arange(Hd, dtype=np.float64))
    rays = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], axis=-1)
    dirs = rays @ R
    origin = -(R.T @ t)
    lam = (d - n @ origin) / (dirs @ n)
    X = origin + lam[..., None] * dirs
    return img1, img2, np.clip(np.rint(rc._tex_at(tex, X[..., 0], X[..., 1])), 0, 255).astype(np.uint8)


SCENE_VIEWS = ((np.eye(3).reshape(9), np.zeros(3), 1), (np.ascontiguousarray(rc.SCENE_R).reshape(9), np.asarray(rc.SCENE_T, dtype=np.float64), 1))


def scene_sources():
    """The statement's chain on the pairs (0, 1) and (1, 2) with the true poses -> two sources in camera 1's frame."""
    import stereo_sgm_ref
    imgs = scene3()
    P = rr.make_plan(rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, rc.SCENE_SIZE)
    f16 = (rc.SCENE_SGM["min_disparity"] - 1) * 16
    out = []
    for a in (0, 1):
        r1, v1 = rr.rectify(imgs[a], rc.SCENE_CAMERA, None, P, 1)
        r2, _ = rr.rectify(imgs[a + 1], rc.SCENE_CAMERA, None, P, 2)
        disp, _ = stereo_sgm_ref.stereo_sgm(r1, r2, **rc.SCENE_SGM)
        G = SCENE_VIEWS[a]
        xyz, col, _ = rr.cloud(disp, v1, r1, P, f16, 16, 1.0, (G[0], G[1]))
        out.append(fr.source(disp, v1, P, xyz, color=col.reshape(-1, 1), filtered16=f16, min_disp16=16, view=G, reg=(1.0, 0)))
    return out


def scene_figures(sources, fused=None):
    """(a), (b), (c), (d) of two scene sources under the statement."""
    fused = fr.fuse(sources) if fused is None else fused
    n1 = fr.n_points(sources[1])
    l = fr.look(sources[0], sources[1]["xyz"][:n1], 16)
    a = float(np.mean(l[l != fr.UNSEEN] == fr.CONSISTENT))
    b = float(fused["counts"][-1]) / float(fr.n_points(sources[0]) + n1)
    c = rc.scene_depth_error_share(fused["points"][fused["support"] >= 2])
    # (d): where each dropped point of source 1 falls in source 0's map, and whether source 0 kept the point of that pixel
    dec = fr.decide(sources, fr.default_neighbors(2))
    dropped = sources[1]["xyz"][:n1][(l == fr.CONSISTENT) & ~dec[1][2]]
    kept0 = _kept_pixels(sources[0], dec[0][2])
    ui, vi = _project(sources[0], dropped)
    d = int((~kept0[vi, ui]).sum())
    return a, b, c, d


def _kept_pixels(s, kept):
    d = s["disp16"].astype(np.int64)
    is_pt = (d != s["filtered16"]) & (d >= s["min_disp16"]) & (s["valid"] != 0)
    out = np.zeros(d.shape, bool)
    v, u = np.nonzero(is_pt)
    out[v[:len(kept)], u[:len(kept)]] = kept
    return out


def _project(s, xyz):
    p = np.asarray(s["plan"]).reshape(-1)[0]
    GR, Gt = np.asarray(s["view"][0]).reshape(3, 3), np.asarray(s["view"][1])
    r = (xyz.astype(np.float64) @ GR.T + Gt) @ p["R1"].reshape(3, 3).T
    return (np.rint(p["fx"] * r[:, 0] / r[:, 2] + p["cx"]).astype(np.int64), np.rint(p["fy"] * r[:, 1] / r[:, 2] + p["cy"]).astype(np.int64))


# ---- a case as the file tests/cpp/dense_fuse_host.cpp and tests/cpp/dense_fuse_shim_main.cpp read, and a result as the former writes -----
VIEW_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("registered", "<i4"), ("pair", "<i4")])
REG_DTYPE = np.dtype([("r", "<f8"), ("S", "<f8"), ("n_links", "<i4"), ("depth", "<i4"), ("link", "<i4"), ("role", "<i4"), ("status", "<i4"),
                      ("reserved", "<i4")])


def view_record(view):
    G = np.zeros(1, VIEW_DTYPE)
    if view is not None:
        G["R"][0], G["t"][0], G["registered"], G["pair"] = view[0], view[1], view[2], -1
    return G


def reg_record(reg):
    r = np.zeros(1, REG_DTYPE)
    if reg is not None:
        r["S"], r["status"] = reg
    return r


def case_bytes(case, total_cap):
    nb = case["neighbors"]
    cap = total_cap if case["fused_cap"] is None else case["fused_cap"]
    out = [np.array([len(case["sources"]), nb.shape[1], case["channels"], case["tol16"], case["min_support"], cap], np.int32).tobytes(), nb.tobytes()]
    for s in case["sources"]:
        h, w = s["disp16"].shape
        out.append(np.array([w, h, s["filtered16"], s["min_disp16"], len(s["xyz"]), s["count"], s["color"] is not None, s["view"] is not None,
                             s["reg"] is not None], np.int32).tobytes())
        out += [np.asarray(s["plan"]).tobytes(), view_record(s["view"]).tobytes(), reg_record(s["reg"]).tobytes(), s["disp16"].tobytes(),
                s["valid"].tobytes(), s["xyz"].tobytes()]
        if s["color"] is not None:
            out.append(s["color"].tobytes())
    return b"".join(out)


def result_bytes(want, channels=None):
    return b"".join(np.ascontiguousarray(want[k]).tobytes() for k in ("counts", "points", "colors", "source", "index", "support", "conflict"))
