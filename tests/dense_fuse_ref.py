"""The fusion of per-pair dense clouds as sfm-gms_amd/csrc/dense_fuse_core.h defines it, in numpy: whether a source
sees a point where its own disparity map says it is, and the rule that keeps a point once. fp64, only + - * / rint, every sum written
out in the header's order; no matrix product and no linear-algebra routine (a BLAS may fuse products into sums). The GPU, the host
build of the header and this file agree bit for bit.

A source is a dict: disp16 int16 [H, W], valid uint8 [H, W], plan (a rectify_ref.PLAN_DTYPE record), filtered16, min_disp16,
xyz float32 [cap, 3], color uint8 [cap, channels] or None, count (may exceed cap), view None or (R [9], t [3], registered),
reg None or (S, status)."""
import numpy as np

GMS_OK = 0
UNSEEN, CONSISTENT, CONFLICT = 0, 1, 2
MAX_SIDE = 8192
MAX_NEIGHBORS = 32


def source(disp16, valid, plan, xyz, count=None, color=None, filtered16=-16, min_disp16=16, view=None, reg=None):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    return dict(disp16=np.ascontiguousarray(disp16, dtype=np.int16), valid=np.ascontiguousarray(valid, dtype=np.uint8), plan=plan, xyz=xyz,
                count=len(xyz) if count is None else int(count), color=None if color is None else np.ascontiguousarray(color, dtype=np.uint8),
                filtered16=int(filtered16), min_disp16=int(min_disp16), view=view, reg=reg)


def _plan(s):
    return np.asarray(s["plan"]).reshape(-1)[0]


def is_live(s):
    H, W = s["disp16"].shape
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        return False
    if int(_plan(s)["status"]) != GMS_OK:
        return False
    if s["reg"] is not None and not (int(s["reg"][1]) == GMS_OK and float(s["reg"][0]) > 0.0):
        return False
    if s["view"] is not None and int(s["view"][2]) == 0:
        return False
    return True


def n_points(s):
    return max(0, min(int(s["count"]), len(s["xyz"]))) if is_live(s) else 0


def _round_i32(v):
    r = np.rint(v)
    with np.errstate(invalid="ignore"):
        r = np.where(~(r >= -2147483648.0), -2147483648.0, np.where(r >= 2147483647.0, 2147483647.0, r))
    return r.astype(np.int64)


def look(s, xyz, tol16):
    """fuse::look of every point of xyz (float32 [k, 3]) against the live source s -> int64 [k] of UNSEEN / CONSISTENT / CONFLICT."""
    p = _plan(s)
    R1 = [float(v) for v in np.asarray(p["R1"]).reshape(9)]
    fx, fy, cx, cy, B = (float(p[k]) for k in ("fx", "fy", "cx", "cy", "B"))
    if s["view"] is None:
        GR, Gt = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
    else:
        GR, Gt = [float(v) for v in np.asarray(s["view"][0]).reshape(9)], [float(v) for v in np.asarray(s["view"][1]).reshape(3)]
    S = 1.0 if s["reg"] is None else float(s["reg"][0])
    H, W = s["disp16"].shape
    P = [np.asarray(xyz, dtype=np.float32).reshape(-1, 3)[:, c].astype(np.float64) for c in range(3)]
    with np.errstate(all="ignore"):
        q = [((GR[3 * i] * P[0] + GR[3 * i + 1] * P[1] + GR[3 * i + 2] * P[2]) + Gt[i]) / S for i in range(3)]
        r = [R1[3 * i] * q[0] + R1[3 * i + 1] * q[1] + R1[3 * i + 2] * q[2] for i in range(3)]
        u, v = fx * (r[0] / r[2]) + cx, fy * (r[1] / r[2]) + cy
        ui, vi = _round_i32(u), _round_i32(v)
        inside = (r[2] > 0.0) & (ui >= 0) & (ui < W) & (vi >= 0) & (vi < H)
        at_v, at_u = np.where(inside, vi, 0), np.where(inside, ui, 0)
        ok = s["valid"][at_v, at_u].astype(np.int64)
        d16 = s["disp16"][at_v, at_u].astype(np.int64)
        seen = inside & (ok != 0) & (d16 != s["filtered16"]) & (d16 >= s["min_disp16"])
        e = fx * B * 16.0 / r[2]
        agree = np.abs(d16.astype(np.float64) - e) <= float(tol16)
    return np.where(seen, np.where(agree, CONSISTENT, CONFLICT), UNSEEN).astype(np.int64)


def default_neighbors(n_src):
    """Every other source, in ascending order; a lone source gets one empty slot."""
    if n_src - 1 > MAX_NEIGHBORS:
        raise ValueError("more than 32 other sources: pass neighbors")
    nb = np.full((n_src, max(n_src - 1, 1)), -1, np.int32)
    for i in range(n_src):
        nb[i, :n_src - 1] = [j for j in range(n_src) if j != i]
    return nb


def decide(sources, neighbors, tol16=16, min_support=1):
    """Per source: (support uint8 [n_i], conflict uint8 [n_i], kept bool [n_i])."""
    neighbors = np.asarray(neighbors, dtype=np.int32).reshape(len(sources), -1)
    out = []
    for i, s in enumerate(sources):
        n = n_points(s)
        support, conflict, dup = np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
        for j in neighbors[i] if n else ():
            j = int(j)
            if j < 0 or j >= len(sources) or j == i or not is_live(sources[j]):
                continue
            l = look(sources[j], s["xyz"][:n], tol16)
            support += l == CONSISTENT
            conflict += l == CONFLICT
            if j < i:
                dup |= l == CONSISTENT
        out.append((support.astype(np.uint8), conflict.astype(np.uint8), ~dup & (support >= min_support)))
    return out


def fuse(sources, neighbors=None, channels=1, tol16=16, min_support=1, fused_cap=None):
    """-> dict of points float32 [k, 3], colors uint8 [k, channels], source, index int32 [k], support, conflict uint8 [k] with
    k = min(total, fused_cap), and counts int32 [n_src + 1]: kept per source, then the total (also beyond fused_cap)."""
    if neighbors is None:
        neighbors = default_neighbors(len(sources))
    dec = decide(sources, neighbors, tol16, min_support)
    xyz, col, src, idx, sup, con, counts = [], [], [], [], [], [], []
    for i, (s, (support, conflict, kept)) in enumerate(zip(sources, dec)):
        k = np.nonzero(kept)[0]
        counts.append(len(k))
        xyz.append(s["xyz"][k])
        col.append(np.zeros((len(k), channels), np.uint8) if s["color"] is None else s["color"].reshape(len(s["xyz"]), channels)[k])
        src.append(np.full(len(k), i, np.int32))
        idx.append(k.astype(np.int32))
        sup.append(support[k])
        con.append(conflict[k])
    total = int(sum(counts))
    cap = total if fused_cap is None else min(total, int(fused_cap))
    cat = lambda parts, shape, dt: (np.concatenate(parts) if parts else np.zeros(shape, dt))[:cap]
    return dict(points=cat(xyz, (0, 3), np.float32), colors=cat(col, (0, channels), np.uint8), source=cat(src, (0,), np.int32),
                index=cat(idx, (0,), np.int32), support=cat(sup, (0,), np.uint8), conflict=cat(con, (0,), np.uint8),
                counts=np.asarray(counts + [total], dtype=np.int32))
