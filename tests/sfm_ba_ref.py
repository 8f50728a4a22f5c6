"""Bundle adjustment behind the registration, stated in numpy: the library's own definition, which sfm_ba_core.h /
sfm_ba_kernels.hip compute on the device and tests/cpp/sfm_ba_host.cpp on the host.

Inputs are what gms_two_view_batch_device and gms_sfm_register_device leave: the keypoints' pixel positions `xy` ([K, 2] float32, all
frames back to back), frame_off, pairs, the survivors `matches`, `mask`, and the registration's views, registration records, track
(per match slot), cloud and cloud_id (cloud_cap entries, of which the first min(n_tracks, cloud_cap) count; n_tracks is the
registration summary's and defaults to all of them), and the camera (fx, fy, cx, cy, k1, k2, p1, p2, k3). Every sum over observations runs in ascending global keypoint index (np.add.at and np.cumsum are sequential); order=-1 runs every
one of them in descending index instead, which is how the tests measure what the order of a sum is worth."""
import numpy as np

GMS_OK, GMS_ERR_NO_MODEL = 0, -8
REFINED, MULTI, FEW, KEPT = 0, 1, 2, 3   # track_status: refined; excluded: two keypoints of a frame; excluded: fewer than two
                                         # observations; refined, but re-triangulation was refused and it started from its cloud point
PARAMS = dict(n_iters=10, n_cg=50, lambda0=1e-3, cg_tol=1e-8, ftol=1e-10, huber_px=2.0, retriangulate=1)
BA_PARAMS_DTYPE = np.dtype([("lambda0", "<f8"), ("cg_tol", "<f8"), ("ftol", "<f8"), ("huber_px", "<f8"), ("n_iters", "<i4"), ("n_cg", "<i4"),
                            ("retriangulate", "<i4"), ("reserved", "<i4")])
BA_SUMMARY_DTYPE = np.dtype([("cost0", "<f8"), ("cost", "<f8"), ("rms0_px", "<f8"), ("rms_px", "<f8"), ("lambda", "<f8"), ("n_obs", "<i8"),
                             ("n_active", "<i8"), ("n_tracks_used", "<i8"), ("n_tracks_multi", "<i8"), ("n_frames_free", "<i4"),
                             ("iters_run", "<i4"), ("iters_accepted", "<i4"), ("cg_iters", "<i4"), ("status", "<i4"), ("reserved", "<i4")])


def undistort(cam, xy):
    """cv::undistortPoints of twoview_core.h: five fixed-point iterations."""
    fx, fy, cx, cy, k1, k2, p1, p2, k3 = [float(v) for v in cam]
    x0, y0 = (xy[:, 0].astype(np.float64) - cx) / fx, (xy[:, 1].astype(np.float64) - cy) / fy
    x, y = x0.copy(), y0.copy()
    if k1 != 0 or k2 != 0 or p1 != 0 or p2 != 0 or k3 != 0:
        for _ in range(5):
            r2 = x * x + y * y
            ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (x0 - dx) * ic, (y0 - dy) * ic
    return np.stack([x, y], 1)


def rodrigues(w):
    """exp([w]x) = I + A [w]x + B [w]x^2, A = sin(th) / th, B = (sin(th / 2) / (th / 2))^2 / 2; A = 1, B = 1/2 below th^2 = 1e-20."""
    w = np.asarray(w, dtype=np.float64)
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    A, B = 1.0, 0.5
    if th2 >= 1e-20:
        th = np.sqrt(th2)
        h = np.sin(0.5 * th) / (0.5 * th)
        A, B = np.sin(th) / th, 0.5 * h * h
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * K + B * (K @ K)


def observations(frame_off, pairs, matches, mask, views, reg, track, cloud_id, n_tracks=None, total_m=None):
    """kp_track int32 [K]: the cloud entry a keypoint is an observation of, -1 otherwise. Only the first min(n_tracks, len(cloud_id))
    entries of cloud_id are searched (n_tracks: the registration summary's; what lies behind them need not be sorted). A pair whose
    frames, frame offsets or match range (inside the total_m slots of matches, mask and track; len(mask) by default) do not fit the
    arrays has no observations."""
    frame_off = np.asarray(frame_off, dtype=np.int64)
    n_frames, total_kp = len(frame_off) - 1, int(frame_off[-1])
    counts = np.diff(frame_off)
    kp_track = np.full(total_kp, -1, np.int32)
    n_c = len(cloud_id) if n_tracks is None else max(0, min(int(n_tracks), len(cloud_id)))
    ids = np.asarray(cloud_id, dtype=np.int64)[:n_c]
    total_m = len(mask) if total_m is None else int(total_m)
    for i, p in enumerate(pairs):
        a, b, off, m = int(p["frame_a"]), int(p["frame_b"]), int(p["match_off"]), int(p["m"])
        if reg[i]["status"] != GMS_OK:
            continue
        if not (0 <= a < n_frames and 0 <= b < n_frames) or m < 0 or off < 0 or off + m > total_m:
            continue
        if not views[a]["registered"] or not views[b]["registered"]:
            continue
        if min(frame_off[a], frame_off[b], counts[a], counts[b]) < 0 or max(frame_off[a + 1], frame_off[b + 1]) > total_kp:
            continue
        mk = mask[off:off + m] != 0
        rank = np.cumsum(mk) - mk
        q, t = matches["queryIdx"][off:off + m].astype(np.int64), matches["trainIdx"][off:off + m].astype(np.int64)
        for k in np.nonzero(mk & (q >= 0) & (q < counts[a]) & (t >= 0) & (t < counts[b]))[0]:
            T = int(track[off + rank[k]])
            c = int(np.searchsorted(ids, T)) if T >= 0 else len(ids)
            if c < len(ids) and ids[c] == T:
                kp_track[frame_off[a] + q[k]] = c
                kp_track[frame_off[b] + t[k]] = c
    return kp_track


def _seq(v):
    """The sum of v in order."""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def _segsum(n, idx, vals):
    out = np.zeros((n,) + vals.shape[1:])
    np.add.at(out, idx, vals)
    return out


def inv3(V):
    """Closed-form inverses of symmetric 3 x 3 matrices [n, 3, 3] (adjugate over determinant); zeros where the determinant is not a
    positive finite number."""
    a, b, c, d, e, f = V[:, 0, 0], V[:, 0, 1], V[:, 0, 2], V[:, 1, 1], V[:, 1, 2], V[:, 2, 2]
    A, B, C = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * A + b * B + c * C
    with np.errstate(all="ignore"):
        inv = np.stack([np.stack([A, B, C], 1), np.stack([B, a * f - c * c, b * c - a * e], 1), np.stack([C, b * c - a * e, a * d - b * b], 1)], 1)
        inv = inv / det[:, None, None]
    bad = ~(np.isfinite(det) & (det > 0)) | ~np.isfinite(inv).all((1, 2))
    inv[bad] = 0.0
    return inv


def chol6(M):
    """Lower Cholesky factor of a symmetric 6 x 6 matrix, or None when a pivot is not a positive finite number."""
    L = np.zeros((6, 6))
    for j in range(6):
        s = M[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        if not (np.isfinite(s) and s > 0):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            s = M[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    return L


def chol6_solve(L, b):
    y = np.zeros(6)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * x[k]
        x[i] = s / L[i, i]
    return x


def project(R, t, X, uv, f):
    """Per observation: camera point Pc [n, 3], active (finite and z > 0), residual r [n, 2] in px (0 where inactive)."""
    with np.errstate(all="ignore"):
        Pc = np.stack([R[:, i, 0] * X[:, 0] + R[:, i, 1] * X[:, 1] + R[:, i, 2] * X[:, 2] + t[:, i] for i in range(3)], 1)
        active = np.isfinite(Pc).all(1) & (Pc[:, 2] > 0)
        iz = 1.0 / np.where(active, Pc[:, 2], 1.0)
        r = f * np.stack([Pc[:, 0] * iz - uv[:, 0], Pc[:, 1] * iz - uv[:, 1]], 1)
    r[~active] = 0.0
    return Pc, active, r


def jacobians(R, t, Pc, active, f):
    """Jc [n, 2, 6] = dr / d(omega, tau) for R <- exp([omega]x) R, t <- t + tau, and Jp [n, 2, 3] = dr / dX; zeros where inactive."""
    n = len(Pc)
    z = np.where(active, Pc[:, 2], 1.0)
    iz = 1.0 / z
    x, y = Pc[:, 0] * iz, Pc[:, 1] * iz
    D = np.zeros((n, 2, 3))                       # f d(pi) / dPc
    D[:, 0, 0], D[:, 0, 2], D[:, 1, 1], D[:, 1, 2] = f * iz, -f * x * iz, f * iz, -f * y * iz
    a = Pc - t                                    # R X
    Jc = np.zeros((n, 2, 6))
    for k in range(2):                            # D (-[a]x): row k
        Jc[:, k, 0] = D[:, k, 2] * a[:, 1] - D[:, k, 1] * a[:, 2]
        Jc[:, k, 1] = D[:, k, 0] * a[:, 2] - D[:, k, 2] * a[:, 0]
        Jc[:, k, 2] = D[:, k, 1] * a[:, 0] - D[:, k, 0] * a[:, 1]
        Jc[:, k, 3:] = D[:, k]
    Jp = np.stack([np.stack([D[:, k, 0] * R[:, 0, c] + D[:, k, 1] * R[:, 1, c] + D[:, k, 2] * R[:, 2, c] for c in range(3)], 1) for k in range(2)], 1)
    Jc[~active], Jp[~active] = 0.0, 0.0
    return Jc, Jp


def huber(r, h):
    """-> (weight w, cost rho) per observation: w = 1, rho = |r|^2 up to h; w = h / |r|, rho = 2 h |r| - h^2 past it; h = 0: no weights."""
    n2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    n = np.sqrt(n2)
    if h <= 0:
        return np.ones(len(r)), n2
    far = n > h
    with np.errstate(all="ignore"):
        return np.where(far, h / np.where(far, n, 1.0), 1.0), np.where(far, 2.0 * h * n - h * h, n2)


def bundle_adjust(xy, frame_off, pairs, matches, mask, views, reg, track, cloud, cloud_id, camera, order=1, trace=None, n_tracks=None,
                  total_m=None, **params):
    """-> dict(views_ba, cloud_ba, track_status int32 per cloud entry, ba_summary BA_SUMMARY_DTYPE [1], kp_track, lists, factors = per
    outer iteration the free frames that had a Cholesky factor, kept_why = per KEPT entry what refused its re-triangulation).
    n_tracks, total_m: as observations() takes them; the entries of cloud_id past min(n_tracks, len(cloud_id)) are neither searched
    nor visited: status FEW, their rows of cloud unchanged. trace, when a list, gets per outer iteration (accepted, the cost before,
    the candidate's cost, lambda, conjugate-gradient iterations, what ended them: "rz0", "n_cg", "pq" or "cg_tol")."""
    P = dict(PARAMS, **params)
    n_iters, n_cg, lam, cg_tol, ftol, h = int(P["n_iters"]), int(P["n_cg"]), float(P["lambda0"]), float(P["cg_tol"]), float(P["ftol"]), float(P["huber_px"])
    frame_off = np.asarray(frame_off, dtype=np.int64)
    n_frames, n_c = len(frame_off) - 1, len(cloud_id)
    cam = [float(v) for v in np.asarray(camera).reshape(-1).tolist()] if not isinstance(camera, np.ndarray) or camera.dtype.names is None else \
        [float(camera.reshape(-1)[0][n]) for n in camera.dtype.names]
    f = 0.5 * (cam[0] + cam[1])
    views_out = np.array(views, copy=True)
    X = np.array(cloud, dtype=np.float64, copy=True).reshape(-1, 3)[:n_c]
    kp_track = observations(frame_off, pairs, matches, mask, views, reg, track, cloud_id, n_tracks, total_m)
    g_all = np.nonzero(kp_track >= 0)[0]
    fr_all = np.searchsorted(frame_off, g_all, side="right") - 1
    c_all = kp_track[g_all]
    status = np.full(n_c, FEW, np.int32)
    lists = [g_all[c_all == c] for c in range(n_c)]
    for c in range(n_c):
        fr = fr_all[c_all == c]
        if len(fr) and (np.diff(fr) == 0).any():
            status[c] = MULTI
        elif len(fr) >= 2:
            status[c] = REFINED
    used = status[c_all] == REFINED
    g, fr, tc = g_all[used], fr_all[used], c_all[used]            # the observations, in ascending global keypoint index
    if order < 0:
        g, fr, tc = g[::-1], fr[::-1], tc[::-1]
    uv = undistort(cam, np.asarray(xy)[g].reshape(-1, 2))
    R, t = views_out["R"].copy(), views_out["t"].copy()
    free = (views_out["registered"] != 0) & (views_out["pair"] >= 0)
    fidx = np.nonzero(free)[0]
    kept_why = {}
    # re-triangulation over all views
    if P["retriangulate"] and len(g):
        Rt = np.transpose(R[fr], (0, 2, 1))
        cen = -np.stack([Rt[:, i, 0] * t[fr][:, 0] + Rt[:, i, 1] * t[fr][:, 1] + Rt[:, i, 2] * t[fr][:, 2] for i in range(3)], 1)
        d = np.stack([Rt[:, i, 0] * uv[:, 0] + Rt[:, i, 1] * uv[:, 1] + Rt[:, i, 2] for i in range(3)], 1)
        d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
        Pm = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
        A = _segsum(n_c, tc, Pm)
        b = _segsum(n_c, tc, np.stack([Pm[:, i, 0] * cen[:, 0] + Pm[:, i, 1] * cen[:, 1] + Pm[:, i, 2] * cen[:, 2] for i in range(3)], 1))
        Ai = inv3(A)
        Xn = np.stack([Ai[:, i, 0] * b[:, 0] + Ai[:, i, 1] * b[:, 1] + Ai[:, i, 2] * b[:, 2] for i in range(3)], 1)
        Pc, act, _ = project(R[fr], t[fr], Xn[tc], uv, f)
        bad = np.zeros(n_c, bool)
        np.logical_or.at(bad, tc, ~act)
        singular = ~Ai.any((1, 2))
        bad |= ~np.isfinite(Xn).all(1) | singular
        for c in np.nonzero(status == REFINED)[0]:
            if bad[c]:
                status[c] = KEPT
                kept_why[int(c)] = "singular" if singular[c] else "behind" if np.isfinite(Xn[c]).all() else "not finite"
            else:
                X[c] = Xn[c]

    def cost_of(R, t, X):
        _, act, r = project(R[fr], t[fr], X[tc], uv, f)
        _, rho = huber(r, h)
        rho = np.where(act, rho, 0.0)
        sq = np.where(act, r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1], 0.0)
        # per frame in order, then the frames in order
        cf, sf = _segsum(n_frames, fr, rho), _segsum(n_frames, fr, sq)
        return _seq(cf), _seq(sf), int(act.sum())

    cost, sq, n_act = cost_of(R, t, X)
    cost0, sq0, n_act0 = cost, sq, n_act
    iters_run = iters_acc = cg_total = 0
    factors = []
    done = not (len(g) and len(fidx))
    for it in range(n_iters):
        if done:
            break
        iters_run += 1
        Pc, act, r = project(R[fr], t[fr], X[tc], uv, f)
        Jc, Jp = jacobians(R[fr], t[fr], Pc, act, f)
        w, _ = huber(r, h)
        sw = np.sqrt(w)
        Jc, Jp, r = Jc * sw[:, None, None], Jp * sw[:, None, None], r * sw[:, None]
        Jc[~free[fr]] = 0.0
        V = _segsum(n_c, tc, np.einsum("nki,nkj->nij", Jp, Jp))
        gp = -_segsum(n_c, tc, np.einsum("nki,nk->ni", Jp, r))
        V[:, [0, 1, 2], [0, 1, 2]] *= 1.0 + lam
        Vi = inv3(V)
        y = np.einsum("nij,nj->ni", Vi, gp)
        U = _segsum(n_frames, fr, np.einsum("nki,nkj->nij", Jc, Jc))
        gc = -_segsum(n_frames, fr, np.einsum("nki,nk->ni", Jc, r))
        Wo = np.einsum("nki,nkj->nij", Jc, Jp)                      # [n, 6, 3]
        bvec = gc - _segsum(n_frames, fr, np.einsum("nij,nj->ni", Wo, y[tc]))
        WV = np.einsum("nij,njk->nik", Wo, Vi[tc])
        E = _segsum(n_frames, fr, np.einsum("nik,njk->nij", WV, Wo))
        U[:, range(6), range(6)] *= 1.0 + lam
        Ls = {int(k): chol6(U[k] - E[k]) for k in fidx}
        factors.append(np.array([k for k in fidx if Ls[int(k)] is not None], dtype=np.int64))

        def precond(v):
            out = np.zeros_like(v)
            for k in fidx:
                if Ls[int(k)] is not None:
                    out[k] = chol6_solve(Ls[int(k)], v[k])
            return out

        def dot(a, b):
            return _seq([_seq(a[k] * b[k]) for k in fidx])

        def S_times(p):
            s2 = np.einsum("nki,ni->nk", Jc, p[fr])
            qt = np.einsum("nij,nj->ni", Vi, _segsum(n_c, tc, np.einsum("nki,nk->ni", Jp, s2)))
            s3 = np.einsum("nki,ni->nk", Jp, qt[tc])
            out = np.einsum("nij,nj->ni", U, p) - _segsum(n_frames, fr, np.einsum("nki,nk->ni", Jc, s3))
            out[~free] = 0.0
            return out

        bvec[~free] = 0.0
        x = np.zeros((n_frames, 6))
        rr = bvec.copy()
        z = precond(rr)
        p = z.copy()
        rz = rz0 = dot(rr, z)
        cg_done = not (np.isfinite(rz0) and rz0 > 0)
        cg_before, cg_end = cg_total, "rz0" if cg_done else "n_cg"   # how the solve ends: r0.z0 <= 0, n_cg used up, p.Sp, cg_tol
        for _ in range(n_cg):
            if cg_done:
                break
            q = S_times(p)
            pq = dot(p, q)
            cg_total += 1
            if not (np.isfinite(pq) and pq > 0):
                cg_end = "pq"
                break
            alpha = rz / pq
            x, rr = x + alpha * p, rr - alpha * q
            z = precond(rr)
            rz_new = dot(rr, z)
            if not np.isfinite(rz_new) or rz_new <= cg_tol * cg_tol * rz0:
                cg_end = "cg_tol"
                break
            p = z + (rz_new / rz) * p
            rz = rz_new
        # points back, the candidate and its cost
        s2 = np.einsum("nki,ni->nk", Jc, x[fr])
        dX = np.einsum("nij,nj->ni", Vi, gp - _segsum(n_c, tc, np.einsum("nki,nk->ni", Jp, s2)))
        Xc = X + dX
        Rc, tcand = R.copy(), t.copy()
        for k in fidx:
            Rc[k] = rodrigues(x[k, :3]) @ R[k]
            tcand[k] = t[k] + x[k, 3:]
        c_new, sq_new, act_new = cost_of(Rc, tcand, Xc)
        accept = bool(np.isfinite(c_new) and c_new < cost and act_new >= n_act)
        if trace is not None:
            trace.append((accept, cost, c_new, lam, cg_total - cg_before, cg_end))
        if accept:
            iters_acc += 1
            done = cost - c_new <= ftol * cost
            R, t, X, cost, sq, n_act = Rc, tcand, Xc, c_new, sq_new, act_new
            lam = max(lam / 10.0, 1e-12)
        else:
            lam = 10.0 * lam
    # the gauge: the first pair's unit, kept
    factor = 1.0
    if n_iters > 0:   # (without an outer iteration nothing is touched: n_iters = 0 copies the poses)
        first = [i for i in range(len(pairs)) if reg[i]["status"] == GMS_OK and reg[i]["link"] < 0]
        if first:
            b = int(pairs[first[0]]["frame_b"])
            cen = -np.array([R[b][0, i] * t[b][0] + R[b][1, i] * t[b][1] + R[b][2, i] * t[b][2] for i in range(3)])
            nrm = np.sqrt(cen[0] * cen[0] + cen[1] * cen[1] + cen[2] * cen[2])
            if np.isfinite(nrm) and nrm > 0:
                factor = 1.0 / nrm
    views_out["R"], views_out["t"] = R, t * factor
    cloud_out = np.array(cloud, dtype=np.float64, copy=True).reshape(-1, 3)[:n_c]
    ref = (status == REFINED) | (status == KEPT)
    cloud_out[ref] = X[ref] * factor
    s = np.zeros(1, BA_SUMMARY_DTYPE)
    s["cost0"], s["cost"], s["lambda"] = cost0, cost, lam
    s["rms0_px"], s["rms_px"] = (np.sqrt(sq0 / n_act0) if n_act0 else 0.0), (np.sqrt(sq / n_act) if n_act else 0.0)
    s["n_obs"], s["n_active"], s["n_tracks_used"], s["n_tracks_multi"] = len(g), n_act, int(ref.sum()), int((status == MULTI).sum())
    s["n_frames_free"], s["iters_run"], s["iters_accepted"], s["cg_iters"] = len(fidx), iters_run, iters_acc, cg_total
    s["status"] = GMS_OK if n_act else GMS_ERR_NO_MODEL
    return dict(views_ba=views_out, cloud_ba=cloud_out, track_status=status, ba_summary=s, kp_track=kp_track, lists=lists, factors=factors, kept_why=kept_why)
