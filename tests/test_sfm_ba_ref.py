"""CPU: the bundle adjustment statement (tests/sfm_ba_ref.py) -- its Jacobians against central differences of its own
residual, the five-view scene with ground-truth poses through the CPU two-view chain and the registration statement (without noise and
with half a pixel of it), what the order of the sums is worth on every hand-made case (tests/sfm_ba_cases.py) against the table the GPU
test's tolerances come from, what each case is there for -- the structural ones too: a second scan tile, more than 256 frames, more
frames than cloud entries, a cloud_cap past n_tracks, the sorted-neighbour test, KEPT for two reasons, dropped steps, both ends of
conjugate gradients and of the outer loop, records that do not fit the arrays --, the host build of sfm_ba_core.h
(tests/cpp/sfm_ba_host.cpp), and the C ABI's host-only parts."""
import ctypes as C

import numpy as np
import pytest

import sfm_ba_cases as cases
import sfm_ba_ref as B
import sfm_ref
import sfm_register_ref as R
from test_sfm_register_ref import check_against_truth, close, truth_scene
import hostbuild as hb

HOST_SRC = "sfm_ba_host.cpp"
CASE_NAMES = sorted(cases.CASES)

# What the order of the observations inside every sum is worth (DESIGN.md §4.10c has the measured values): per case the largest
# difference between the statement as written and with every sum reversed, over views, points (relative to max(|value|, 1)) and cost
# (relative). MEASURED_SPREAD holds the measurements (the second digit rounded up). The GPU is held to 16 times the measurement,
# with a floor of 1e-12. The CPU test, which measures again, allows the next power of ten above three times the entry, so that
# another numpy build's rounding does not trip it; that headroom is the CPU test's alone.
MEASURED_SPREAD = {"as_is": 0.0, "behind": 5.9e-16, "multi": 2.3e-14, "outlier_huber": 3.0e-14, "outlier_plain": 8.2e-14,
                   "retriangulate_only": 2.4e-14, "small_cap": 3.8e-14, "three_chain": 2.4e-14, "twelve_frames": 2.8e-14, "two_frames": 2.6e-14,
                   "unregistered": 2.8e-14, "wide": 8.0e-15, "five_views_noisy": 9.5e-15,
                   "two_tiles": 4.2e-15, "many_frames": 2.0e-12, "frames_past_cap": 1.5e-12, "cap_past_tracks": 2.4e-14, "multi_sorted": 4.8e-15,
                   "kept": 2.5e-13, "misfit_records": 2.4e-14, "rejected_step": 1.1e-13, "cg_short": 2.2e-14, "cg_converges": 2.2e-14,
                   "ftol_stops": 7.3e-13, "iters_run_out": 7.3e-13}


def tolerance(name):
    """What the device is held to on a hand-made case: 16 times the measured order spread, at least 1e-12."""
    return max(16.0 * MEASURED_SPREAD[name], 1e-12)


def cpu_guard(name):
    """What the CPU test lets its own measurement of the spread be: the next power of ten above three times the table's entry."""
    m = MEASURED_SPREAD[name]
    return 0.0 if m == 0 else 10.0 ** np.ceil(np.log10(3.0 * m))


def run_statement(c, **kw):
    """The statement on a case: n_tracks is the registration summary's, total_m the case's own where it states one."""
    reg = c["reg"]
    return B.bundle_adjust(cases.xy_of(c["kp"]), c["frame_off"], c["pairs"], c["matches"], c["mask"], reg["views"], reg["registration"],
                           reg["track"], reg["cloud"], reg["cloud_id"], c["camera"], n_tracks=int(reg["summary"]["n_tracks"][0]),
                           total_m=c.get("total_m"), **dict(c["params"], **kw))


def spread(a, b):
    """The largest difference between two results: views and points relative to max(|value|, 1), the costs relative."""
    def rel(x, y, floor):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return float((np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), floor)).max()) if x.size else 0.0
    sa, sb = a["ba_summary"][0], b["ba_summary"][0]
    return max(rel(a["views_ba"]["R"], b["views_ba"]["R"], 1.0), rel(a["views_ba"]["t"], b["views_ba"]["t"], 1.0), rel(a["cloud_ba"], b["cloud_ba"], 1.0),
               *(rel(sa[k], sb[k], 1e-300) for k in ("cost0", "cost", "rms0_px", "rms_px")))


def same_result(got, want, tol, what=""):
    """Integers exact -- statuses, counts, the accepted iterations --; views, points and costs within tol in close()'s sense. cg_iters
    is not held: conjugate gradients stop at a threshold on r.z, which an ill-conditioned case ("behind") crosses one iteration
    sooner or later with the order of the sums."""
    assert np.array_equal(got["track_status"], want["track_status"]), what
    gs, ws = got["ba_summary"][0], want["ba_summary"][0]
    for k in ("n_obs", "n_active", "n_tracks_used", "n_tracks_multi", "n_frames_free", "iters_run", "iters_accepted", "status", "reserved"):
        assert gs[k] == ws[k], (what, k, gs, ws)
    for k in ("registered", "pair"):
        assert np.array_equal(got["views_ba"][k], want["views_ba"][k]), (what, k)
    assert close(got["views_ba"]["R"], want["views_ba"]["R"], tol, 1.0) and close(got["views_ba"]["t"], want["views_ba"]["t"], tol, 1.0), what
    assert close(got["cloud_ba"], want["cloud_ba"], tol, 1.0), what
    for k in ("cost0", "cost", "rms0_px", "rms_px", "lambda"):
        assert close(gs[k], ws[k], tol), (what, k, gs, ws)


@pytest.fixture(scope="module")
def statement_of():
    done = {}

    def get(name):
        if name not in done:
            tr = []
            done[name] = dict(run_statement(cases.case(name), trace=tr), accepts=[x[0] for x in tr], trace=tr)
        return done[name]
    return get


# ---- the Jacobians --------------------------------------------------------------------------------------------------------------------
def test_jacobians_against_central_differences():
    rng = np.random.default_rng(3)
    n, f = 50, 795.0
    Rm = np.stack([B.rodrigues(rng.normal(0, 0.2, 3)) for _ in range(n)])
    t, X = rng.normal(0, 0.5, (n, 3)), np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 9, n)], 1)
    uv = rng.normal(0, 0.2, (n, 2))
    Pc, act, r = B.project(Rm, t, X, uv, f)
    assert act.all()
    Jc, Jp = B.jacobians(Rm, t, Pc, act, f)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        rp = B.project(np.stack([B.rodrigues(d[:3]) @ M for M in Rm]), t + d[3:], X, uv, f)[2]
        rm = B.project(np.stack([B.rodrigues(-d[:3]) @ M for M in Rm]), t - d[3:], X, uv, f)[2]
        assert np.abs((rp - rm) / (2 * h) - Jc[:, :, k]).max() < 1e-5 * np.abs(Jc).max()
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        num = (B.project(Rm, t, X + d, uv, f)[2] - B.project(Rm, t, X - d, uv, f)[2]) / (2 * h)
        assert np.abs(num - Jp[:, :, k]).max() < 1e-5 * np.abs(Jp).max()
    X[0, 2] = -5.0                                            # behind: inactive, zero residual and Jacobians
    Pc, act, r = B.project(Rm, t, X, uv, f)
    Jc, Jp = B.jacobians(Rm, t, Pc, act, f)
    assert not act[0] and not r[0].any() and not Jc[0].any() and not Jp[0].any() and act[1:].all()


def test_rodrigues_and_the_small_solves():
    w = np.array([0.3, -0.2, 0.5])
    E = B.rodrigues(w)
    assert np.abs(E @ E.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(E) - 1) < 1e-15 and np.abs(E @ w - w).max() < 1e-15
    assert np.array_equal(B.rodrigues(np.zeros(3)), np.eye(3)) and np.abs(B.rodrigues([1e-11, 0, 0]) - np.eye(3)).max() < 2e-11
    rng = np.random.default_rng(4)
    A = rng.normal(size=(5, 3, 4))
    V = A @ np.transpose(A, (0, 2, 1))
    assert np.abs(B.inv3(V) @ V - np.eye(3)).max() < 1e-12
    assert not B.inv3(np.zeros((1, 3, 3))).any()
    A6 = rng.normal(size=(6, 9))
    M = A6 @ A6.T
    b = rng.normal(size=6)
    assert np.abs(B.chol6_solve(B.chol6(M), b) - np.linalg.solve(M, b)).max() < 1e-12 and B.chol6(-M) is None


# ---- the five-view scene --------------------------------------------------------------------------------------------------------------
def five_views(synth, noise_px):
    """make_multi_view_scene(7, 5, n_kp=400, noise_px) through the CPU two-view chain (as test_sfm_register_ref's) and the registration
    statement -> the scene, the bundle adjustment's arguments, the registration."""
    sc0, frame_pairs, pairs, matches, mask, points, tv = truth_scene(synth, None)
    sc = sc0 if noise_px == 0 else synth.make_multi_view_scene(7, 5, n_kp=400, noise_px=noise_px)
    for i, (a, b) in enumerate(frame_pairs):
        q, t = matches["queryIdx"][i * 400:(i + 1) * 400], matches["trainIdx"][i * 400:(i + 1) * 400]
        uv1 = np.stack([sc["frames"][a]["x"][q], sc["frames"][a]["y"][q]], 1)
        uv2 = np.stack([sc["frames"][b]["x"][t], sc["frames"][b]["y"][t]], 1)
        r = sfm_ref.two_view(uv1, uv2, sc["camera"], None, 0.7, 1.0, 1000)
        assert r["E"] is not None
        k = int((r["mask"] != 0).sum())
        tv[i]["R"], tv[i]["t"], tv[i]["n_points"], tv[i]["n_triangulated"] = r["R"], np.asarray(r["t"]).reshape(3), 400, k
        mask[i * 400:(i + 1) * 400] = r["mask"]
        points[i * 400:i * 400 + k] = r["points"]
    frame_off = np.arange(6, dtype=np.int64) * 400
    reg = R.register(frame_off, pairs, matches, mask, points, tv)
    xy = np.concatenate([np.stack([fr["x"], fr["y"]], 1) for fr in sc["frames"]]).astype(np.float32)
    cam = tuple(sc["camera"]) + (0.0,) * 5
    args = (xy, frame_off, pairs, matches, mask, reg["views"], reg["registration"], reg["track"], reg["cloud"], reg["cloud_id"], cam)
    return sc, args, reg


def centre_error(sc, views):
    """The worst camera-centre error, in first baselines (as check_against_truth measures it)."""
    Rt, tt = sc["R"], sc["t"]
    c_true = np.array([-Rt[f].T @ tt[f] for f in range(5)])
    base = np.linalg.norm(c_true[1] - c_true[0])
    centres = R.camera_centres(views)
    return max(np.linalg.norm(centres[f] - Rt[0] @ (c_true[f] - c_true[0]) / base) for f in range(5))


def test_five_views_without_noise_stay_on_the_truth(synth):
    sc, args, reg = five_views(synth, 0.0)
    out = B.bundle_adjust(*args)
    s = out["ba_summary"][0]
    print("five views, no noise:", s, "centre error", centre_error(sc, reg["views"]), "->", centre_error(sc, out["views_ba"]))
    check_against_truth(sc, dict(reg, views=out["views_ba"]))
    assert s["cost"] <= s["cost0"] and s["n_frames_free"] == 4 and s["n_tracks_used"] > 300 and s["status"] == 0


def test_five_views_with_half_a_pixel_of_noise_come_closer_to_the_truth(synth):
    sc, args, reg = five_views(synth, 0.5)
    tr, tr_rev = [], []
    out = B.bundle_adjust(*args, trace=tr)
    rev = B.bundle_adjust(*args, order=-1, trace=tr_rev)
    s = out["ba_summary"][0]
    before, after = centre_error(sc, reg["views"]), centre_error(sc, out["views_ba"])
    print("five views, 0.5 px:", s, "centre error", before, "->", after, "order spread", spread(out, rev))
    assert s["cost"] <= s["cost0"] and after < before
    assert [x[0] for x in tr] == [x[0] for x in tr_rev] and spread(out, rev) <= cpu_guard("five_views_noisy")


# ---- the hand-made cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_order_of_the_sums_on_hand_made_cases(statement_of, name):
    """Both orders take the same accept / reject sequence and agree within the table's spread; and what each case is there for."""
    c = cases.case(name)
    tr = []
    rev = run_statement(c, order=-1, trace=tr)
    out = statement_of(name)
    s = out["ba_summary"][0]
    sp = spread(out, rev)
    print(name, "order spread", sp, s)
    assert sp <= cpu_guard(name), (name, sp)
    for k in ("n_obs", "n_active", "n_tracks_used", "n_tracks_multi", "iters_run", "iters_accepted"):
        assert s[k] == rev["ba_summary"][0][k], k
    assert np.array_equal(out["track_status"], rev["track_status"]) and s["cost"] <= s["cost0"]
    assert out["accepts"] == [x[0] for x in tr] and len(tr) == s["iters_run"]


def test_what_the_cases_are_there_for(statement_of):
    s = {n: statement_of(n)["ba_summary"][0] for n in CASE_NAMES}
    assert s["two_frames"]["n_frames_free"] == 1 and s["two_frames"]["n_tracks_used"] == 8 and s["two_frames"]["iters_accepted"] > 0
    v = statement_of("two_frames")["views_ba"][1]
    assert abs(np.linalg.norm(v["R"].T @ v["t"]) - 1) < 1e-12                       # the gauge: the first baseline is 1
    lens = np.bincount([len(x) for x in statement_of("three_chain")["lists"]])
    assert lens[2] == 20 and lens[3] == 20
    assert s["twelve_frames"]["n_frames_free"] == 11
    assert s["wide"]["n_tracks_used"] == 700 and s["wide"]["n_obs"] == 2100
    m = statement_of("multi")
    assert s["multi"]["n_tracks_multi"] == 1 and (m["track_status"] == B.MULTI).sum() == 1
    e = int(np.nonzero(m["track_status"] == B.MULTI)[0][0])
    assert m["cloud_ba"][e].tobytes() == cases.case("multi")["reg"]["cloud"][e].tobytes() and len(m["lists"][e]) == 6
    b0 = run_statement(cases.case("behind"), n_iters=0)["ba_summary"][0]
    assert b0["n_obs"] == 100 and b0["n_active"] == 99
    u = statement_of("unregistered")
    assert not u["views_ba"][3]["R"].any() and not u["views_ba"][3]["t"].any() and u["views_ba"][3]["registered"] == 0
    assert len(statement_of("small_cap")["track_status"]) == 20 and s["small_cap"]["n_tracks_used"] == 20
    assert s["outlier_huber"]["cost0"] < s["outlier_plain"]["cost0"] and s["outlier_plain"]["rms0_px"] > 2.0
    a, c = statement_of("as_is"), cases.case("as_is")
    assert a["views_ba"].tobytes() == c["reg"]["views"].tobytes() and a["cloud_ba"].tobytes() == c["reg"]["cloud"].tobytes()
    assert s["retriangulate_only"]["iters_run"] == 0 and s["retriangulate_only"]["cost0"] < s["as_is"]["cost0"]
    # -- the structural edges: a second scan tile, a second pass over the frames, frames past the cloud, a cap past the tracks
    tt = statement_of("two_tiles")
    assert len(tt["track_status"]) >= 4200 and s["two_tiles"]["n_tracks_used"] == len(tt["track_status"]) == 4300
    assert (tt["track_status"][[0, 4095, 4096, 4299]] == B.REFINED).all() and min(len(x) for x in tt["lists"]) >= 2
    mf, cm = statement_of("many_frames"), cases.case("many_frames")
    assert s["many_frames"]["n_frames_free"] == cases.MANY_FRAMES - 1 > 256 and s["many_frames"]["n_active"] == s["many_frames"]["n_obs"] > 0
    assert run_statement(cm, n_iters=0, retriangulate=0)["ba_summary"][0]["n_active"] == s["many_frames"]["n_obs"]   # and at the registration's points
    assert max(len(x) for x in mf["lists"]) == 7 and (cm["params"]["n_iters"], cm["params"]["n_cg"]) == (3, 10)
    assert all(len(x) == cases.MANY_FRAMES - 1 for x in mf["factors"]) and [x[5] for x in mf["trace"]] == ["n_cg"] * 3
    fp, cf = statement_of("frames_past_cap"), cases.case("frames_past_cap")
    n_frames = len(cf["frame_off"]) - 1
    assert len(cf["reg"]["cloud_id"]) == cases.FRAMES_PAST_CAP < n_frames and cases.FRAMES_PAST_CAP <= 256 and s["frames_past_cap"]["n_frames_free"] == n_frames - 1
    seen_by = np.unique(np.searchsorted(cf["frame_off"], np.nonzero(fp["kp_track"] >= 0)[0], side="right") - 1)
    for has in fp["factors"]:   # chol6 gave None for every free frame without an observation, and a factor for the others
        assert 0 < len(has) < n_frames - 1 and np.array_equal(has, seen_by[seen_by > 0])
    assert B.chol6(np.zeros((6, 6))) is None and fp["views_ba"][n_frames - 1]["R"].tobytes() == cf["reg"]["views"][n_frames - 1]["R"].tobytes()
    cp, cc, tc = statement_of("cap_past_tracks"), cases.case("cap_past_tracks"), statement_of("three_chain")
    n_real = cc["n_real"]
    assert n_real == int(cc["reg"]["summary"]["n_tracks"][0]) == 40 and len(cp["track_status"]) == 90
    assert (cp["track_status"][n_real:] == B.FEW).all() and cp["cloud_ba"][n_real:].tobytes() == cc["reg"]["cloud"][n_real:].tobytes()
    assert (cc["reg"]["cloud"][n_real:] == cases.CAP_FILL).all() and (np.diff(cc["reg"]["cloud_id"][n_real:]) < 0).any()
    assert np.isin(cc["reg"]["cloud_id"][n_real:], cc["reg"]["cloud_id"][:n_real]).all()
    assert cp["cloud_ba"][:n_real].tobytes() == tc["cloud_ba"].tobytes() and cp["views_ba"].tobytes() == tc["views_ba"].tobytes()
    assert np.array_equal(cp["track_status"][:n_real], tc["track_status"]) and cp["ba_summary"].tobytes() == tc["ba_summary"].tobytes()
    # (without n_tracks the padding is searched too, and the repeated ids send observations elsewhere)
    loose = B.observations(cc["frame_off"], cc["pairs"], cc["matches"], cc["mask"], cc["reg"]["views"], cc["reg"]["registration"], cc["reg"]["track"],
                           cc["reg"]["cloud_id"])
    assert not np.array_equal(loose, cp["kp_track"])
    # -- the sorted-neighbour test, KEPT, a dropped step
    ms, cs = statement_of("multi_sorted"), cases.case("multi_sorted")
    e = cs["entry"]
    assert len(cs["frame_off"]) - 1 == 4 and s["multi_sorted"]["n_tracks_multi"] == 1 and np.nonzero(ms["track_status"] == B.MULTI)[0].tolist() == [e]
    fr = np.searchsorted(cs["frame_off"], ms["lists"][e], side="right") - 1
    assert fr.tolist() == [1, 1, 2] and ms["cloud_ba"][e].tobytes() == cs["reg"]["cloud"][e].tobytes()   # n = 3 <= n_frames = 4
    for w in cs["whole"]:
        assert (np.searchsorted(cs["frame_off"], ms["lists"][w], side="right") - 1).tolist() == [0, 1, 2, 3] and ms["track_status"][w] == B.REFINED
    kt, ck = statement_of("kept"), cases.case("kept")
    assert ck["params"].get("retriangulate", 1) == 1 and kt["kept_why"] == {ck["behind"]: "behind", ck["singular"]: "singular"}
    assert np.nonzero(kt["track_status"] == B.KEPT)[0].tolist() == sorted([ck["behind"], ck["singular"]])
    assert s["kept"]["n_tracks_used"] == len(kt["track_status"]) == 41 and s["kept"]["n_obs"] == 102
    k0 = run_statement(ck, n_iters=0)   # the registration's point is where they start from
    for e in (ck["behind"], ck["singular"]):
        assert k0["cloud_ba"][e].tobytes() == ck["reg"]["cloud"][e].tobytes()
    assert (k0["cloud_ba"][k0["track_status"] == B.REFINED] != ck["reg"]["cloud"][k0["track_status"] == B.REFINED]).any(1).all()
    rs = statement_of("rejected_step")
    assert rs["accepts"] == [False] * 7 + [True] * 3 and s["rejected_step"]["iters_accepted"] == 3
    for accept, cost, c_new, lam, _, _ in rs["trace"][:7]:   # dropped for the cost alone, and by far
        assert not accept and c_new > 1.5 * cost and cost == rs["trace"][0][1]
    assert [x[3] for x in rs["trace"][:8]] == pytest.approx([1e-9 * 10.0 ** k for k in range(8)], rel=1e-12) and s["rejected_step"]["n_active"] == 100
    # -- how conjugate gradients and the outer loop end (cg_iters by both orders of the sums: test_cg_iters_of_the_cg_cases_by_both_orders)
    assert [x[4:] for x in statement_of("cg_short")["trace"]] == [(2, "n_cg")] * 10 and s["cg_short"]["cg_iters"] == 20
    cv = statement_of("cg_converges")["trace"]
    assert all(x[5] == "cg_tol" and 0 < x[4] < 40 for x in cv) and s["cg_converges"]["cg_iters"] == sum(x[4] for x in cv) == 160
    assert all(x[5] == "cg_tol" for x in statement_of("twelve_frames")["trace"]) and s["twelve_frames"]["cg_iters"] == 257
    assert s["ftol_stops"]["iters_run"] == 3 < B.PARAMS["n_iters"] and cases.case("ftol_stops")["params"] == dict(ftol=1e-3)
    assert s["iters_run_out"]["iters_run"] == 3 == cases.case("iters_run_out")["params"]["n_iters"] and s["iters_run_out"]["iters_accepted"] == 3
    last = statement_of("iters_run_out")["trace"][-1]
    assert last[1] - last[2] > 0.0 and last[1] - last[2] <= 1e-3 * last[1]   # ftol = 0 did not stop it; ftol = 1e-3 stops at this very step
    # -- records that do not fit
    mr, cr = statement_of("misfit_records"), cases.case("misfit_records")
    assert len(cr["pairs"]) == 7 and (cr["reg"]["registration"]["status"] == 0).all() and cr["total_m"] == len(cr["mask"])
    for k in ("views_ba", "cloud_ba", "track_status", "ba_summary", "kp_track"):
        assert np.asarray(mr[k]).tobytes() == np.asarray(tc[k]).tobytes(), k


def cg_iters_by_both_orders(name):
    """cg_iters of a case by the statement as written and with every sum reversed: what the device's count must lie between (and
    equal, where the two agree)."""
    c = cases.case(name)
    return tuple(int(run_statement(c, order=o)["ba_summary"][0]["cg_iters"]) for o in (1, -1))


def test_cg_iters_of_the_cg_cases_by_both_orders():
    """cg_short: n_cg = 2 ends every one of the 10 solves, whatever the order. cg_converges: the threshold ends each; the order of the
    sums may move a crossing by an iteration, here it does not."""
    assert cg_iters_by_both_orders("cg_short") == (20, 20)
    a, b = cg_iters_by_both_orders("cg_converges")
    print("cg_converges: cg_iters", a, "and with the sums reversed", b)
    assert a == 160 and abs(a - b) <= 6


# ---- the host build -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(HOST_SRC)
    lib = C.CDLL(so)
    vp, dbl = C.c_void_p, C.c_double
    lib.sba_host_observation.argtypes = [vp, vp, vp, dbl, dbl, dbl, dbl, vp, vp, vp, vp, vp, vp]
    lib.sba_host_rodrigues.argtypes = [vp, vp]
    lib.sba_host_inv3.argtypes = [vp, vp]
    lib.sba_host_solve6.argtypes = [vp, vp, vp]
    lib.sba_host_triangulate.argtypes = [vp, vp, vp, C.c_int, vp]
    lib.sba_host_params_ok.argtypes = [vp]
    return lib


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_build_of_the_core_equals_the_statement(host, name):
    """Every observation of the case at the registration's views and cloud: residual, Jacobians, Huber's weight and cost; and every
    track's re-triangulated point."""
    c = cases.case(name)
    reg = c["reg"]
    kp_track = B.observations(c["frame_off"], c["pairs"], c["matches"], c["mask"], reg["views"], reg["registration"], reg["track"], reg["cloud_id"],
                              int(reg["summary"]["n_tracks"][0]), c.get("total_m"))
    g = np.nonzero(kp_track >= 0)[0]
    fr, tc = np.searchsorted(c["frame_off"], g, side="right") - 1, kp_track[g]
    uv = B.undistort(c["camera"], cases.xy_of(c["kp"])[g])
    f, h = 0.5 * (c["camera"][0] + c["camera"][1]), 2.0
    Rm, t, X = np.ascontiguousarray(reg["views"]["R"][fr]), np.ascontiguousarray(reg["views"]["t"][fr]), np.ascontiguousarray(reg["cloud"][tc])
    Pc, act, r = B.project(Rm, t, X, uv, f)
    Jc, Jp = B.jacobians(Rm, t, Pc, act, f)
    w, rho = B.huber(r, h)
    assert len(g) > 0
    for i in range(len(g)):
        o = [np.zeros(3), np.zeros(2), np.zeros(12), np.zeros(6), C.c_double(), C.c_double()]
        a = host.sba_host_observation(Rm[i].ctypes.data, t[i].ctypes.data, X[i].ctypes.data, uv[i, 0], uv[i, 1], f, h, o[0].ctypes.data,
                                      o[1].ctypes.data, o[2].ctypes.data, o[3].ctypes.data, C.byref(o[4]), C.byref(o[5]))
        assert bool(a) == bool(act[i])
        assert close(o[1], r[i], 1e-12, 1e-6) and close(o[2], Jc[i].reshape(-1), 1e-12, 1.0) and close(o[3], Jp[i].reshape(-1), 1e-12, 1.0)
        assert close(o[4].value, w[i]) and close(o[5].value, rho[i], 1e-12, 1e-12)
    want = run_statement(c, n_iters=0, retriangulate=1)
    for e in np.unique(tc)[:50]:
        mine = np.nonzero(tc == e)[0]
        if want["track_status"][e] != B.REFINED:
            continue
        Xh = np.zeros(3)
        Rs, ts, uvs = np.ascontiguousarray(Rm[mine]), np.ascontiguousarray(t[mine]), np.ascontiguousarray(uv[mine])
        assert host.sba_host_triangulate(Rs.ctypes.data, ts.ctypes.data, uvs.ctypes.data, len(mine), Xh.ctypes.data) == 1
        assert close(Xh, want["cloud_ba"][e], 1e-12, 1.0)


def test_host_small_solves_and_rodrigues(host):
    rng = np.random.default_rng(6)
    for _ in range(20):
        w, E = rng.normal(0, 0.5, 3), np.zeros((3, 3))
        host.sba_host_rodrigues(w.ctypes.data, E.ctypes.data)
        assert close(E, B.rodrigues(w), 1e-14, 1.0)
        A = rng.normal(size=(3, 4))
        V, Vi = np.ascontiguousarray(A @ A.T), np.zeros((3, 3))
        assert host.sba_host_inv3(V.ctypes.data, Vi.ctypes.data) == 1 and close(Vi, B.inv3(V[None])[0], 1e-12, np.abs(Vi).max())
        A6 = rng.normal(size=(6, 8))
        M, b, x = np.ascontiguousarray(A6 @ A6.T), rng.normal(size=6), np.zeros(6)
        assert host.sba_host_solve6(M.ctypes.data, b.ctypes.data, x.ctypes.data) == 1
        assert close(x, B.chol6_solve(B.chol6(M), b), 1e-12, np.abs(x).max())
    Z, out = np.zeros((3, 3)), np.ones((3, 3))
    assert host.sba_host_inv3(Z.ctypes.data, out.ctypes.data) == 0 and not out.any()
    M = -np.eye(6)
    assert host.sba_host_solve6(M.ctypes.data, np.ones(6).ctypes.data, np.zeros(6).ctypes.data) == 0
    E = np.zeros((3, 3))
    host.sba_host_rodrigues(np.zeros(3).ctypes.data, E.ctypes.data)
    assert np.array_equal(E, np.eye(3))


def test_stand_alone_host_program_under_sanitizers():
    out = hb.run(hb.host_exe_sanitized(HOST_SRC, defines=("SBA_HOST_MAIN",)))
    assert out.returncode == 0 and out.stdout.startswith("sba_host: tiny 1 0.000000 0.000000 1 0.500000 0.250000 4.000000 1 3.000000 layout 0 bad"), \
        out.stdout + out.stderr


# ---- the C ABI's host-only parts ------------------------------------------------------------------------------------------------------
def test_dtypes_layout_and_refusals_through_the_c_abi(pkg, host):
    assert pkg.SFM_BA_PARAMS_DTYPE == B.BA_PARAMS_DTYPE and pkg.SFM_BA_SUMMARY_DTYPE == B.BA_SUMMARY_DTYPE
    assert (pkg.SFM_BA_REFINED, pkg.SFM_BA_MULTI, pkg.SFM_BA_FEW, pkg.SFM_BA_KEPT) == (B.REFINED, B.MULTI, B.FEW, B.KEPT)
    assert pkg.SFM_BA_DEFAULTS == B.PARAMS
    p = pkg.sfm_ba_params()
    assert {k: p[k][0] for k in B.PARAMS} == B.PARAMS and host.sba_host_params_ok(p.ctypes.data) == 1
    with pytest.raises(TypeError):
        pkg.sfm_ba_params(n_iter=3)
    assert host.sba_host_layout_check() == 0
    lib = pkg.load_library()
    ws = lib.gms_sfm_ba_workspace_bytes
    assert ws(0, 1, 10, 10) == 0 and ws(2, -1, 10, 10) == 0 and ws(2, 1, 2**31 - 1, 10) == 0 and ws(2, 1, 10, -1) == 0 and ws(2, 1, -1, 10) == 0 and ws((1 << 24) + 1, 1, 10, 10) == 0
    assert ws(8, 7, 16000, 8000) % 256 == 0 and ws(1, 0, 0, 0) > 0 and ws(12, 11, 1000, 500) > 184 * 1000
    # the one-shot refuses bad parameters and null pointers before it touches a device
    c = cases.case("two_frames")
    bad = [dict(n_iters=-1), dict(n_cg=0), dict(lambda0=-1.0), dict(lambda0=np.nan), dict(cg_tol=np.inf), dict(cg_tol=-1e-8), dict(ftol=np.nan),
           dict(ftol=-1.0), dict(huber_px=-2.0), dict(huber_px=np.inf)]
    for change in bad:
        assert host.sba_host_params_ok(pkg.sfm_ba_params(**change).ctypes.data) == 0, change
        with pytest.raises(pkg.GmsError) as e:
            pkg.bundleAdjust(c["kp"], c["frame_off"], c["pairs"], c["matches"], c["mask"], c["reg"], c["camera"][:4], c["camera"][4:], **change)
        assert e.value.code == -1, change
    prm, cam = pkg.sfm_ba_params(), pkg.types.make_camera(c["camera"][:4], c["camera"][4:])
    fo = np.ascontiguousarray(c["frame_off"])
    views, vout, summ = np.ascontiguousarray(c["reg"]["views"]), np.zeros(2, pkg.SFM_VIEW_DTYPE), np.zeros(1, pkg.SFM_BA_SUMMARY_DTYPE)
    good = [cam.ctypes.data, prm.ctypes.data, c["kp"].ctypes.data, fo.ctypes.data, 2, None, 0, None, None, views.ctypes.data, None, None, 0, None, None,
            0, vout.ctypes.data, None, None, summ.ctypes.data]
    for i, v in ((0, None), (1, None), (3, None), (4, 0), (6, -1), (9, None), (12, -1), (15, -1), (16, None), (19, None), (12, 5)):
        args = list(good)
        args[i] = v
        assert lib.gms_sfm_ba(*args) == -1, i
