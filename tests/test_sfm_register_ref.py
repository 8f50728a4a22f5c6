"""CPU: the registration statement (tests/sfm_register_ref.py) -- a five-view scene with ground-truth poses through the
CPU two-view chain, hand-made records with analytically known scales (tests/sfm_register_cases.py), the tracks against
scipy.sparse.csgraph.connected_components, the host build of sfm_register_core.h (tests/cpp/sfm_register_host.cpp) and the C ABI's
gms_sfm_plan against the Python plan, and the workspace's layout (tests/cpp/sfm_register_layout_check.cpp). The cases whose records
or plan do not fit (cases.UNFIT) have tests of their own here, and the stand-alone host program hands their records to
sfr::pair_fits under the sanitizers."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import sfm_ref
import sfm_register_cases as cases
import sfm_register_ref as R
import hostbuild as hb

HOST_SRC = "sfm_register_host.cpp"
LAYOUT_SRC = "sfm_register_layout_check.cpp"
CASE_NAMES = sorted(cases.CASES)
SANE_NAMES = [name for name in CASE_NAMES if name not in cases.UNFIT]   # the pair list alone says what the device reads
# sha256 over the statement's arrays (in the order of their names) on the five cases it was first written for, as it stood before it
# learnt the kernels' rule for records that do not fit
STATEMENT_BEFORE = {"chain_roles": "ec0f73ce93fd766d829a932efc01c597e13d1524478d3a488fe7a8023745c612",
                    "invalid_links_and_min_links": "a17ee900a5c352f5c0292af44edd059efb7c0ae99acb9a34279ed86a25c34b0e",
                    "lowest_k_wins": "00077c0d6c0cb1be9debacf09121ff6ec41390ffcc828f61ddde158988488db8",
                    "many_links": "8316f24cc5ce2c7579e88dd32ca0f83351f72a8bb90bf54a608fa6b95dbc93c0",
                    "upstream_failures": "1b9de0f5f9cb13d41c45eac481a5107628384eaaeeb1099d583e71156e2620fc"}


def run_ref(c, **kw):
    """The statement on a case: a case that states a plan or the arrays' length (cases.UNFIT) hands them on."""
    kw = dict({k: c[k] for k in ("plan", "total_m") if k in c}, **kw)
    return R.register(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], **kw)


@pytest.fixture(scope="module")
def ref_of():
    done = {}

    def get(name):
        if name not in done:
            done[name] = run_ref(cases.case(name))
        return done[name]
    return get


# ---- ground truth ---------------------------------------------------------------------------------------------------------------------
def truth_scene(synth, _unused=None):
    """make_multi_view_scene(7, 5, n_kp=400, noise_px=0.0), pairs (0,1), (1,2), (2,3), (0,4), per pair 20 % of the train indices replaced by
    default_rng(1) draws. Returns the scene, the pairs and their putative matches, and empty mask / points / two-view arrays to fill."""
    sc = synth.make_multi_view_scene(7, 5, n_kp=400, noise_px=0.0)
    frame_pairs = [(0, 1), (1, 2), (2, 3), (0, 4)]
    rng = np.random.default_rng(1)
    n = 400
    pairs, tv = np.zeros(4, cases.PAIR_DTYPE), np.zeros(4, cases.TWO_VIEW_DTYPE)
    matches, mask, points = np.zeros(4 * n, cases.DMATCH_DTYPE), np.zeros(4 * n, np.uint8), np.zeros((4 * n, 3))
    for i, (a, b) in enumerate(frame_pairs):
        t = np.arange(n)
        bad = rng.choice(n, n // 5, replace=False)
        t[bad] = rng.integers(0, n, n // 5)
        pairs[i] = (a, b, n, 0, i * n)
        matches["queryIdx"][i * n:(i + 1) * n], matches["trainIdx"][i * n:(i + 1) * n] = np.arange(n), t
    return sc, frame_pairs, pairs, matches, mask, points, tv


def check_against_truth(sc, out, n_links_min=150):
    """Centres within 1e-3 of the true first baseline, rotations within 1e-3 degrees, every pair ok, every linked pair with at least
    n_links_min links."""
    Rt, tt = sc["R"], sc["t"]
    c_true = np.array([-Rt[f].T @ tt[f] for f in range(5)])
    base = np.linalg.norm(c_true[1] - c_true[0])
    reg, views = out["registration"], out["views"]
    assert (reg["status"] == 0).all() and (views["registered"] == 1).all()
    assert (reg["n_links"][reg["link"] >= 0] >= n_links_min).all(), reg["n_links"]
    centres = R.camera_centres(views)
    worst_c = worst_r = 0.0
    for f in range(5):
        want_c = Rt[0] @ (c_true[f] - c_true[0]) / base       # in camera 0's frame, in units of the first baseline
        want_R = Rt[f] @ Rt[0].T
        worst_c = max(worst_c, np.linalg.norm(centres[f] - want_c))
        cos = (np.trace(views[f]["R"] @ want_R.T) - 1) / 2
        worst_r = max(worst_r, np.degrees(np.arccos(np.clip(cos, -1, 1))))
    print(f"n_links {reg['n_links'].tolist()}, S {reg['S'].tolist()}, centre error {worst_c:.3g} baselines, rotation error {worst_r:.3g} degrees")
    assert worst_c < 1e-3 and worst_r < 1e-3


def test_five_views_against_ground_truth(synth):
    sc, frame_pairs, pairs, matches, mask, points, tv = truth_scene(synth, None)
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
    out = R.register(frame_off, pairs, matches, mask, points, tv)
    assert out["plan"]["link"].tolist() == [-1, 0, 1, 0] and out["plan"]["role"].tolist() == [0, 1, 1, 0]
    check_against_truth(sc, out)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_plan_by_hand():
    p = R.plan([(0, 1), (1, 2), (2, 1), (0, 3), (3, 1), (5, 6), (0, 0), (3, 4), (0, 5)], 7)
    assert p["registers"].tolist() == [1, 1, 0, 1, 0, 0, 0, 1, 1]
    assert p["link"].tolist() == [-1, 0, -1, 0, -1, -1, -1, 3, 0]
    assert p["role"].tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0]
    assert p["depth"].tolist() == [0, 1, 0, 1, 0, 0, 0, 2, 1]
    p = R.plan([(0, 1), (2, 0), (2, 3), (0, 1)], 4, root=2)             # the first pair waits for a frame that comes later: skipped
    assert p["registers"].tolist() == [0, 1, 1, 1] and p["link"].tolist() == [-1, -1, 1, 1] and p["role"].tolist() == [0, 0, 0, 1]
    for bad in ([(0, 7)], [(-1, 0)]):
        with pytest.raises(ValueError):
            R.plan(bad, 7)
    with pytest.raises(ValueError):
        R.plan([(0, 1)], 2, root=2)


# ---- hand-made records ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SANE_NAMES)
def test_hand_made_records_have_the_stated_scales(ref_of, name):
    c, out = cases.case(name), ref_of(name)
    reg = out["registration"]
    assert set(c["expect"]) == set(range(len(reg)))
    for i, (status, n_links, S) in c["expect"].items():
        assert reg[i]["status"] == status, (i, reg[i])
        if n_links is not None:
            assert reg[i]["n_links"] == n_links, (i, reg[i])
        assert abs(reg[i]["S"] - S) <= 1e-12 * S, (i, reg[i])
    # the views of the ok pairs are the true ones in the root's frame (every case's first unit is 1), the others stay unregistered
    truth = cases.truth_views(c)
    registered = {c["root"]} | {int(c["pairs"][i]["frame_b"]) for i in range(len(reg)) if reg[i]["status"] == 0}
    for f, v in enumerate(out["views"]):
        assert bool(v["registered"]) == (f in registered)
        if f in registered:
            assert np.abs(v["R"] - truth[f][0]).max() < 1e-12 and np.abs(v["t"] - truth[f][1]).max() < 1e-11
        else:
            assert not v["R"].any() and not v["t"].any() and v["pair"] == -1
    # world points of the ok pairs: the scene in the root's frame; slots that hold no point are 0 / -1
    world, track = out["points_world"], out["track"]
    owned = np.zeros(len(world), bool)
    for i in np.nonzero(reg["status"] == 0)[0]:
        o, k = int(c["pairs"][i]["match_off"]), int(c["tv"][i]["n_triangulated"])
        owned[o:o + k] = True
    assert not world[~owned].any() and (track[~owned] == -1).all()
    assert out["summary"]["n_ok_pairs"][0] == int((reg["status"] == 0).sum()) and out["summary"]["n_registered"][0] == len(registered)


def test_lower_median_and_lowest_k(ref_of):
    """The even case: 20 ratios at the true value and 20 at 1.5 times it -- element 19 is the true one, element 20 is not. The duplicate
    case: any slot other than the lowest k triples the ratio."""
    assert R.lower_median([3.0, 1.0, 2.0, 4.0]) == 2.0 and R.lower_median([5.0]) == 5.0 and R.lower_median([1.0, 1.0, 7.0]) == 1.0
    reg = ref_of("chain_roles")["registration"]
    assert reg[1]["n_links"] == 40 and abs(reg[1]["r"] / 2.5 - 1) < 1e-12
    reg = ref_of("lowest_k_wins")["registration"]
    assert abs(reg[1]["r"] / 0.4 - 1) < 1e-12
    assert ref_of("lowest_k_wins")["summary"]["n_multi"][0] > 0     # the extra matches chain two keypoints of frame 0 into one track


def test_many_links_case_is_past_one_pass():
    c = cases.case("many_links")
    assert c["tv"]["n_points"].min() > 5000 and c["frame_off"][-1] > 3 * 4096


def test_the_statement_without_the_new_arguments_is_unchanged(ref_of):
    """plan= and total_m= left out: the five cases the statement was written for give the bytes they gave before it had them."""
    for name, before in STATEMENT_BEFORE.items():
        out = ref_of(name)
        assert "plan" not in cases.case(name) and "total_m" not in cases.case(name)
        assert hashlib.sha256(b"".join(np.ascontiguousarray(out[k]).tobytes() for k in sorted(out))).hexdigest() == before, name


def test_the_long_cases_reach_what_they_are_for(ref_of):
    """Conditions on the inputs and on the statement's outcome that the device tests rely on (DESIGN.md 4.10b names the kernel paths)."""
    for name in ("chain_300", "star_300", "two_branches_300"):
        assert len(cases.case(name)["pairs"]) == 300 > 256              # past one staging pass of the walk
    reg = ref_of("chain_300")["registration"]
    assert (reg["status"] == 0).all() and reg["depth"].tolist() == list(range(300)) and reg["link"].tolist() == list(range(-1, 299))
    out = ref_of("chain_300")
    assert out["summary"]["n_tracks"][0] == 24 and (out["cloud_obs"] == 301).all() and (out["cloud_est"] == 300).all()
    reg = ref_of("star_300")["registration"]
    assert (reg["status"] == 0).all() and (reg["link"][1:] == 0).all() and (reg["role"] == 0).all() and reg["depth"].max() == 1
    c, reg = cases.case("two_branches_300"), ref_of("two_branches_300")["registration"]
    assert reg["link"].tolist() == [-1, 0] + list(range(298)) and (c["pairs"]["frame_a"][2:] != c["pairs"]["frame_b"][1:-1]).all()
    assert int((reg["status"] == 0).sum()) == 278 and np.nonzero(reg["status"] == R.GMS_ERR_NO_MODEL)[0].tolist() == list(range(256, 300, 2))
    # tiles_past_256: more than 256 tiles of 4096 keypoints, and track ids on both sides of tile 256
    c, out = cases.case("tiles_past_256"), ref_of("tiles_past_256")
    tile = out["cloud_id"] // 4096
    assert int(c["frame_off"][-1]) == 1100185 and -(-1100185 // 4096) == 269 and out["summary"]["n_tracks"][0] == 60
    print("tiles_past_256: ids below tile 256:", int((tile < 256).sum()), "at or past it:", int((tile >= 256).sum()))
    assert (tile < 256).sum() >= 5 and (tile >= 256).sum() >= 5 and (tile < 256).sum() > 20   # (20: the small capacity of the device test)
    # ratio_spread: the ratios of each pair differ in every byte above the lowest, and the medians are the true ones
    reg = ref_of("ratio_spread")["registration"]
    assert reg["n_links"].tolist() == [0, 41, 40, 257, 63] and np.allclose(reg["r"][1:], [2.5, 0.7, 0.3, 1.7], rtol=1e-12, atol=0)
    reg = ref_of("first_root_pair_fails")["registration"]
    assert reg["status"].tolist() == [-8, -8, -8, -8, -8, 1, -8] and reg["role"][[3, 6]].tolist() == [0, 0] and not reg["r"][[3, 6]].any()


def check_expect(c, reg, expect):
    for i, (status, n_links, S) in expect.items():
        assert reg[i]["status"] == status and (n_links is None or reg[i]["n_links"] == n_links) and abs(reg[i]["S"] - S) <= 1e-12 * S, (i, reg[i])
        if status == R.GMS_SFM_SKIPPED:                                  # link -1 and zeros
            assert reg[i].tobytes() == np.array([(0.0, 0.0, 0, 0, -1, 0, R.GMS_SFM_SKIPPED, 0)], R.PAIR_REG_DTYPE).tobytes(), (i, reg[i])


def test_misfit_records_are_skipped_and_the_rest_is_chain_roles(ref_of):
    """The records that do not fit end skipped with zeros, the pair that hangs on one of them has no model, and every other output
    byte is chain_roles' own. The statement is fed the device's records, the host's plan and the arrays' length."""
    c, out, base, want = cases.case("misfit_records"), ref_of("misfit_records"), cases.case("chain_roles"), ref_of("chain_roles")
    n0, f0, m0 = c["n_base_pairs"], c["n_base_frames"], len(base["mask"])
    assert set(c["expect"]) == set(range(len(c["pairs"]))) and c["total_m"] == len(c["mask"]) and len(c["pairs"]) == n0 + 7
    assert c["plan"]["registers"][n0:].all() and c["plan"]["link"][n0:].tolist() == [0, 1, 2, 6, 0, 1, n0 + 4]
    assert [R.pair_fits(p, c["frame_off"], c["total_m"]) for p in c["pairs"]] == [True] * n0 + [False] * 6 + [True]
    assert all(R.pair_fits(p, c["frame_off"], c["total_m"]) for p in c["host_pairs"])
    p = c["pairs"][n0:]
    assert (p["frame_a"][0], p["frame_b"][1], p["m"][2], p["match_off"][3]) == (f0 + 7, -1, -3, -1)
    assert p["match_off"][4] + p["m"][4] == c["total_m"] + 5 and (c["mask"][-5:] != 0).all() and np.isfinite(c["points3d"][-5:]).all()
    assert (int(p["match_off"][5]), int(p["m"][5])) == (2 ** 63 - 2, 5)
    check_expect(c, out["registration"], c["expect"])
    assert out["registration"][:n0].tobytes() == want["registration"].tobytes() and out["views"][:f0].tobytes() == want["views"].tobytes()
    blank = np.zeros(7, R.VIEW_DTYPE)
    blank["pair"] = -1
    assert out["views"][f0:].tobytes() == blank.tobytes() and out["summary"].tobytes() == want["summary"].tobytes()
    for k in ("cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread"):
        assert out[k].tobytes() == want[k].tobytes(), k
    assert out["track"][:m0].tobytes() == want["track"].tobytes() and out["points_world"][:m0].tobytes() == want["points_world"].tobytes()
    assert (out["track"][m0:] == -1).all() and not out["points_world"][m0:].any()
    with pytest.raises(ValueError):                                      # the pair list's own plan refuses these records: one must be given
        run_ref(c, plan=None)


def test_bad_plan_links_are_skipped_and_take_their_descendants(ref_of):
    """A registering entry whose link is the pair itself, a later pair, below -1 or past the list: skipped with zeros; what hangs on
    it has no model; what does not is chain_roles' own."""
    c, want = cases.case("bad_plan_links"), ref_of("chain_roles")["registration"]
    n = len(c["pairs"])
    assert c["plan"]["link"][[1, 2]].tolist() == [1, 2 + 2] and c["more_plans"][0][0]["link"][[1, 6]].tolist() == [-2, n + 5]
    for given, expect in [(c["plan"], c["expect"])] + c["more_plans"]:
        assert set(expect) == set(range(n))
        out = run_ref(c, plan=given)
        assert out["plan"].tobytes() == given.tobytes()
        check_expect(c, out["registration"], expect)
        for i, (status, _, _) in expect.items():
            if status == 0:
                assert out["registration"][i].tobytes() == want[i].tobytes(), i
        assert out["summary"]["n_ok_pairs"][0] == sum(1 for e in expect.values() if e[0] == 0)


# ---- tracks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SANE_NAMES)
def test_tracks_against_scipy(ref_of, name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    c, out = cases.case(name), ref_of(name)
    K = int(c["frame_off"][-1])
    counts = np.diff(c["frame_off"])
    us, vs, est_at = [], [], []
    for i in np.nonzero(out["registration"]["status"] == 0)[0]:
        p = c["pairs"][i]
        o, n = int(p["match_off"]), int(c["tv"][i]["n_points"])
        mk = c["mask"][o:o + n] != 0
        q, t = c["matches"]["queryIdx"][o:o + n].astype(np.int64), c["matches"]["trainIdx"][o:o + n].astype(np.int64)
        rank = np.cumsum(mk) - mk
        assert ((q[mk] >= 0) & (q[mk] < counts[p["frame_a"]]) & (t[mk] >= 0) & (t[mk] < counts[p["frame_b"]])).all()
        us.append(c["frame_off"][p["frame_a"]] + q[mk])
        vs.append(c["frame_off"][p["frame_b"]] + t[mk])
        est_at.append(o + rank[mk])
    u, v, at = (np.concatenate(x) if x else np.zeros(0, np.int64) for x in (us, vs, est_at))   # (no ok pair: no edge)
    _, label = connected_components(coo_matrix((np.ones(len(u)), (u, v)), shape=(K, K)), directed=False)
    touched = np.zeros(K, bool)
    touched[u], touched[v] = True, True
    least = np.full(label.max() + 1, K)
    np.minimum.at(least, label, np.arange(K))                 # a component's id: its least keypoint
    ids = np.unique(least[label[touched]])
    assert np.array_equal(out["cloud_id"], ids) and (np.diff(out["cloud_id"]) > 0).all()
    assert np.array_equal(out["track"][at], least[label[u]])
    assert np.array_equal(out["cloud_obs"], [int((touched & (least[label] == g)).sum()) for g in ids])
    assert np.array_equal(out["cloud_est"], [int((least[label[u]] == g).sum()) for g in ids])
    assert out["summary"]["n_tracks"][0] == len(ids) and out["summary"]["n_points"][0] == len(u)
    order = np.argsort(at, kind="stable")                     # ascending (pair, rank): the offsets ascend with the pair index
    for c_i, g in enumerate(ids):
        mine = at[order][least[label[u[order]]] == g]
        assert np.array_equal(out["cloud"][c_i], out["points_world"][mine[0]], equal_nan=True)
        with np.errstate(all="ignore"):
            d = np.linalg.norm(out["points_world"][mine] - out["cloud"][c_i], axis=1)
        d = np.append(d[~np.isnan(d)], 0.0)                   # (a distance that is not a number does not count)
        assert out["cloud_spread"][c_i] == d.max() or abs(out["cloud_spread"][c_i] - d.max()) <= 1e-14 * d.max()
    frame_of = np.searchsorted(c["frame_off"], np.arange(K), side="right") - 1
    multi = sum(1 for g in ids if len(set(frame_of[touched & (least[label] == g)])) < int((touched & (least[label] == g)).sum()))
    assert out["summary"]["n_multi"][0] == multi


# ---- host builds ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(HOST_SRC)
    lib = C.CDLL(so)
    lib.sfr_host_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sfr_host_register.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def close(a, b, rel=1e-12, floor=0.0):
    """Finite values within rel of each other (of `floor`, where both are smaller: the entries of a rotation or of a point are held to
    the size of the whole, not each to its own); non-finite ones the same (NaN where NaN, the same infinity)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    fin = np.isfinite(a) & np.isfinite(b)
    same = (a[~fin] == b[~fin]) | (np.isnan(a[~fin]) & np.isnan(b[~fin]))
    return bool(same.all() and (np.abs(a[fin] - b[fin]) <= rel * np.maximum(np.maximum(np.abs(a[fin]), np.abs(b[fin])), floor)).all())


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_build_of_the_core_equals_the_statement(host, ref_of, name):
    """Every case, those of cases.UNFIT with their records, their plan and the arrays' length: the host build applies sfr::pair_fits
    and sfr::plan_entry_fits as the kernels do."""
    c, want = cases.case(name), ref_of(name)
    n_frames, n_pairs = len(c["frame_off"]) - 1, len(c["pairs"])
    views, reg = np.zeros(n_frames, R.VIEW_DTYPE), np.zeros(n_pairs, R.PAIR_REG_DTYPE)
    world = np.zeros_like(c["points3d"])
    arrs = [np.ascontiguousarray(c[k]) for k in ("frame_off", "pairs", "matches", "mask", "points3d", "tv")]
    given = np.ascontiguousarray(c["plan"]) if "plan" in c else None
    assert host.sfr_host_register(arrs[0].ctypes.data, n_frames, arrs[1].ctypes.data, n_pairs, c.get("total_m", len(c["mask"])),
                                  None if given is None else given.ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data,
                                  arrs[4].ctypes.data, arrs[5].ctypes.data, c["root"], c["min_links"], views.ctypes.data, reg.ctypes.data,
                                  world.ctypes.data) == 0
    for f in ("n_links", "depth", "link", "role", "status"):
        assert np.array_equal(reg[f], want["registration"][f]), f
    assert np.array_equal(views["registered"], want["views"]["registered"]) and np.array_equal(views["pair"], want["views"]["pair"])
    assert close(reg["r"], want["registration"]["r"]) and close(reg["S"], want["registration"]["S"])
    assert close(views["R"], want["views"]["R"], floor=1.0) and close(views["t"], want["views"]["t"], floor=1.0)
    assert close(world, want["points_world"], floor=1.0)


def test_plans_agree_on_random_pair_lists(host, pkg):
    """The host build and the C ABI's gms_sfm_plan against the Python plan, exactly: random lists over few frames (many reverse, loop and
    repeated pairs), every root, and the refusals."""
    rng = np.random.default_rng(5)
    for trial in range(200):
        n_frames = int(rng.integers(1, 9))
        n_pairs = int(rng.integers(0, 20))
        fp = rng.integers(0, n_frames, (n_pairs, 2))
        root = int(rng.integers(0, n_frames))
        want = R.plan(fp, n_frames, root)
        recs = np.zeros(n_pairs, pkg.PAIR_DTYPE)
        recs["frame_a"], recs["frame_b"] = fp[:, 0], fp[:, 1]
        got = np.zeros(n_pairs, R.PLAN_DTYPE)
        assert host.sfr_host_plan(recs.ctypes.data, n_pairs, n_frames, root, got.ctypes.data) == 0
        assert got.tobytes() == want.tobytes()
        assert pkg.sfm_plan(recs, n_frames, root).tobytes() == want.tobytes()
        assert pkg.sfm_plan(fp, n_frames, root).tobytes() == want.tobytes()
    for fp, n_frames, root in (([(0, 3)], 3, 0), ([(-1, 0)], 3, 0), ([(0, 1)], 3, 3), ([(0, 1)], 3, -1), ([(0, 1)], 0, 0)):
        with pytest.raises(pkg.GmsError) as e:
            pkg.sfm_plan(fp, n_frames, root)
        assert e.value.code == -1


def test_dtypes_match_the_statement(pkg):
    assert pkg.SFM_PLAN_DTYPE == R.PLAN_DTYPE and pkg.SFM_VIEW_DTYPE == R.VIEW_DTYPE and pkg.SFM_PAIR_REG_DTYPE == R.PAIR_REG_DTYPE
    assert pkg.SFM_SUMMARY_DTYPE == R.SUMMARY_DTYPE and pkg.GMS_SFM_SKIPPED == R.GMS_SFM_SKIPPED
    lib = pkg.load_library()
    assert lib.gms_sfm_register_workspace_bytes(0, 1, 10, 10) == 0 and lib.gms_sfm_register_workspace_bytes(2, -1, 10, 10) == 0
    assert lib.gms_sfm_register_workspace_bytes(2, 1, 2**31 - 1, 10) == 0 and lib.gms_sfm_register_workspace_bytes(2, 1, 10, -1) == 0
    assert lib.gms_sfm_register_workspace_bytes(8, 7, 16000, 21000) % 256 == 0 and lib.gms_sfm_register_workspace_bytes(1, 0, 0, 0) > 0


def test_stand_alone_host_program_under_sanitizers():
    out = hb.run(hb.host_exe_sanitized(HOST_SRC, defines=("SFR_HOST_MAIN",)))
    assert out.returncode == 0 and out.stdout.startswith("sfr_host: tiny 0 40 2.000000"), out.stdout + out.stderr
    # sfr::pair_fits on the records of misfit_records, match_off = 2^63 - 2 with m = 5 among them: a sum of the two would stop the
    # program here ("signed integer overflow", -fno-sanitize-recover)
    assert "sfr_host: misfit records, 0 wrong" in out.stdout and "runtime error" not in out.stderr, out.stdout + out.stderr


# ---- the workspace's layout -----------------------------------------------------------------------------------------------------------
def _run_layout(exe):
    res = hb.run_clean(exe)
    report = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and "cases: 0 bad" in res.stdout, report


def test_layout(pkg):
    exe = hb.host_exe(LAYOUT_SRC)
    _run_layout(exe)


def test_layout_under_sanitizers():
    exe = hb.host_exe_sanitized(LAYOUT_SRC)
    _run_layout(exe)
