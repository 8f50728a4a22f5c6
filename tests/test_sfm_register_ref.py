"""CPU: the registration statement (tests/sfm_register_ref.py) -- a five-view scene with ground-truth poses through the
CPU two-view chain, hand-made records with analytically known scales (tests/sfm_register_cases.py), the tracks against
scipy.sparse.csgraph.connected_components, the host build of sfm_register_core.h (tests/cpp/sfm_register_host.cpp) and the C ABI's
gms_sfm_plan against the Python plan, and the workspace's layout (tests/cpp/sfm_register_layout_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sfm_ref
import sfm_register_cases as cases
import sfm_register_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, "tests", "cpp", "sfm_register_host.cpp")
LAYOUT_SRC = os.path.join(ROOT, "tests", "cpp", "sfm_register_layout_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "sfm-gms_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
CASE_NAMES = sorted(cases.CASES)


def run_ref(c):
    return R.register(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])


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
@pytest.mark.parametrize("name", CASE_NAMES)
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


# ---- tracks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
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
    u, v, at = np.concatenate(us), np.concatenate(vs), np.concatenate(est_at)
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
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sfr") / "libsfr_host.so")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-shared", "-fPIC", "-o", so, HOST_SRC])
    lib = C.CDLL(so)
    lib.sfr_host_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sfr_host_register.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
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
    c, want = cases.case(name), ref_of(name)
    n_frames, n_pairs = len(c["frame_off"]) - 1, len(c["pairs"])
    views, reg = np.zeros(n_frames, R.VIEW_DTYPE), np.zeros(n_pairs, R.PAIR_REG_DTYPE)
    world = np.zeros_like(c["points3d"])
    arrs = [np.ascontiguousarray(c[k]) for k in ("frame_off", "pairs", "matches", "mask", "points3d", "tv")]
    assert host.sfr_host_register(arrs[0].ctypes.data, n_frames, arrs[1].ctypes.data, n_pairs, arrs[2].ctypes.data, arrs[3].ctypes.data,
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


def test_stand_alone_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sfr_host_asan")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *FLAGS, "-DSFR_HOST_MAIN", "-o", exe,
                            HOST_SRC], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("this toolchain cannot build with -fsanitize=address,undefined: " + (build.stderr.strip().splitlines() or ["?"])[-1][:200])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("sfr_host: tiny 0 40 2.000000"), out.stdout + out.stderr


# ---- the workspace's layout -----------------------------------------------------------------------------------------------------------
def _run_layout(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    report = (res.stdout + res.stderr)[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, report
    assert res.returncode == 0 and "cases: 0 bad" in res.stdout, report


def test_layout(tmp_path, pkg):
    exe = str(tmp_path / "sfm_register_layout_check")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-o", exe, LAYOUT_SRC])
    _run_layout(exe)


def test_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sfm_register_layout_check_san")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS, "-o", exe, LAYOUT_SRC],
                           capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("this toolchain cannot build with -fsanitize=address,undefined: " + (build.stderr.strip().splitlines() or ["?"])[-1][:200])
    _run_layout(exe)
