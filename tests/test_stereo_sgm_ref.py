"""CPU: the semi-global matching statement (tests/stereo_sgm_ref.py) -- a hand-worked path, the literal loop against
the vectorised form over a parameter sweep, the host build of stereo_sgm_core.h (tests/cpp/stereo_sgm_host.cpp) against both, p1 = p2 =
0 against StereoBM, the bound 0 <= L <= C + p2 and the parameter rule at 65535, the committed 450 x 375 pair against its ground truth
beside StereoBM, and the named cases of tests/stereo_sgm_cases.py: each contains what it is named for, by the statement's own census."""
import ctypes as C

import numpy as np
import pytest

import stereo_bm_ref as B
import stereo_sgm_cases as cases
import stereo_sgm_ref as R
import hostbuild as hb

SRC = "stereo_sgm_host.cpp"


@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(SRC)
    lib = C.CDLL(so)
    lib.sgm_host_params_ok.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.sgm_host_aggregate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sgm_host_decide.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sgm_host_layout.argtypes = [C.c_int] * 6 + [C.c_void_p]
    return lib


def _record(p):
    return np.array([p[n] for n in R.PARAM_NAMES], np.int32)


def _host_maps(host, left, right, **kw):
    """The statement with its aggregation and decision replaced by the host build's."""
    p, left, right, H, W = R._prepare(left, right, kw)
    assert host.sgm_host_params_ok(_record(p).ctypes.data, W, H) == 1
    w2 = p["block_size"] // 2
    disp = np.full((H, W), B.filtered_value(p), np.int16)
    cost = np.full((H, W), -1, np.int32)
    lofs, _, _, none = B.ranges(p, W)
    if none:
        return disp, cost
    vol, tex = R.cost_volume(left, right, p)
    ny, wx, nd = vol.shape
    c16 = np.ascontiguousarray(vol, np.uint16)
    s16 = np.zeros_like(c16)
    lmax = np.zeros(8, np.int32)
    assert host.sgm_host_aggregate(c16.ctypes.data, ny, wx, nd, p["p1"], p["p2"], p["n_paths"], s16.ctypes.data, lmax.ctypes.data) == 0
    assert (s16 == R.aggregate(vol, p)).all()
    assert (lmax[:p["n_paths"]] <= vol.max() + p["p2"]).all() and not lmax[p["n_paths"]:].any()
    t32 = np.ascontiguousarray(tex, np.int32)
    d, c = np.zeros(ny * wx, np.int32), np.zeros(ny * wx, np.int32)
    host.sgm_host_decide(s16.ctypes.data, t32.ctypes.data, ny * wx, _record(p).ctypes.data, d.ctypes.data, c.ctypes.data)
    disp[w2:H - w2, lofs:lofs + wx] = d.reshape(ny, wx)
    cost[w2:H - w2, lofs:lofs + wx] = c.reshape(ny, wx)
    if p["disp12_max_diff"] >= 0:
        B.validate(disp, cost, p)
    B.roi_fill(disp, p, lofs)
    return disp, cost


# ---- the path step ----------------------------------------------------------------------------------------------------------------
def test_hand_worked_path():
    # one line of three pixels, four disparities, p1 = 2, p2 = 5
    vol = np.array([[[4, 0, 9, 9], [1, 7, 7, 0], [3, 3, 3, 3]]], np.int32)
    L = R.path_costs(vol, 0, 1, 2, 5)
    # pixel 1: Lp = (4, 0, 9, 9), m = 0: min(4, 0+2, -, 5) = 2; min(0, 4+2, 9+2, 5) = 0; min(9, 0+2, 9+2, 5) = 2; min(9, 9+2, -, 5) = 5
    assert L[0, 1].tolist() == [1 + 2, 7 + 0, 7 + 2, 0 + 5]
    # pixel 2: Lp = (3, 7, 9, 5), m = 3: (3, min(7, 5, 11, 8) = 5, min(9, 9, 7, 8) = 7, min(5, 11, 8) = 5) - 3
    assert L[0, 2].tolist() == [3 + 0, 3 + 2, 3 + 4, 3 + 2]
    assert R.path_costs(vol, 0, -1, 2, 5)[0, 2].tolist() == [3, 3, 3, 3]            # the other way round pixel 2 starts the line
    assert R.path_costs_loop(vol.tolist(), 0, 1, 2, 5) == L.tolist()
    for dy, dx in R.DIRECTIONS[2:]:                                                 # one row: every other direction leaves at once
        assert (R.path_costs(vol, dy, dx, 2, 5) == vol).all()


# ---- the two forms and the host build ---------------------------------------------------------------------------------------------
# nd, md, block_size, cap, texture, uniqueness, disp12, p1, p2, n_paths[, the true disparity of the pair: -3 where not given]
SWEEP = [
    (16, 0, 5, 61, 0, 0, 1, None, None, 8),
    (16, -4, 5, 61, 0, 0, 1, None, None, 4),
    (16, 3, 5, 31, 100, 10, 0, 0, 120, 8),
    (16, -8, 7, 15, 0, 15, -1, 40, 40, 8),
    (32, -20, 5, 63, 507, 0, 2, 5041, 5041, 8),
    (16, 0, 9, 7, 0, 5, 1, 7, 900, 4),
    (16, 0, 5, 61, 0, 0, 1, 0, 0, 8),
    (16, -20, 5, 61, 0, 0, 1, None, None, 8, -12),   # md <= -nd: rofs = 5, lofs = 0
    (16, -15, 5, 61, 0, 0, 1, None, None, 8, -7),    # md = -(nd - 1): both offsets 0
]


def _sweep_pair(h, w, seed, disparity=-3):
    """right[x] = left[x + disparity] plus noise, cut from one wider image: `disparity` is at most 0."""
    rng = np.random.default_rng(seed)
    m = max(8, -disparity)
    left = cases._smooth(f"sweep{seed}", h, w + m)
    right = np.clip(left[:, m + disparity:w + m + disparity].astype(np.int32) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(left[:, m:]), right


@pytest.mark.parametrize("shape", [(19, 44), (20, 45)])
@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_loop_vectorised_and_host_agree(host, shape, case):
    nd, md, bs, cap, tex, ur, dmd, p1, p2, n_paths, *true = SWEEP[case]
    left, right = _sweep_pair(*shape, case, *true)
    assert not true or md <= true[0] < md + nd
    kw = dict(num_disparities=nd, min_disparity=md, block_size=bs, pre_filter_cap=cap, texture_threshold=tex, uniqueness_ratio=ur,
              disp12_max_diff=dmd, p1=p1, p2=p2, n_paths=n_paths)
    want = R.stereo_sgm_loop(left, right, **kw)
    for got in (R.stereo_sgm(left, right, **kw), _host_maps(host, left, right, **kw)):
        assert got[0].dtype == np.int16 and got[1].dtype == np.int32
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), kw
    assert (want[0] != B.filtered_value(R.make_params(**kw))).any() or tex == 507, kw
    lofs, rofs = B.ranges(R.make_params(**kw), shape[1])[:2]
    assert (lofs, rofs) == (max(nd - 1 + md, 0), max(-(nd - 1 + md), 0))


@pytest.mark.parametrize("name", ["diag_wide", "diag_tall", "two_rows", "one_column", "unsigned_range", "stripes8", "nd_80", "bs7_seams",
                                  "rofs_5", "offsets_zero", "ends", "bs51_seams"])
def test_host_build_on_named_cases(host, name):
    left, right, kw = cases.case(name)
    got = _host_maps(host, left, right, **kw)
    want = cases.expected(name)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_sanitizer_run_of_the_stand_alone_program():
    exe = hb.host_exe_sanitized(SRC, defines=("SGM_HOST_MAIN",))
    out = hb.run(exe)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("sgm_host: tiny ")


# ---- properties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_paths", [4, 8])
@pytest.mark.parametrize("name", ["diag_wide", "md_negative", "stripes8", "lr_0", "rofs_5", "bs7_seams", "bs21"])
def test_zero_penalties_reproduce_stereo_bm(name, n_paths):
    left, right, kw = cases.case(name)
    kw = {k: v for k, v in kw.items() if k in B.PARAM_NAMES}
    kw["uniqueness_ratio"] = 0
    bd, bc = B.stereo_bm(left, right, **kw)
    sd, sc = R.stereo_sgm(left, right, p1=0, p2=0, n_paths=n_paths, **kw)
    assert (sd == bd).all()
    assert (sc == np.where(bc >= 0, n_paths * bc, -1)).all()
    assert (bd != B.filtered_value(B.make_params(**kw))).sum() > 100


@pytest.mark.parametrize("name", ["unsigned_range", "diag_tall", "p1_zero", "p1_eq_p2", "stripes64"])
def test_path_costs_stay_within_their_bound(name):
    left, right, kw = cases.case(name)
    p = R.make_params(**kw)
    vol, _ = R.cost_volume(left, right, p)
    assert vol.min() >= 0 and vol.max() <= p["block_size"] ** 2 * 2 * p["pre_filter_cap"]
    for dy, dx in R.DIRECTIONS:
        L = R.path_costs(vol, dy, dx, p["p1"], p["p2"])
        assert (L >= vol).all() and (L <= vol + p["p2"]).all()            # min(...) - m lies in [0, p2]
    assert R.aggregate(vol, p).max() <= R.LIMIT


def test_parameter_rule_at_the_limit(host):
    # 65535 is odd and n_paths is 4 or 8, so no accepted set lands on the bound itself: the last accepted p2 gives 8 (25 * 126 + 5041) =
    # 65528 and 4 (25 * 126 + 13233) = 65532, and one step of p2 further is past 65535
    ok = R.make_params(pre_filter_cap=63, p1=5041, p2=5041)
    R.check_params(ok, 100, 50)
    assert host.sgm_host_params_ok(_record(ok).ctypes.data, 100, 50) == 1
    for n_paths, p2 in ((8, 5041), (4, 13233)):
        at = R.make_params(pre_filter_cap=63, p1=0, p2=p2, n_paths=n_paths)
        past = dict(at, p2=p2 + 1)
        assert n_paths * (25 * 126 + p2) <= 65535 < n_paths * (25 * 126 + p2 + 1)
        R.check_params(at, 100, 50)
        assert host.sgm_host_params_ok(_record(at).ctypes.data, 100, 50) == 1
        with pytest.raises(ValueError):
            R.check_params(past, 100, 50)
        assert host.sgm_host_params_ok(_record(past).ctypes.data, 100, 50) == 0
    for bad in (dict(p1=-1), dict(p1=801), dict(n_paths=5), dict(n_paths=16), dict(speckle_window_size=100), dict(block_size=6),
                dict(num_disparities=24)):
        p = R.make_params(**bad)
        with pytest.raises(ValueError):
            R.check_params(p, 100, 50)
        assert host.sgm_host_params_ok(_record(p).ctypes.data, 100, 50) == 0, bad


def test_workspace_layout(host):
    """StereoBM's regions first, then the texture plane and the two volumes: in order, 256-byte aligned, each as large as stated, and a
    total of 0 where the size does not fit."""
    def layout(*a):
        out = np.zeros(5, np.uint64)
        host.sgm_host_layout(*a, out.ctypes.data)
        return [int(v) for v in out]

    for n, W, H, ny, wx, nd in ((1, 450, 375, 371, 227, 224), (3, 60, 24, 20, 45, 16), (2, 16, 24, 20, 1, 16), (1, 100, 20, 0, 0, 112),
                                (65535, 8192, 4000, 3996, 8177, 512)):
        bm, tex, vol_c, vol_s, total = layout(n, W, H, ny, wx, nd)
        px = n * ny * wx
        assert bm >= 6 * n * W * H and tex >= bm and vol_c >= tex + 4 * px and vol_s >= vol_c + 2 * nd * px and total >= vol_s + 2 * nd * px
        assert all(v % 256 == 0 for v in (bm, tex, vol_c, vol_s, total))
        assert total - (6 * n * W * H + 4 * px + 4 * nd * px) < 6 * 256          # nothing but round-ups besides
    assert layout(65535, 8192, 2 ** 31 - 1, 2 ** 31 - 5, 8177, 512)[4] == 0


# ---- the committed pair -----------------------------------------------------------------------------------------------------------
def test_committed_pair_beats_block_matching():
    """The reference's parameters on its 450 x 375 pair: among the pixels with ground truth that get a value, those within 1 px of
    gt / 4. Recorded in DESIGN.md §4.8b: StereoBM 46 662 of 53 473 (0.873), SGM with 8 paths 51 035 of 55 384 (0.921)."""
    left, right, gt = cases.golden_pair()
    inv = B.filtered_value(B.make_params())
    counts = {}
    for name, disp in (("bm", B.stereo_bm(left, right)[0]), ("sgm", cases.golden_expected(8)[0])):
        valid = (disp != inv) & (gt > 0)
        good = np.abs(disp[valid] / 16.0 - gt[valid] / 4.0) <= 1.0
        counts[name] = (int(valid.sum()), int(good.sum()))
        print(f"{name}: {counts[name][1]} of {counts[name][0]} within 1 px ({good.mean():.3f})")
    assert counts["sgm"][1] > counts["bm"][1]
    assert counts["sgm"][1] / counts["sgm"][0] >= 0.9


# ---- the named cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_named_cases_contain_what_they_are_for(name):
    left, right, kw = cases.case(name)
    assert sorted(cases.FLOORS) == sorted(cases.NAMES)
    cases.check_floors(name, cases.census(left, right, **kw))


def test_left_right_cases_are_ordered():
    got = {n: cases.census(*cases.case(n)[:2], **cases.case(n)[2])["lr_removed"] for n in ("lr_off", "lr_0", "lr_2")}
    assert got["lr_off"] == 0 < got["lr_2"] <= got["lr_0"]
