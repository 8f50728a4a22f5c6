"""CPU: the named LOGOS cases (tests/logos_cases.py) reach the regimes they are named for, by the statement tests/logos_ref.py alone;
the keypoint domain (kp_ok) in the statement, in the host build of logos_core.h and at the library's one-shot entry point, which
refuses what lies outside before any device work. This module is the only place where angles beyond 1e5 degrees are passed to the
library: the refusal comes from a host loop, and no kernel ever sees them."""
import ctypes as C

import numpy as np
import pytest

import logos_cases as LC
import logos_ref
from test_logos_oracle import host  # noqa: F401  (the host build of logos_core.h, a module-scoped fixture)

GMS_ERR_DOMAIN = -2


def _counts(name, a, b):
    res, (nc, ns, peak) = LC.expected(name, a, b)
    return len(res), nc, ns, peak


def tie_points(kp, k=logos_ref.NUM):
    """The points with more than min(k, n - 1) other points at or within their k-th distance: those the tie kernels redo."""
    x, y = kp[:, 0], kp[:, 1]
    n = len(x)
    kk = min(k, n - 1)
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    d = (dx * dx + dy * dy).astype(np.float32)
    np.fill_diagonal(d, np.inf)
    dk = np.sort(d, axis=1)[:, kk - 1:kk]
    return np.nonzero((d <= dk).sum(1) > kk)[0], np.argsort(d, axis=1, kind="stable")[:, :kk]


def test_case_names_and_sizes():
    names = [c["name"] for c in LC.all_cases()]
    assert len(set(names)) == len(names) == 17
    assert [len(f) for f in LC.case("empty_in_table")["frames"]] == list(LC.EMPTY_TABLE_COUNTS)
    assert len(LC.case("empty_in_table")["pairs"]) == 100
    assert [len(f) for f in LC.case("tiny")["frames"]] == [k for k in range(1, 9) for _ in (0, 1)] + [40]
    assert [len(f) for f in LC.case("scan_edges")["frames"]] == [1023, 1024, 1025, 300]
    assert [len(f) for f in LC.case("tile_edges")["frames"]] == [256, 256, 257, 257] * 2
    for c in LC.all_cases():
        for f in c["frames"]:
            assert not f.flags.writeable and logos_ref.kp_ok(f[:, 0], f[:, 1], f[:, 3]).all(), c["name"]
            assert not (np.isfinite(f[:, 3]) & (np.abs(f[:, 3]) > 1e5)).any()
    for f in LC.domain_refusals()["frames"]:      # the GPU tests' refused values: nothing finite beyond 3601 degrees
        assert (np.abs(f[:, 3][np.isfinite(f[:, 3])]) <= 3601.0).all()


def test_tiny_frames_have_survivors_from_two_keypoints_on():
    for k in range(1, 9):
        a, b = 2 * k - 2, 2 * k - 1
        want = 0 if k == 1 else k
        assert _counts("tiny", a, b)[0] == want and _counts("tiny", b, a)[0] == want, k
        nb = logos_ref.neighbours(LC.case("tiny")["frames"][a][:, 0], LC.case("tiny")["frames"][a][:, 1])
        assert ((nb >= 0).sum(1) == min(5, k - 1)).all()          # -1 pads below six keypoints
    # seven keypoints with six others at unequal distances: no tie here; the tie list with m = 6 is coincident_7's


def test_empty_frames_give_empty_results_and_the_large_pairs_survivors():
    c = LC.case("empty_in_table")
    n = LC.EMPTY_TABLE_COUNTS
    for a, b in c["pairs"]:
        got = _counts("empty_in_table", a, b)
        if n[a] == 0 or n[b] == 0:
            assert got == (0, 0, 0, -1)
    for a, b in ((1, 7), (7, 1), (1, 8), (8, 7)):
        assert _counts("empty_in_table", a, b)[0] >= 200


@pytest.mark.parametrize("n", [6, 7, 40, 300])
def test_coincident_points_have_candidates_and_no_support(n):
    name = f"coincident_{n}"
    assert _counts(name, 0, 0) == (0, n * n, 0, -1)
    kp = LC.case(name)["frames"][0]
    ties, stable = tie_points(kp)
    assert len(ties) == (0 if n == 6 else n)                       # 6: five others, no tie; from 7 on every point is tied
    nb = logos_ref.neighbours(kp[:, 0], kp[:, 1])
    # all records equal: the insertion sort (up to 32 records) and the partition above it (39, 299 records: everything lands in
    # the pivot's range) both leave them in index order
    assert all(list(nb[i]) == list(stable[i]) for i in range(n))


def test_triples_on_lattice_counts():
    # (survivors, candidates, supported, peak bin) of the lattice against its moved copy, both ways, and against itself
    assert len(LC.case("triples_on_lattice")["frames"][0]) == 432
    assert _counts("triples_on_lattice", 0, 1) == (361, 46764, 364, 105)
    assert _counts("triples_on_lattice", 1, 0) == (360, 46764, 364, 81)
    assert _counts("triples_on_lattice", 0, 0) == (440, 46764, 440, 93)
    kp = LC.case("triples_on_lattice")["frames"][0]
    ties, stable = tie_points(kp)
    # six tied points at the two nearest sites for three places; the first and last row have one nearest site and no tie
    assert len(ties) == 432 - 2 * 12 * 3
    nb = logos_ref.neighbours(kp[:, 0], kp[:, 1])
    d0 = ((kp[nb, 0] - kp[:, None, 0]) ** 2 + (kp[nb, 1] - kp[:, None, 1]) ** 2 == 0).sum(1)
    assert (d0 == 2).all()                                           # two coincident neighbours each: NaN geometry
    assert any(set(nb[i]) != set(stable[i]) for i in ties)
    kp2 = LC.case("triples_on_lattice")["frames"][1]


def test_value_limits_change_the_output_without_emptying_it():
    clean, limits = _counts("value_limits", 0, 1), _counts("value_limits", 2, 3)
    assert clean[0] == 400
    assert 0 < limits[0] < clean[0] and limits[1] == clean[1]
    assert limits[0] == 236 and _counts("value_limits", 3, 2)[0] == 236 and _counts("value_limits", 2, 2)[0] == 390
    c = LC.case("value_limits")
    for f in (2, 3):
        kp = c["frames"][f]
        assert set(np.float32(LC.LIMIT_ANGLES).tolist()) <= set(kp[:, 3].tolist()) and (kp[:60, 3] == -1).all()
        s = kp[:, 2]
        assert np.isnan(s).any() and np.isposinf(s).any() and (s == 0).any() and (s < 0).any() and (s == np.float32(3.4e38)).any()
        assert ((s > 0) & (s < np.float32(1.2e-38))).any()                                  # the subnormal


def test_word_scan_and_tile_edges_have_survivors():
    for n_words in LC.WORD_EDGES:
        name = f"word_edges_{n_words}"
        c = LC.case(name)
        assert [int(w.max()) for w in c["words"][2:4]] == [n_words - 1] * 2 and (c["words"][2] == n_words - 1).all()
        assert set(c["words"][4].tolist()) == ({0, n_words - 1})
        for a, b in c["pairs"]:
            assert _counts(name, a, b)[0] >= 300
    assert [_counts("scan_edges", a, 3)[0] for a in range(3)] == [300, 300, 300]
    c = LC.case("tile_edges")
    for a, b in c["pairs"]:
        assert _counts("tile_edges", a, b)[0] >= 256
    for f in range(8):   # ties in the integer frames alone
        ties, stable = tie_points(c["frames"][f])
        assert (len(ties) > 0) == (f in (4, 6)), f
        if len(ties):
            kp = c["frames"][f]
            nb = logos_ref.neighbours(kp[:, 0], kp[:, 1])
            assert any(set(nb[i]) != set(stable[i]) for i in ties)


# ---- the keypoint domain ---------------------------------------------------------------------------------------------------------
INSIDE = [3600.0, -3600.0, -1.0, 0.0, 360.0, 359.99997, 540.0]
OUTSIDE = [float(np.nextafter(np.float32(3600.0), np.float32(np.inf))), -float(np.nextafter(np.float32(3600.0), np.float32(np.inf))),
           1e5, -1e5, 1e10, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan]


def _host_kp_ok(host, x, y, angle):  # noqa: F811
    host.logos_host_kp_ok.argtypes = [C.c_float] * 3
    host.logos_host_kp_ok.restype = C.c_int
    return bool(host.logos_host_kp_ok(x, y, angle))


def test_kp_ok_of_host_build_and_statement_agree(host):  # noqa: F811
    for a in INSIDE:
        assert _host_kp_ok(host, 1.0, 2.0, a) and bool(logos_ref.kp_ok(1.0, 2.0, a)), a
    for a in OUTSIDE:
        assert not _host_kp_ok(host, 1.0, 2.0, a) and not bool(logos_ref.kp_ok(1.0, 2.0, a)), a
    for v in (np.inf, -np.inf, np.nan):
        assert not _host_kp_ok(host, v, 2.0, 0.0) and not bool(logos_ref.kp_ok(v, 2.0, 0.0))
        assert not _host_kp_ok(host, 1.0, v, 0.0) and not bool(logos_ref.kp_ok(1.0, v, 0.0))
    assert _host_kp_ok(host, -3.4e38, 3.4e38, 0.0) and bool(logos_ref.kp_ok(-3.4e38, 3.4e38, 0.0))   # finite is enough for x, y


def test_rel_ori_stays_within_pi_over_the_whole_domain(host):  # noqa: F811
    host.logos_host_orientation.argtypes = [C.c_float]
    host.logos_host_orientation.restype = C.c_float
    host.logos_host_rel_ori.argtypes = [C.c_float, C.c_float]
    host.logos_host_rel_ori.restype = C.c_float
    angles = np.float32([3600.0, -3600.0, 3599.9, -3599.9, -1.0, 0.0, 360.0])
    ori = [host.logos_host_orientation(float(a)) for a in angles]
    want = ((angles.astype(np.float64) * logos_ref.PI) / 180.0).astype(np.float32)
    assert np.float32(ori).tobytes() == want.tobytes()
    for i, o1 in enumerate(ori):
        for j, o2 in enumerate(ori):
            r = host.logos_host_rel_ori(o1, o2)
            assert -np.pi <= float(r) <= np.pi, (angles[i], angles[j], r)
            ref = logos_ref._wrap_pair(np.float32([o1]) - np.float32([o2]))[0]
            assert np.float32(r).tobytes() == ref.tobytes()
            # the same angle up to whole turns, within the rounding of a float near 40 pi
            assert abs(np.remainder(float(r) - (float(o1) - float(o2)) + np.pi, 2 * np.pi) - np.pi) < 1e-4


@pytest.mark.parametrize("name,a,b", [("triples_on_lattice", 0, 1), ("coincident_40", 0, 0), ("value_limits", 2, 3)])
def test_host_support_equals_statement_on_nan_geometry(host, name, a, b):  # noqa: F811
    c = LC.case(name)
    kp1, kp2 = np.ascontiguousarray(c["frames"][a]), np.ascontiguousarray(c["frames"][b])
    l1, l2 = np.ascontiguousarray(c["words"][a]), np.ascontiguousarray(c["words"][b])
    with np.errstate(all="ignore"):
        P1, P2 = logos_ref.points(kp1, l1), logos_ref.points(kp2, l2)
        nb1, nb2 = logos_ref.neighbours(P1[0], P1[1]), logos_ref.neighbours(P2[0], P2[1])
        ci, cj = logos_ref.candidates(l1, l2)
        want, want_o = logos_ref.local_support(P1, P2, nb1, nb2, ci, cj)
    got, got_o = np.zeros(len(ci), np.int32), np.zeros(len(ci), np.float32)
    ci64, cj64 = np.ascontiguousarray(ci, np.int64), np.ascontiguousarray(cj, np.int64)
    host.logos_host_support(kp1.ctypes.data, l1.ctypes.data, nb1.ctypes.data, kp2.ctypes.data, l2.ctypes.data, nb2.ctypes.data,
                            ci64.ctypes.data, cj64.ctypes.data, len(ci), got.ctypes.data, got_o.ctypes.data)
    assert got_o.tobytes() == want_o.tobytes()
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {len(ci)} candidate supports differ"
    assert int((want > 0).sum()) == LC.expected(name, a, b)[1][1]


# ---- the one-shot refuses what lies outside the domain before any device work ---------------------------------------------------
REFUSED = [("angle", 1e10), ("angle", 3.4e38), ("angle", -1e10), ("angle", np.inf), ("angle", np.nan), ("x", np.inf), ("y", np.nan),
           ("angle", float(np.nextafter(np.float32(3600.0), np.float32(np.inf))))]


@pytest.mark.parametrize("field,value", REFUSED)
@pytest.mark.parametrize("frame", [0, 1])
def test_one_shot_refuses_outside_the_domain_without_a_device(pkg, field, value, frame):
    lib = pkg.load_library()
    rng = np.random.default_rng(3)
    kps = [np.zeros(20, pkg.KEYPOINT_DTYPE) for _ in range(2)]
    for k in kps:
        k["x"], k["y"], k["size"], k["angle"] = rng.uniform(0, 100, 20), rng.uniform(0, 100, 20), 5.0, rng.uniform(0, 360, 20)
    kps[frame][field][19 if frame else 0] = value
    l = np.zeros(20, np.int32)
    out = np.full(16 * 40, 0x5A, np.uint8)
    n = C.c_int64(77)
    res = np.zeros(1, pkg.LOGOS_RESULT_DTYPE)
    rc = lib.gms_logos_match(kps[0].ctypes.data, 20, kps[1].ctypes.data, 20, l.ctypes.data, l.ctypes.data, out.ctypes.data, 40,
                             C.byref(n), res.ctypes.data)
    assert rc == GMS_ERR_DOMAIN and n.value == 0 and res["status"][0] == GMS_ERR_DOMAIN
    assert (res["n_candidates"][0], res["n_supported"][0], res["n_out"][0], res["peak_bin"][0]) == (0, 0, 0, -1)
    assert (out == 0x5A).all()
    with pytest.raises(pkg.GmsError) as e:
        pkg.matchLOGOS(kps[0], kps[1], l, l)
    assert e.value.code == GMS_ERR_DOMAIN
    a4 = [np.stack([k["x"], k["y"], k["size"], k["angle"]], 1) for k in kps]
    with pytest.raises(ValueError):
        logos_ref.match(a4[0], a4[1], l, l)


def test_one_shot_checks_the_domain_of_a_frame_matched_against_an_empty_one(pkg):
    lib = pkg.load_library()
    kp = np.zeros(3, pkg.KEYPOINT_DTYPE)
    kp["angle"][1] = 1e10
    l = np.zeros(3, np.int32)
    n = C.c_int64(5)
    assert lib.gms_logos_match(kp.ctypes.data, 3, None, 0, l.ctypes.data, None, None, 0, C.byref(n), None) == GMS_ERR_DOMAIN
    assert n.value == 0
    with pytest.raises(ValueError):
        logos_ref.match(np.float32([[0, 0, 1, 1e10]]), np.zeros((0, 4), np.float32), [0], [])
