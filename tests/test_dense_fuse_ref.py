"""The statement of the dense fusion in numpy (tests/dense_fuse_ref.py) against a g++ build of the header the kernels compile
(sfm-gms_amd/csrc/dense_fuse_core.h through the stand-alone program tests/cpp/dense_fuse_host.cpp), byte for byte, plain and under
sanitizers; that each case of tests/dense_fuse_cases.py holds what it is named for; the workspace's layout; and the rule's effect on
the rendered plane seen by three cameras. The host program never runs inside Python: cases go to it as files."""

import numpy as np
import pytest

import dense_fuse_cases as fc
import dense_fuse_ref as fr
import hostbuild as hb

SRC = "dense_fuse_host.cpp"

def statement(case):
    return fr.fuse(case["sources"], case["neighbors"], case["channels"], case["tol16"], case["min_support"], case["fused_cap"])


def run_host(exe, case, tmp_path):
    total_cap = sum(len(s["xyz"]) for s in case["sources"])
    src, dst = tmp_path / (case["name"] + ".in"), tmp_path / (case["name"] + ".out")
    src.write_bytes(fc.case_bytes(case, total_cap))
    res = hb.run(exe, src, dst)
    assert res.returncode == 0, (case["name"], res.returncode, res.stderr)
    return dst.read_bytes()


@pytest.fixture(scope="module")
def cases():
    return fc.hand_cases()


@pytest.fixture(scope="module")
def host_exe():
    exe = hb.host_exe(SRC)
    return exe


@pytest.fixture(scope="module")
def scene_sources():
    return fc.scene_sources()


def test_cases_hold_what_they_are_named_for(cases):
    seen = set()
    for case in cases:
        dec = fr.decide(case["sources"], case["neighbors"], case["tol16"], case["min_support"])
        for i, (support, conflict, kept) in (case["expect"] or {}).items():
            assert np.array_equal(dec[i][0], support) and np.array_equal(dec[i][1], conflict) and np.array_equal(dec[i][2], kept), (case["name"], i)
        seen.add(case["name"])
    assert {"probe_tol16", "probe_tol0", "owner_min1", "owner_min2", "skipped_slots", "count_and_cap", "view_and_scale", "quarter_turn", "wild"} <= seen


def test_probe_case_is_exact(cases):
    """The hand-made plan keeps the probe exact: the two ties project to 10.5 and 15.5, and e is the integer the map holds."""
    case = cases[0]
    s1 = case["sources"][1]
    p = np.asarray(s1["plan"]).reshape(-1)[0]
    for x, want in ((1.0, 10.5), (3.0, 15.5)):
        assert p["fx"] * (x / 16.0) + p["cx"] == want and p["fx"] * p["B"] * 16.0 / 16.0 == 40.0
    assert np.rint(10.5) == 10 and np.rint(15.5) == 16
    assert (case["sources"][0]["xyz"].astype(np.float64)[:4, 2] == 10.0).all() and 40.0 * 16.0 / 10.0 == 64.0


def test_owner_rule_counts(cases):
    by = {c["name"]: statement(c) for c in cases if c["name"].startswith("owner")}
    assert by["owner_min1"]["counts"].tolist() == [12, 10, 3, 25] and by["owner_min2"]["counts"].tolist() == [12, 10, 0, 22]
    one = by["owner_min1"]
    assert one["source"].tolist() == [0] * 12 + [1] * 10 + [2] * 3 and one["support"].tolist() == [3] * 12 + [2] * 10 + [1] * 3
    assert one["index"].tolist() == list(range(12)) + list(range(12, 22)) + list(range(22, 25))


def test_count_above_cap_and_fused_cap(cases):
    case = next(c for c in cases if c["name"] == "count_and_cap")
    got = statement(case)
    assert got["counts"].tolist() == [12, 0, 5, 17] and len(got["points"]) == 14 and got["source"].tolist() == [0] * 12 + [2] * 2
    assert got["points"].tobytes() == np.concatenate([case["sources"][0]["xyz"], case["sources"][2]["xyz"][:2]]).tobytes()
    assert got["colors"].tobytes() == np.concatenate([case["sources"][0]["color"], case["sources"][2]["color"][:2]]).tobytes()


def test_quarter_turn_sources_see_each_other(cases):
    case = next(c for c in cases if c["name"] == "quarter_turn")
    a, b = case["sources"]
    assert a["disp16"].shape == (29, 37) and b["disp16"].shape == (37, 29)
    l = fr.look(a, b["xyz"], 16)
    assert (l == fr.CONSISTENT).all() and len(l) == 37 * 29   # the turned map covers the same pixels of camera 1
    assert statement(case)["counts"].tolist() == [37 * 29, 0, 37 * 29]


def test_wild_inputs_are_unseen(cases):
    case = next(c for c in cases if c["name"] == "wild")
    s0 = case["sources"][0]
    finite_front = np.isfinite(s0["xyz"]).all(axis=1) & (s0["xyz"][:, 2] > 0)
    for j in range(1, len(case["sources"])):
        if fr.is_live(case["sources"][j]):
            l = fr.look(case["sources"][j], s0["xyz"], 16)
            assert (l[~finite_front] == fr.UNSEEN).all(), j
    for j in (2, 4, 5, 6):   # the zeroed plan, the huge t, the NaN view, the denormal scale: nothing is seen at all
        assert (fr.look(case["sources"][j], s0["xyz"], 16) == fr.UNSEEN).all(), j


def test_default_neighbors():
    assert fr.default_neighbors(3).tolist() == [[1, 2], [0, 2], [0, 1]] and fr.default_neighbors(1).tolist() == [[-1]]
    assert fr.default_neighbors(33).shape == (33, 32)
    with pytest.raises(ValueError):
        fr.default_neighbors(34)


def test_host_build_equals_statement(cases, host_exe, tmp_path):
    for case in cases:
        want = statement(case)
        assert run_host(host_exe, case, tmp_path) == fc.result_bytes(want, case["channels"]), case["name"]


def test_host_build_equals_statement_on_scene(scene_sources, host_exe, tmp_path):
    case = fc._case("scene", scene_sources)
    assert run_host(host_exe, case, tmp_path) == fc.result_bytes(statement(case), 1)


def test_stand_alone_program_under_sanitizers(cases, tmp_path):
    exe = hb.host_exe_sanitized(SRC)
    for case in cases:
        assert run_host(exe, case, tmp_path) == fc.result_bytes(statement(case), case["channels"]), case["name"]


def test_layout():
    res = hb.run(hb.host_exe("dense_fuse_layout_check.cpp"))
    assert res.returncode == 0 and res.stdout.strip() == "dense_fuse_layout: ok", res.stdout


def test_scene_figures(scene_sources):
    a, b, c, d = fc.scene_figures(scene_sources)
    print(f"scene: (a) consistent share {a:.4f}, (b) fused / parts {b:.4f}, (c) supported within 1 px {c:.4f}, (d) orphans {d}")
    assert a >= fc.SCENE_CONSISTENT_SHARE_MEASURED - fc.SCENE_MARGIN
    assert b <= fc.SCENE_FUSED_RATIO_MEASURED + fc.SCENE_MARGIN
    assert c >= fc.SCENE_SUPPORTED_SHARE_MEASURED - fc.SCENE_MARGIN
