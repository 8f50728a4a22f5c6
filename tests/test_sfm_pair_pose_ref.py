"""CPU: the pair records from views (tests/sfm_pair_pose_ref.py) -- the host build of sfm_pair_pose_core.h
(tests/cpp/sfm_pair_pose_host.cpp, a stand-alone program that reads a case file) against the numpy statement byte for byte, plain and
under sanitizers; the registration's own views giving back each ok pair's two-view pose and scale; what the records are worth on the
rendered plane of tests/dense_fuse_cases.py when a view is wrong; and the argument checks of the public calls."""

import numpy as np
import pytest

import dense_fuse_cases as fc
import sfm_pair_pose_cases as pc
import sfm_pair_pose_ref as pp
import hostbuild as hb

SRC = "sfm_pair_pose_host.cpp"

# Measured here (numpy 2.x, x86-64) on the five-view scene, records from the registration's own views against the two-view records and
# the registration's S: the largest |difference| of R 7.8e-16, of t 3.3e-16, of S relative 1.2e-15; the statement against itself
# with every sum reversed: 3.3e-16. The tolerance is 16 times the latter, at least 1e-12 (the rule of tests/test_gpu_sfm_ba.py).
# On the rendered plane: true views 3782 of 3790 overlap points agree (0.9979, the existing scene's figures exactly) and 4248 points are
# fused; camera 2's centre at 1.05 / 1.1 / 1.2 of the baseline: 3806 of 3836 (0.9922), 1311 of 3873 (0.3385), 7 of 3935 (0.0018) and
# 4224, 6719, 8023 fused. f = 1.1 is the smallest with a share below one half.
SCENE_F = 1.1
SCENE_F_CANDIDATES = (1.05, 1.1, 1.2)
SCENE_SHARE_MARGIN = 0.01


@pytest.fixture(scope="module")
def five(synth):
    return pc.five_view_registration(synth)


@pytest.fixture(scope="module")
def cases(five):
    tv, reg, frame_pairs = five
    return pc.hand_cases(reg["views"], frame_pairs)


def run_host(exe, case, tmp_path):
    name, views, frame_pairs = case
    src, dst = tmp_path / (name + ".in"), tmp_path / (name + ".out")
    src.write_bytes(pp.case_bytes(views, pp.pair_table(frame_pairs)))
    res = hb.run(exe, src, dst)
    assert res.returncode == 0, (name, res.returncode, res.stderr)
    return dst.read_bytes()


def test_cases_hold_what_they_are_named_for(cases):
    by = {c[0]: pc.statement(c) for c in cases}
    assert set(by) == {"five_views", "same_frame", "unregistered", "unregistered_flag", "bad_index", "coincident", "non_finite", "empty"}
    ok = lambda name: (by[name][0]["status"] == pp.GMS_OK).tolist()
    assert all(ok("five_views")) and len(by["five_views"][0]) == 12
    assert ok("same_frame") == [False, False, True, False]
    assert ok("unregistered") == [True, False, False, False, True] and ok("unregistered_flag") == [False, False, True, False]
    assert ok("bad_index") == [False] * 9 + [True, True]
    assert ok("coincident") == [False, False, False, False, True, True]
    nf = ok("non_finite")
    assert nf[:22] == [False] * 22 and nf[22:] == [False, False, False, False] and len(by["empty"][0]) == 0
    for tv, reg in by.values():
        bad = tv["status"] != pp.GMS_OK
        assert (tv["status"] == reg["status"]).all() and (reg["link"] == -1).all()
        assert not tv["R"][bad].any() and not tv["t"][bad].any() and not reg["S"][bad].any()
        assert np.isfinite(tv["R"]).all() and np.isfinite(tv["t"]).all() and (reg["S"][~bad] > 0).all()
        z = tv.copy()
        z["R"], z["t"], z["status"] = 0, 0, 0
        assert not z.tobytes().strip(b"\0")   # no essential matrix, no counts
    tv, reg = by["coincident"]
    assert reg["S"][4] == 0.5 and tv["t"][4].tolist() == [0.0, 0.0, 1.0] and tv["t"][5].tolist() == [0.0, 0.0, -1.0]


def test_host_build_equals_statement(cases, tmp_path):
    exe = hb.host_exe(SRC)
    for case in cases:
        assert run_host(exe, case, tmp_path) == pp.result_bytes(*pc.statement(case)), case[0]


def test_stand_alone_program_under_sanitizers(cases, tmp_path):
    exe = hb.host_exe_sanitized(SRC)
    for case in cases:
        assert run_host(exe, case, tmp_path) == pp.result_bytes(*pc.statement(case)), case[0]


def test_registration_views_reproduce_the_two_view_pose(five):
    """Records from the registration's own views against each ok pair's two-view R, unit t and the registration's S: within 16 times
    what reversing every sum changes in the statement itself, at least 1e-12."""
    tv, reg, frame_pairs = five
    views = pc.as_views(reg["views"])
    got_tv, got_reg = pp.pair_poses(views, frame_pairs)
    rev_tv, rev_reg = pp.pair_poses(views, frame_pairs, reverse=True)
    order = max(np.abs(got_tv["R"] - rev_tv["R"]).max(), np.abs(got_tv["t"] - rev_tv["t"]).max(),
                (np.abs(got_reg["S"] - rev_reg["S"]) / got_reg["S"]).max())
    tol = max(16.0 * order, 1e-12)
    ok = reg["registration"]["status"] == pp.GMS_OK
    assert ok.all() and (got_tv["status"] == pp.GMS_OK).all()
    dR = np.abs(got_tv["R"] - tv["R"]).max()
    dt = np.abs(got_tv["t"] - tv["t"]).max()
    dS = (np.abs(got_reg["S"] - reg["registration"]["S"]) / reg["registration"]["S"]).max()
    print(f"registration views -> records: |dR| {dR:.3g}, |dt| {dt:.3g}, |dS|/S {dS:.3g}; order of the sums {order:.3g}; tolerance {tol:.3g}")
    assert dR <= tol and dt <= tol and dS <= tol


@pytest.fixture(scope="module")
def plane_runs():
    pairs = [(0, 1), (1, 2)]
    return {f: pc.agreement(pc.scene_chain(pc.scene_views(f), pairs)) for f in (1.0,) + SCENE_F_CANDIDATES}


def test_plane_quality_true_views_against_a_wrong_scale(plane_runs):
    """The numpy chain on records from the true views against records from views with camera 2's centre at SCENE_F of the baseline."""
    share = {f: a / n for f, (a, n, _) in plane_runs.items()}
    print("plane:", {f: (v, round(share[f], 4)) for f, v in plane_runs.items()})
    assert SCENE_F == min(f for f in SCENE_F_CANDIDATES if share[f] < 0.5)
    (a_true, _, fused_true), (a_bad, _, fused_bad) = plane_runs[1.0], plane_runs[SCENE_F]
    assert a_true > a_bad and fused_true < fused_bad
    assert abs(share[1.0] - fc.SCENE_CONSISTENT_SHARE_MEASURED) <= SCENE_SHARE_MARGIN


# ---- the public calls' argument checks (refused before any device work) ---------------------------------------------------------------
def _images():
    return [np.zeros((72, 96), np.uint8)] * 3


@pytest.mark.parametrize("kw", [dict(dense_poses="bundle"), dict(dense_poses="pair", dense_pairs=[(0, 2)], bundle=True),
                                dict(dense_pairs=[(0, 2)]), dict(dense_poses="views"), dict(dense_poses=None)])
def test_dense_pose_arguments_are_checked(pkg, kw):
    cam = (90.0, 90.0, 47.5, 35.5)
    with pytest.raises(ValueError, match="dense_poses|dense_pairs"):
        pkg.structureFromMotionMulti(_images(), cam, dense=True, fuse=True, **kw)
    import importlib
    pipeline = importlib.import_module(pkg.__name__ + ".pipeline")
    with pytest.raises(ValueError, match="dense_poses|dense_pairs"):
        pipeline.run_images(None, _images(), cam, dense=True, fuse=True, register=True, **kw)
