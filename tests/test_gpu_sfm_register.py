"""-m gpu: many views into one frame on the device -- gms_sfm_register_device on the hand-made records of
tests/sfm_register_cases.py against the numpy statement (tests/sfm_register_ref.py) fed the same arrays, the one-shot gms_sfm_register
against the device call, pipeline.run_dataset(register=True) on the five-view scene against the statement fed the GPU's own two-view
records and against the ground truth, batch.SfmRegister in a captured graph, the four photographs, and the refusals of the C ABI.
Integers are exact; doubles are held to 1e-9 (the tolerance of the two-view tests), relative to the value, or to the size of the vector
for the entries of a rotation, a translation or a point.

The structural edges among the hand-made cases (DESIGN.md §4.10b lists what each reaches and which wrong answers they catch): more
than 256 pairs, walked from registers (chain_300), with every link's outcome read from global memory (star_300) and every view too,
and a failure carried across the staging boundary (two_branches_300); more than 256 scan tiles (tiles_past_256, also with a capacity
that ends below tile 256); link ratios that differ in every byte, an even count, more links than lanes with 200 equal ratios
(ratio_spread); the first pair out of the root without a model (first_root_pair_fails); device records that do not fit the arrays
(misfit_records) and plan entries the walk cannot follow (bad_plan_links), which must be ignored.

Still untested: frame offsets on the device that descend or pass total_kp (sfr::pair_fits sees them only in the stand-alone host
program); the probe sequence of sfr_flatten_kernel wrapping round the end of its hash table; total_kp near 2^31 - 1 and a
match_off past 2^31 (the arrays would take tens of GB); a median wrong in its lowest three bytes alone, which is 3.7e-9 of its value
at most and near the 1e-9 the doubles are held to; and a captured graph of more than one staging pass or scan pass (the replay test
is chain_roles')."""
import importlib
import os

import numpy as np
import pytest
import torch

import sfm_register_cases as cases
import sfm_register_ref as R
from test_sfm_register_ref import CASE_NAMES, check_against_truth, check_expect, close, run_ref, truth_scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-9


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def pipeline():
    return importlib.import_module("sfm-gms_amd.pipeline")


def same_registration(got, want, what=""):
    """Every integer identical; doubles within TOL. The cloud's spread is a distance between two points that are each good to TOL of
    their size, so it is held to TOL of the size of the cloud."""
    assert got["plan"].tobytes() == want["plan"].tobytes(), what
    n = len(got["track"])                                    # the device's arrays end with the last pair's range; the statement's may go on, empty
    assert len(got["points_world"]) == n <= len(want["track"]) and (want["track"][n:] == -1).all() and not want["points_world"][n:].any(), what
    want = dict(want, track=want["track"][:n], points_world=want["points_world"][:n])
    for f in ("n_links", "depth", "link", "role", "status", "reserved"):
        assert np.array_equal(got["registration"][f], want["registration"][f]), (what, f, got["registration"][f], want["registration"][f])
    for f in ("registered", "pair"):
        assert np.array_equal(got["views"][f], want["views"][f]), (what, f)
    for k in ("track", "cloud_id", "cloud_obs", "cloud_est"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k)
    assert got["summary"].tobytes() == want["summary"].tobytes(), (what, got["summary"], want["summary"])
    assert close(got["registration"]["r"], want["registration"]["r"], TOL) and close(got["registration"]["S"], want["registration"]["S"], TOL), what
    assert close(got["views"]["R"], want["views"]["R"], TOL, 1.0) and close(got["views"]["t"], want["views"]["t"], TOL, 1.0), what
    assert close(got["points_world"], want["points_world"], TOL, 1.0) and close(got["cloud"], want["cloud"], TOL, 1.0), what
    finite = want["cloud"][np.isfinite(want["cloud"])]
    size = 1.0 + (np.abs(finite).max() if finite.size else 0.0)
    assert close(got["cloud_spread"], want["cloud_spread"], TOL, size), what


def want_of(c, **kw):
    """The statement fed the arrays the device is fed: for the cases of cases.UNFIT the device's records, its plan and the arrays' length."""
    return run_ref(c, **kw)


@pytest.fixture(scope="module")
def wanted():
    done = {}

    def get(name):
        if name not in done:
            done[name] = want_of(cases.case(name))
        return done[name]
    return get


def job_of(ctx, batch, c, plan=None, cloud_cap=None):
    """A loaded batch.SfmRegister on a case, with the cloud capacity the case states. The host's pair list makes the plan, total_m and
    max_m; a case with `host_pairs` (misfit_records) puts other records on the device through d_pairs, and a case with `plan`
    (bad_plan_links; or `plan` here) overwrites the device's plan after construction -- and the host's copy, which results() returns."""
    cap = c.get("cloud_cap") if cloud_cap is None else cloud_cap
    d_pairs = None
    if "host_pairs" in c:
        d_pairs = torch.from_numpy(np.ascontiguousarray(c["pairs"]).view(np.uint8).reshape(-1)).to(f"cuda:{ctx.device}")
    job = batch.SfmRegister(ctx, c["frame_off"], c.get("host_pairs", c["pairs"]), c["root"], c["min_links"], cap, d_pairs=d_pairs)
    assert job.total_m == c.get("total_m", job.total_m)
    plan = c.get("plan") if plan is None else plan
    if plan is not None:
        assert plan.dtype == job.plan.dtype and len(plan) == job.n_pairs
        job.plan = plan.copy()
        job.d_plan.copy_(torch.from_numpy(np.ascontiguousarray(plan).view(np.uint8).reshape(-1)))
    job.load(c["matches"], c["mask"], c["points3d"], c["tv"])
    torch.cuda.synchronize(job.device)
    return job


def device_call(ctx, batch, c, **kw):
    if "host_pairs" in c or "plan" in c or "plan" in kw:
        job = job_of(ctx, batch, c, **kw)
        job.run()
        return job.results()
    kw.setdefault("cloud_cap", c.get("cloud_cap"))
    return batch.register_pairs(ctx, c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], **kw)


# ---- hand-made records ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hand_made_records_equal_the_statement(ctx, batch, wanted, name):
    c = cases.case(name)
    got = device_call(ctx, batch, c)
    same_registration(got, wanted(name), name)
    for i, (status, n_links, S) in c["expect"].items():      # and the analytic scales, at the device's tolerance
        assert got["registration"][i]["status"] == status and abs(got["registration"][i]["S"] - S) <= TOL * S
        assert n_links is None or got["registration"][i]["n_links"] == n_links


def test_the_same_result_run_after_run(ctx, batch):
    """Every atomic is an integer minimum, maximum or sum: three runs on one object give the same bytes -- also with a walk of two
    staging passes that reads global memory at every step, and with a scan of two passes."""
    for name in ("many_links", "two_branches_300", "tiles_past_256"):
        job = job_of(ctx, batch, cases.case(name))
        seen = set()
        for _ in range(3):
            job.run()
            r = job.results()
            seen.add(b"".join(r[k].tobytes() for k in sorted(r)))
        assert len(seen) == 1, name


def test_a_capacity_that_ends_below_tile_256_keeps_the_first_tracks_and_writes_nothing_behind(ctx, batch, wanted):
    """tiles_past_256 with room for 20 tracks, fewer than its ids below tile 256: n_tracks still counts all 60 (the scan's second pass
    and its carry), the 20 entries are the statement's first 20, and the cloud arrays -- 64 entries long here -- keep behind them the
    fill they held before the call."""
    c, want = cases.case("tiles_past_256"), wanted("tiles_past_256")
    assert int((want["cloud_id"] // 4096 < 256).sum()) > 20
    job = job_of(ctx, batch, c, cloud_cap=20)
    dev = job.device
    job.d_cloud = torch.full((64 * 3,), -7.0, dtype=torch.float64, device=dev)
    job.d_cloud_id, job.d_cloud_obs, job.d_cloud_est = (torch.full((64,), -7, dtype=torch.int32, device=dev) for _ in range(3))
    job.d_cloud_spread = torch.full((64,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    job.run()
    got = job.results(trim=False)
    assert got["summary"].tobytes() == want["summary"].tobytes() and got["summary"]["n_tracks"][0] == 60 and len(got["cloud_id"]) == 20
    assert np.array_equal(got["cloud_id"], want["cloud_id"][:20]) and np.array_equal(got["cloud_obs"], want["cloud_obs"][:20])
    assert np.array_equal(got["cloud_est"], want["cloud_est"][:20]) and close(got["cloud"], want["cloud"][:20], TOL, 1.0)
    assert np.array_equal(got["track"], want["track"][:len(got["track"])])
    for t in (job.d_cloud[60:], job.d_cloud_id[20:], job.d_cloud_obs[20:], job.d_cloud_est[20:], job.d_cloud_spread[20:]):
        assert bool((t == -7).all())


def test_misfit_records_leave_chain_roles_bytes(ctx, batch):
    """Beside the comparison with the statement (test_hand_made_records_equal_the_statement): the device's own result on chain_roles
    comes back byte for byte around the records that do not fit, each of which ends skipped with zeros."""
    c, base = cases.case("misfit_records"), cases.case("chain_roles")
    got, plain = device_call(ctx, batch, c), device_call(ctx, batch, base)
    n0, f0, m0 = c["n_base_pairs"], c["n_base_frames"], len(plain["track"])
    check_expect(c, got["registration"], c["expect"])
    assert got["registration"][:n0].tobytes() == plain["registration"].tobytes() and got["views"][:f0].tobytes() == plain["views"].tobytes()
    assert not got["views"]["registered"][f0:].any() and (got["views"]["pair"][f0:] == -1).all() and not got["views"]["R"][f0:].any()
    for k in ("cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary"):
        assert got[k].tobytes() == plain[k].tobytes(), k
    assert got["track"][:m0].tobytes() == plain["track"].tobytes() and got["points_world"][:m0].tobytes() == plain["points_world"].tobytes()
    assert (got["track"][m0:] == -1).all() and not got["points_world"][m0:].any()


def test_plan_entries_the_walk_cannot_follow(ctx, batch):
    """bad_plan_links' further plans (its first is among the hand-made cases): link -2, link n_pairs + 5, and the first pair out of the
    root with link -2, each against the statement given the same plan and against the stated outcome."""
    c = cases.case("bad_plan_links")
    for given, expect in c["more_plans"]:
        got = device_call(ctx, batch, c, plan=given)
        same_registration(got, want_of(c, plan=given), "bad plan")
        check_expect(c, got["registration"], expect)


def test_a_small_cloud_capacity_keeps_the_first_tracks(ctx, batch, wanted):
    c, want = cases.case("chain_roles"), wanted("chain_roles")
    got = device_call(ctx, batch, c, cloud_cap=7)
    assert got["summary"].tobytes() == want["summary"].tobytes() and len(got["cloud_id"]) == 7
    assert np.array_equal(got["cloud_id"], want["cloud_id"][:7]) and np.array_equal(got["cloud_est"], want["cloud_est"][:7])
    assert close(got["cloud"], want["cloud"][:7], TOL, 1.0) and np.array_equal(got["track"], want["track"][:len(got["track"])])


def test_no_pairs_and_no_matches(ctx, batch, pkg):
    got = batch.register_pairs(ctx, np.array([0, 5, 9], np.int64), np.zeros(0, pkg.PAIR_DTYPE), np.zeros(0, pkg.DMATCH_DTYPE), np.zeros(0, np.uint8),
                               np.zeros((0, 3)), np.zeros(0, cases.TWO_VIEW_DTYPE), root=1)
    assert got["views"]["registered"].tolist() == [0, 1] and np.array_equal(got["views"][1]["R"], np.eye(3))
    assert got["summary"][0].tolist() == (0, 0, 0, 1, 0) and len(got["cloud_id"]) == 0
    c = cases.case("upstream_failures")
    empty = {k: c[k] for k in ("frame_off", "pairs", "matches", "mask", "points3d", "root", "min_links")}
    empty["tv"] = c["tv"].copy()
    empty["tv"]["n_points"] = 0                                # every pair without a match
    same_registration(device_call(ctx, batch, empty), want_of(empty), "no matches")


# ---- the one-shot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain_roles", "invalid_links_and_min_links", "upstream_failures"])
def test_one_shot_gives_the_device_calls_bytes(ctx, batch, pkg, name):
    c = cases.case(name)
    want = device_call(ctx, batch, c)
    got = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


# ---- through the pipeline -------------------------------------------------------------------------------------------------------------
def test_run_dataset_registers_the_five_view_scene(ctx, pkg, synth, pipeline):
    """The scene of the CPU test with its keypoints and its putative matches (20 % of them wrong). The filter runs at thresholdFactor
    0.5, where it keeps nearly every match (the CPU statement of the filter keeps 352 to 377 of each pair's 400, about 300 of them
    right), so that RANSAC meets the wrong ones; the two-view stage and the registration follow on the device."""
    io = importlib.import_module("sfm-gms_amd.io")
    sc, frame_pairs, pairs, matches, _, _, _ = truth_scene(synth, None)
    ds = io.Dataset(sc["frames"], sc["sizes"], None, -1, pairs, matches)
    kw = dict(thresholdFactor=0.5, camera=sc["camera"], match=False)
    got = pipeline.run_dataset(ctx, ds, register=True, **kw)
    plain = pipeline.run_dataset(ctx, ds, **kw)
    assert sorted(set(got) - set(plain)) == sorted(["views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est",
                                                    "cloud_spread", "summary", "register_plan"])
    for k in plain:                                          # register=False returns today's dict, and register=True the same under it
        assert np.asarray(got[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    frame_off = np.arange(6, dtype=np.int64) * 400
    want = R.register(frame_off, got["pairs"], got["out"], got["mask"], got["points3d"], got["two_view"])
    same_registration(dict(got, plan=got["register_plan"]), want, "run_dataset")
    check_against_truth(sc, got)
    assert len(got["points_world"]) == len(got["points3d"]) and got["summary"]["n_tracks"][0] == len(got["cloud_id"]) > 300


def test_register_needs_a_camera_and_a_frame_for_a_root(ctx, pkg, synth, pipeline):
    io = importlib.import_module("sfm-gms_amd.io")
    sc, _, pairs, matches, _, _, _ = truth_scene(synth, None)
    ds = io.Dataset(sc["frames"], sc["sizes"], None, -1, pairs, matches)
    with pytest.raises(ValueError):
        pipeline.run_dataset(ctx, ds, register=True, match=False)
    with pytest.raises(ValueError):
        pipeline.run_dataset(ctx, ds, register=True, match=False, camera=sc["camera"], min_links=0)
    with pytest.raises((ValueError, pkg.GmsError)):
        pipeline.run_dataset(ctx, ds, register=True, match=False, camera=sc["camera"], root=5)
    with pytest.raises(ValueError):
        pipeline.run_images(None, np.zeros((2, 64, 64), np.uint8), camera=sc["camera"], register=True, root=2)


# ---- a captured graph -----------------------------------------------------------------------------------------------------------------
def test_captured_graph_replayed_on_changed_inputs(ctx, batch, wanted):
    """One SfmRegister over the pair list of chain_roles, captured once; replayed on that case's records with every point of pair 1
    halved (its scale doubles), on records where pair 2 has no model, and on the first again: each input's own result."""
    c = cases.case("chain_roles")
    second = dict(c, points3d=c["points3d"].copy())
    o, m = int(c["pairs"][1]["match_off"]), int(c["pairs"][1]["m"])
    second["points3d"][o:o + m] *= 0.5
    second["tv"] = c["tv"].copy()
    second["tv"]["t"][1] *= 0.5
    third = dict(c, tv=c["tv"].copy())
    third["tv"]["status"][2] = -8
    inputs = [c, second, third, c]
    want = [wanted("chain_roles"), want_of(second), want_of(third), wanted("chain_roles")]
    assert abs(want[1]["registration"][1]["S"] / 5.0 - 1) < 1e-12 and want[2]["registration"]["status"].tolist() == [0, 0, -8, 1, 1, 1, -8]
    job = batch.SfmRegister(ctx, c["frame_off"], c["pairs"], c["root"], c["min_links"])
    job.load(c["matches"], c["mask"], c["points3d"], c["tv"])
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(stream):
            job.run()                                         # warm-up
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            job.run()
        for which, case_in in enumerate(inputs):
            job.load(case_in["matches"], case_in["mask"], case_in["points3d"], case_in["tv"])
            for t in (job.d_views, job.d_reg, job.d_world, job.d_track, job.d_cloud, job.d_cloud_id, job.d_cloud_obs, job.d_cloud_est,
                      job.d_cloud_spread, job.d_summary):
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            same_registration(job.results(), want[which], f"replay {which}")
    finally:
        ctx.set_stream(None)


# ---- the photographs ------------------------------------------------------------------------------------------------------------------
def test_four_photographs_equal_the_statement_on_the_gpus_own_records(ctx, pkg, pipeline):
    """Views 1, 2, 3, 4 of the reference's scene (the committed pair holds 1 and 4, image_sfm_more_1008x756.npz 2 and 3), the chain
    (0,1), (1,2), (2,3) at 2000 keypoints: whatever statuses come out, the registration equals the statement fed the GPU's two-view
    records."""
    a, b = np.load(os.path.join(GOLDEN, "image_sfm_pair_1008x756.npz")), np.load(os.path.join(GOLDEN, "image_sfm_more_1008x756.npz"))
    images = np.stack([a["left"], b["second"], b["third"], a["right"]])
    chain = [(0, 1), (1, 2), (2, 3)]
    got = pipeline.run_images(ctx, images, tuple(a["camera"]), method="gms", pairs=chain, max_keypoints=2000, withRotation=True, withScale=True,
                              register=True, keep_tables=True)
    frame_off = got["tables"][0].frame_off_host
    want = R.register(frame_off, got["pairs"], got["out"], got["mask"], got["points3d"], got["two_view"])
    same_registration(dict(got, plan=got["register_plan"]), want, "photographs")
    reg = got["registration"]
    print("photographs: two-view status", got["two_view"]["status"].tolist(), "n_links", reg["n_links"].tolist(), "r", reg["r"].tolist(), "S",
          reg["S"].tolist(), "status", reg["status"].tolist(), "summary", got["summary"][0].tolist(),
          "tracks by keypoints", np.bincount(got["cloud_obs"], minlength=5)[2:].tolist())
    multi = pkg.structureFromMotionMulti(images, tuple(a["camera"]), ctx=ctx, max_keypoints=2000)   # the chain and matchGMS(true, true) by default
    for k in ("views", "registration", "points_world", "track", "cloud", "cloud_obs", "cloud_est", "cloud_spread", "summary"):
        assert np.asarray(multi[k]).tobytes() == np.asarray(got[k]).tobytes(), k


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(ctx, pkg, batch):
    """GMS_ERR_BAD_ARG and nothing run: the outputs keep their fill."""
    c = cases.case("lowest_k_wins")
    job = batch.SfmRegister(ctx, c["frame_off"], c["pairs"], c["root"], c["min_links"])
    job.load(c["matches"], c["mask"], c["points3d"], c["tv"])
    d_m, d_mask, d_pts, d_tv = job._own_inputs()
    outs = (job.d_views, job.d_reg, job.d_world, job.d_track, job.d_cloud, job.d_cloud_id, job.d_cloud_obs, job.d_cloud_est, job.d_cloud_spread,
            job.d_summary)
    for t in outs:
        t.view(torch.uint8).fill_(0xA5)
    torch.cuda.synchronize()
    good = [job.d_frame_off.data_ptr(), job.n_frames, job.total_kp, job.d_pairs.data_ptr(), job.d_plan.data_ptr(), job.n_pairs, job.max_m,
            job.total_m, d_m.data_ptr(), d_mask.data_ptr(), d_pts.data_ptr(), d_tv.data_ptr(), job.root, job.min_links, job.d_ws.data_ptr(),
            job.ws_bytes] + [t.data_ptr() for t in outs[:4]] + [job.cloud_cap] + [t.data_ptr() for t in outs[4:]]
    bad = {"root below": (12, -1), "root past the frames": (12, job.n_frames), "min_links 0": (13, 0), "workspace one byte short": (15, job.ws_bytes - 1),
           "workspace off its alignment": (14, job.d_ws.data_ptr() + 16), "no frames": (1, 0), "negative pairs": (5, -1), "negative cloud": (20, -1),
           "too many keypoints": (2, 2**31 - 1)}
    for i in (0, 3, 4, 8, 9, 10, 11, 14, 16, 17, 18, 19, 21, 22, 23, 24, 25, 26):
        bad[f"null pointer {i}"] = (i, None)
    for what, (i, v) in bad.items():
        args = list(good)
        args[i] = v
        with pytest.raises(pkg.GmsError) as e:
            ctx.sfm_register_device(*args)
        assert e.value.code == -1, what
    lib = pkg.load_library()
    assert lib.gms_sfm_register_device(None, *good) == -1
    ctx.synchronize()
    for t in outs:
        assert bool((t.view(torch.uint8) == 0xA5).all())
    # the one-shot: a pair's frame index out of range, the root, min_links, null arrays
    args = dict(frame_off=c["frame_off"], pairs=c["pairs"], matches=c["matches"], mask=c["mask"], points3d=c["points3d"], two_view=c["tv"])
    wrong = c["pairs"].copy()
    wrong["frame_b"][1] = 3
    # ... and a match range that ends past 2^40, refused before match_off + m is formed: 2^63 - 2 with m = 5 does not fit 64 bits
    past, wraps = c["pairs"].copy(), c["pairs"].copy()
    past["match_off"][1], past["m"][1] = 2 ** 40 - 4, 5
    wraps["match_off"][1], wraps["m"][1] = 2 ** 63 - 2, 5
    for change in (dict(pairs=wrong), dict(root=3), dict(root=-1), dict(min_links=0), dict(cloud_cap=-1), dict(pairs=wraps)):
        with pytest.raises(pkg.GmsError) as e:
            pkg.registerViews(**dict(args, **change))
        assert e.value.code == -1, change
    api = importlib.import_module("sfm-gms_amd.api")
    ins = [np.ascontiguousarray(c[k]) for k in ("matches", "mask", "points3d", "tv")]
    for recs in (c["pairs"], past, wraps):                     # (straight to the C call, every pointer good: the arrays end far before 2^40)
        o = api.sfm_outputs(len(c["frame_off"]) - 1, len(recs), len(c["mask"]), 10)
        code = lib.gms_sfm_register(c["frame_off"].ctypes.data, len(c["frame_off"]) - 1, recs.ctypes.data, len(recs), *(a.ctypes.data for a in ins),
                                    c["root"], c["min_links"], *(o[k].ctypes.data for k in ("views", "registration", "points_world", "track")), 10,
                                    *(o[k].ctypes.data for k in ("cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")))
        assert code == (0 if recs is c["pairs"] else -1) and bool(o["summary"]["n_ok_pairs"][0]) == (recs is c["pairs"])
    ctx.sfm_register_device(*good)                             # and the unchanged arguments run
    ctx.synchronize()
    assert int(job.results()["summary"]["n_ok_pairs"][0]) == 2
