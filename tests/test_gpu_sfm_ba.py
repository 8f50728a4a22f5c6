"""-m gpu: bundle adjustment behind the registration on the device -- gms_sfm_ba_device on the hand-made inputs of
tests/sfm_ba_cases.py against the numpy statement (tests/sfm_ba_ref.py) fed the same arrays, the same bytes run after run, the one-shot
gms_sfm_ba against the device call, batch.SfmBundle in a captured graph, pipeline.run_dataset(register=True, bundle=True) on the noisy
five-view scene against the statement fed the GPU's own records and against the ground truth, the four photographs, and the refusals
of the C ABI. Integers -- statuses, counts, the accepted iterations -- are exact; views, points and costs are held to 16 times what the
order of the sums is worth in the statement itself (test_sfm_ba_ref.MEASURED_SPREAD), at least 1e-12, relative as close() measures.

The structural edges among the hand-made cases: a cloud of two scan tiles (two_tiles: the tile carry of the prefix sum), more than
256 frames (many_frames: the second pass of every lane-strided loop over the frames), more frames than cloud entries
(frames_past_cap: the frames size the step kernel's grid, and most free frames have no Cholesky factor), a cloud_cap past n_tracks
(cap_past_tracks), two keypoints of a frame found by the sorted neighbours (multi_sorted), KEPT for a singular normal matrix and for
a point behind a camera (kept), dropped steps (rejected_step), conjugate gradients ended by n_cg and by cg_tol (cg_short,
cg_converges), the outer loop ended by ftol and by n_iters (ftol_stops, iters_run_out), pairs and matches that do not fit the
arrays (misfit_records). Still untested: the second pass of sba_scan_kernel, which takes more than 256 tiles -- a cloud of more than
1,048,576 entries, which the statement's per-entry loop cannot state in the suite's time."""
import importlib
import os

import numpy as np
import pytest
import torch

import sfm_ba_cases as cases
import sfm_ba_ref as B
import sfm_register_ref as R
from test_sfm_ba_ref import CASE_NAMES, centre_error, cg_iters_by_both_orders, run_statement, same_result, spread, tolerance
from test_sfm_register_ref import truth_scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def pipeline():
    return importlib.import_module("sfm-gms_amd.pipeline")


@pytest.fixture(scope="module")
def wanted():
    done = {}

    def get(name):
        if name not in done:
            done[name] = run_statement(cases.case(name))
        return done[name]
    return get


def device_call(ctx, batch, c, **kw):
    """batch.bundle_adjust on a case. A case that states its own total_m (misfit_records: the arrays' length, which a pair's match
    range exceeds) goes through the same steps with the job's total_m set to it, instead of the largest match_off + m."""
    args = (c["kp"], c["frame_off"], c["pairs"], c["matches"], c["mask"], c["reg"], c["camera"][:4], c["camera"][4:])
    if "total_m" not in c:
        return batch.bundle_adjust(ctx, *args, **dict(c["params"], **kw))
    job = batch.SfmBundle(ctx, c["frame_off"], c["pairs"], len(c["reg"]["cloud_id"]), c["camera"][:4], c["camera"][4:], **dict(c["params"], **kw))
    job.total_m = int(c["total_m"])
    job.load(c["kp"], c["matches"], c["mask"], c["reg"])
    torch.cuda.synchronize(job.device)
    job.run()
    return job.results()


def statement_and_tolerance(got, frame_off, xy, camera):
    """The statement fed a pipeline result's own records, and the tolerance measured on them: the statement once more with every sum
    reversed must take the same accept / reject sequence; 16 times the largest difference between the two, at least 1e-12."""
    args = (xy, frame_off, got["pairs"], got["out"], got["mask"], got["views"], got["registration"], got["track"], got["cloud"], got["cloud_id"], camera)
    tr, tr_rev = [], []
    n_tracks = int(got["summary"]["n_tracks"][0])             # the registration's, as the device reads it
    want, rev = B.bundle_adjust(*args, trace=tr, n_tracks=n_tracks), B.bundle_adjust(*args, order=-1, trace=tr_rev, n_tracks=n_tracks)
    assert [x[0] for x in tr] == [x[0] for x in tr_rev]
    sp = spread(want, rev)
    print("order spread on the device's records:", sp)
    return want, max(16.0 * sp, 1e-12)


# ---- hand-made inputs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hand_made_cases_equal_the_statement(ctx, batch, wanted, name):
    """two_frames: one free camera and the gauge; three_chain: tracks of two and three; twelve_frames: 66 camera unknowns; wide: a
    frame past one pass of its workgroup and more tracks than one workgroup holds; multi, behind, unregistered, small_cap, the outlier
    with and without Huber, n_iters = 0 with and without re-triangulation; and the structural edges the module's docstring lists:
    two_tiles, many_frames, frames_past_cap, cap_past_tracks, multi_sorted, kept, rejected_step, cg_short, cg_converges, ftol_stops,
    iters_run_out, misfit_records."""
    c, want = cases.case(name), wanted(name)
    got = device_call(ctx, batch, c)
    print(name, got["ba_summary"][0], "statement", want["ba_summary"][0])
    same_result(got, want, tolerance(name), name)


def test_the_observation_lists_are_the_statements(ctx, batch, wanted):
    """The per-track lists cannot be read back through the interface; what depends on them can: re-triangulation alone (n_iters = 0)
    sums each track's rays in list order, and statuses and counts say which tracks and observations take part. two_tiles: lists on
    both sides of the tile boundary, placed by the carry; cap_past_tracks: only the first n_tracks entries are searched;
    multi_sorted: the list of three keypoints, two of one frame, is excluded by its sorted neighbours."""
    for name in ("multi", "wide", "small_cap", "two_tiles", "cap_past_tracks", "multi_sorted"):
        c = cases.case(name)
        got, want = device_call(ctx, batch, c, n_iters=0, retriangulate=1), run_statement(c, n_iters=0, retriangulate=1)
        same_result(got, want, 1e-12, name)


def test_a_track_with_two_keypoints_of_a_frame_keeps_its_bytes(ctx, batch):
    c = cases.case("multi")
    got = device_call(ctx, batch, c)
    e = np.nonzero(got["track_status"] == B.MULTI)[0]
    assert len(e) == 1 and got["ba_summary"]["n_tracks_multi"][0] == 1 and got["ba_summary"]["n_tracks_used"][0] == len(got["track_status"]) - 1
    assert got["cloud_ba"][e[0]].tobytes() == c["reg"]["cloud"][e[0]].tobytes()


def test_cloud_rows_past_n_tracks_are_neither_searched_nor_touched(ctx, batch):
    """cap_past_tracks: the 50 rows behind the registration's n_tracks repeat real ids in no order and hold a fill: status FEW, their
    bytes kept, with and without iterations; and the real entries are three_chain's."""
    c, n = cases.case("cap_past_tracks"), cases.case("cap_past_tracks")["n_real"]
    for kw in (dict(), dict(n_iters=0)):
        got = device_call(ctx, batch, c, **kw)
        assert len(got["track_status"]) == 90 and (got["track_status"][n:] == B.FEW).all() and (got["track_status"][:n] == B.REFINED).all()
        assert got["cloud_ba"][n:].tobytes() == c["reg"]["cloud"][n:].tobytes() and (got["cloud_ba"][n:] == cases.CAP_FILL).all()
        assert got["ba_summary"]["n_tracks_used"][0] == n and got["ba_summary"]["n_obs"][0] == 100
    got, plain = device_call(ctx, batch, c), device_call(ctx, batch, cases.case("three_chain"))
    assert got["cloud_ba"][:n].tobytes() == plain["cloud_ba"].tobytes() and got["views_ba"].tobytes() == plain["views_ba"].tobytes()
    assert got["ba_summary"].tobytes() == plain["ba_summary"].tobytes()


def test_a_refused_re_triangulation_keeps_the_track_and_its_point(ctx, batch):
    """kept: one track's rays are both (0, 0, 1) (a singular normal matrix), another's meet behind the cameras. Status KEPT, counted in
    n_tracks_used, observations counted, and with n_iters = 0 their points are the registration's bytes while every other moved."""
    c = cases.case("kept")
    mine = sorted([c["behind"], c["singular"]])
    for kw in (dict(n_iters=0), dict()):
        got = device_call(ctx, batch, c, **kw)
        assert np.nonzero(got["track_status"] == B.KEPT)[0].tolist() == mine and (np.delete(got["track_status"], mine) == B.REFINED).all()
        assert got["ba_summary"]["n_tracks_used"][0] == len(got["track_status"]) == 41 and got["ba_summary"]["n_obs"][0] == 102
    got = device_call(ctx, batch, c, n_iters=0)
    assert got["cloud_ba"][mine].tobytes() == c["reg"]["cloud"][mine].tobytes()
    assert (np.delete(got["cloud_ba"], mine, 0) != np.delete(c["reg"]["cloud"], mine, 0)).any(1).all()
    off = device_call(ctx, batch, c, n_iters=0, retriangulate=0)
    assert (off["track_status"] == B.REFINED).all() and off["cloud_ba"].tobytes() == c["reg"]["cloud"].tobytes()


@pytest.mark.parametrize("name", ["cg_short", "cg_converges"])
def test_conjugate_gradients_end_where_the_statements_do(ctx, batch, name):
    """cg_iters is outside same_result; on these two cases it is held: equal to the statement's where both orders of its sums agree,
    between the two counts otherwise. cg_short: n_cg = 2 ends each of the 10 solves; cg_converges: cg_tol = 1e-2 ends each."""
    a, b = cg_iters_by_both_orders(name)
    got = int(device_call(ctx, batch, cases.case(name))["ba_summary"]["cg_iters"][0])
    print(name, "cg_iters", got, "statement", a, "reversed", b)
    assert min(a, b) <= got <= max(a, b)


def test_a_point_behind_a_camera_is_inactive_and_counted(ctx, batch):
    c = cases.case("behind")
    got = device_call(ctx, batch, c, n_iters=0)
    assert got["ba_summary"]["n_obs"][0] == 100 and got["ba_summary"]["n_active"][0] == 99
    assert got["cloud_ba"].tobytes() == c["reg"]["cloud"].tobytes()


def test_an_unregistered_frames_zero_view_stays_zero(ctx, batch):
    got = device_call(ctx, batch, cases.case("unregistered"))
    v = got["views_ba"][3]
    assert not v["R"].any() and not v["t"].any() and v["registered"] == 0 and v["pair"] == -1 and got["ba_summary"]["n_frames_free"][0] == 2


def test_nothing_to_do_returns_the_inputs_bytes(ctx, batch):
    c = cases.case("as_is")
    got = device_call(ctx, batch, c)
    assert got["views_ba"].tobytes() == c["reg"]["views"].tobytes() and got["cloud_ba"].tobytes() == c["reg"]["cloud"].tobytes()
    assert got["ba_summary"]["iters_run"][0] == 0 and got["ba_summary"]["cost"][0] == got["ba_summary"]["cost0"][0]


def test_the_same_bytes_run_after_run(ctx, batch):
    """No floating-point atomics: three runs on one object, and one on a fresh object, give the same bytes -- also past one scan tile
    (two_tiles) and past one pass over the frames (many_frames)."""
    for name in ("wide", "twelve_frames", "two_tiles", "many_frames"):
        c = cases.case(name)
        job = batch.SfmBundle(ctx, c["frame_off"], c["pairs"], len(c["reg"]["cloud_id"]), c["camera"][:4], c["camera"][4:], **c["params"])
        job.load(c["kp"], c["matches"], c["mask"], c["reg"])
        seen = set()
        for _ in range(3):
            job.run()
            r = job.results()
            seen.add(b"".join(r[k].tobytes() for k in sorted(r)))
        r = device_call(ctx, batch, c)
        seen.add(b"".join(r[k].tobytes() for k in sorted(r)))
        assert len(seen) == 1, name


# ---- the one-shot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_chain", "multi", "small_cap"])
def test_one_shot_gives_the_device_calls_bytes(ctx, batch, pkg, name):
    c = cases.case(name)
    want = device_call(ctx, batch, c)
    got = pkg.bundleAdjust(c["kp"], c["frame_off"], c["pairs"], c["matches"], c["mask"], c["reg"], c["camera"][:4], c["camera"][4:], **c["params"])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


# ---- a captured graph -----------------------------------------------------------------------------------------------------------------
def test_captured_graph_replayed_on_changed_inputs(ctx, batch, wanted):
    """One SfmBundle over three_chain's pair list, captured once; replayed on that case, on the case with the moved keypoint (the
    same pair list and registration, other keypoints), and on the first again: each input's own result."""
    names = ["three_chain", "outlier_huber", "three_chain"]
    c = cases.case("three_chain")
    job = batch.SfmBundle(ctx, c["frame_off"], c["pairs"], len(c["reg"]["cloud_id"]), c["camera"][:4], c["camera"][4:])
    job.load(c["kp"], c["matches"], c["mask"], c["reg"])
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(stream):
            job.run()                                         # warm-up
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            job.run()
        for which, name in enumerate(names):
            ci = cases.case(name)
            job.load(ci["kp"], ci["matches"], ci["mask"], ci["reg"])
            for t in (job.d_views_out, job.d_cloud_out, job.d_status, job.d_summary):
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            same_result(job.results(), wanted(name), tolerance(name), f"replay {which}: {name}")
    finally:
        ctx.set_stream(None)


# ---- through the pipeline -------------------------------------------------------------------------------------------------------------
def test_run_dataset_bundles_the_noisy_five_view_scene(ctx, pkg, synth, pipeline):
    """The five-view scene with half a pixel of noise, the filter, the two-view stage and the registration on the device, bundle
    adjustment behind them: against the statement fed the GPU's own records, and closer to the ground truth than the registration."""
    io = importlib.import_module("sfm-gms_amd.io")
    _, _, pairs, matches, _, _, _ = truth_scene(synth, None)
    sc = synth.make_multi_view_scene(7, 5, n_kp=400, noise_px=0.5)
    ds = io.Dataset(sc["frames"], sc["sizes"], None, -1, pairs, matches)
    kw = dict(thresholdFactor=0.5, camera=sc["camera"], match=False, register=True)
    got = pipeline.run_dataset(ctx, ds, bundle=True, **kw)
    plain = pipeline.run_dataset(ctx, ds, **kw)
    assert sorted(set(got) - set(plain)) == ["ba_summary", "cloud_ba", "track_status", "views_ba"]
    for k in plain:                                          # bundle=False returns today's dict, and bundle=True the same under it
        assert np.asarray(got[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    frame_off = np.arange(6, dtype=np.int64) * 400
    xy = np.concatenate([np.stack([fr["x"], fr["y"]], 1) for fr in sc["frames"]]).astype(np.float32)
    want, tol = statement_and_tolerance(got, frame_off, xy, tuple(sc["camera"]) + (0.0,) * 5)
    same_result(got, want, tol, "run_dataset")
    s = got["ba_summary"][0]
    before, after = centre_error(sc, got["views"]), centre_error(sc, got["views_ba"])
    print("five views, 0.5 px, on the device:", s, "centre error", before, "->", after)
    assert s["cost"] <= s["cost0"] and after < before and s["n_tracks_used"] > 300
    with pytest.raises(ValueError):
        pipeline.run_dataset(ctx, ds, bundle=True, thresholdFactor=0.5, camera=sc["camera"], match=False)
    with pytest.raises(TypeError):
        pipeline.run_dataset(ctx, ds, bundle=True, n_iter=3, **kw)


# ---- the photographs ------------------------------------------------------------------------------------------------------------------
def test_four_photographs_equal_the_statement_on_the_gpus_own_registration(ctx, pkg, pipeline):
    """Views 1, 2, 3, 4 of the reference's scene, the chain (0,1), (1,2), (2,3) with "gms" at 2000 keypoints: the device's registration
    fed to the statement, compared under the measured tolerance."""
    a, b = np.load(os.path.join(GOLDEN, "image_sfm_pair_1008x756.npz")), np.load(os.path.join(GOLDEN, "image_sfm_more_1008x756.npz"))
    images = np.stack([a["left"], b["second"], b["third"], a["right"]])
    got = pipeline.run_images(ctx, images, tuple(a["camera"]), method="gms", pairs=[(0, 1), (1, 2), (2, 3)], max_keypoints=2000, withRotation=True,
                              withScale=True, register=True, bundle=True, keep_tables=True)
    frames = got["tables"][0]
    kp = frames.d_kp.cpu().numpy().view(pkg.KEYPOINT_DTYPE)[:int(frames.frame_off_host[-1])]
    want, tol = statement_and_tolerance(got, frames.frame_off_host, cases.xy_of(kp), tuple(a["camera"]) + (0.0,) * 5)
    s = got["ba_summary"][0]
    print("photographs:", s, "statuses", np.bincount(got["track_status"], minlength=4).tolist(), "camera 3",
          R.camera_centres(got["views"])[3].tolist(), "->", R.camera_centres(got["views_ba"])[3].tolist())
    same_result(got, want, tol, "photographs")
    multi = pkg.structureFromMotionMulti(images, tuple(a["camera"]), ctx=ctx, max_keypoints=2000, bundle=True)
    for k in ("views_ba", "cloud_ba", "track_status", "ba_summary"):
        assert np.asarray(multi[k]).tobytes() == np.asarray(got[k]).tobytes(), k


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(ctx, pkg, batch):
    """GMS_ERR_BAD_ARG and nothing run: the outputs keep their fill."""
    c = cases.case("three_chain")
    job = batch.SfmBundle(ctx, c["frame_off"], c["pairs"], len(c["reg"]["cloud_id"]), c["camera"][:4], c["camera"][4:])
    job.load(c["kp"], c["matches"], c["mask"], c["reg"])
    o = job._own_inputs()
    outs = (job.d_views_out, job.d_cloud_out, job.d_status, job.d_summary)
    for t in outs:
        t.view(torch.uint8).fill_(0xA5)
    torch.cuda.synchronize()
    good = [job.camera, job.params, o["kp"].data_ptr(), job.d_frame_off.data_ptr(), job.n_frames, job.total_kp, job.d_pairs.data_ptr(), job.n_pairs,
            job.total_m, o["matches"].data_ptr(), o["mask"].data_ptr(), o["views"].data_ptr(), o["reg"].data_ptr(), o["track"].data_ptr(),
            job.cloud_cap, o["cloud"].data_ptr(), o["cloud_id"].data_ptr(), o["summary"].data_ptr(), job.d_ws.data_ptr(), job.ws_bytes] + \
        [t.data_ptr() for t in outs]
    bad = {"no frames": (4, 0), "too many keypoints": (5, 2**31 - 1), "negative pairs": (7, -1), "negative matches": (8, -1), "negative cloud": (14, -1),
           "workspace one byte short": (19, job.ws_bytes - 1), "workspace off its alignment": (18, job.d_ws.data_ptr() + 16)}
    for i in (0, 1, 2, 3, 6, 9, 10, 11, 12, 13, 15, 16, 17, 18, 20, 21, 22, 23):
        bad[f"null pointer {i}"] = (i, None)
    for change in (dict(n_iters=-1), dict(n_cg=0), dict(lambda0=-1e-3), dict(cg_tol=float("nan")), dict(ftol=float("inf")), dict(huber_px=-1.0)):
        bad[f"params {change}"] = (1, pkg.sfm_ba_params(**change))
    for what, (i, v) in bad.items():
        args = list(good)
        args[i] = v
        with pytest.raises(pkg.GmsError) as e:
            ctx.sfm_ba_device(*args)
        assert e.value.code == -1, what
    ctx.synchronize()
    for t in outs:
        assert bool((t.view(torch.uint8) == 0xA5).all())
    ctx.sfm_ba_device(*good)                                   # and the unchanged arguments run
    assert int(job.results()["ba_summary"]["n_tracks_used"][0]) == 40
    # the one-shot: a match range that ends past 2^40 is refused before match_off + m is formed (2^63 - 2 with m = 5 does not fit 64
    # bits); straight to the C call, every pointer good, and the unchanged records run
    past, wraps = c["pairs"].copy(), c["pairs"].copy()
    past["match_off"][1], past["m"][1] = 2 ** 40 - 4, 5
    wraps["match_off"][1], wraps["m"][1] = 2 ** 63 - 2, 5
    with pytest.raises(pkg.GmsError) as e:
        pkg.bundleAdjust(c["kp"], c["frame_off"], wraps, c["matches"], c["mask"], c["reg"], c["camera"][:4], c["camera"][4:])
    assert e.value.code == -1
    lib, reg = pkg.load_library(), c["reg"]
    ins = {k: np.ascontiguousarray(v) for k, v in dict(kp=c["kp"], off=c["frame_off"], m=c["matches"], mask=c["mask"], views=reg["views"],
                                                       reg=reg["registration"], track=reg["track"], cloud=reg["cloud"], ids=reg["cloud_id"]).items()}
    cap = len(ins["ids"])
    for recs in (c["pairs"], past, wraps):
        out = [np.zeros(job.n_frames, pkg.SFM_VIEW_DTYPE), np.zeros((cap, 3)), np.zeros(cap, np.int32), np.zeros(1, pkg.SFM_BA_SUMMARY_DTYPE)]
        code = lib.gms_sfm_ba(job.camera.ctypes.data, job.params.ctypes.data, ins["kp"].ctypes.data, ins["off"].ctypes.data, job.n_frames,
                              recs.ctypes.data, len(recs), ins["m"].ctypes.data, ins["mask"].ctypes.data, ins["views"].ctypes.data,
                              ins["reg"].ctypes.data, ins["track"].ctypes.data, cap, ins["cloud"].ctypes.data, ins["ids"].ctypes.data,
                              int(reg["summary"]["n_tracks"][0]), *(a.ctypes.data for a in out))
        assert code == (0 if recs is c["pairs"] else -1) and bool(out[3]["n_tracks_used"][0]) == (recs is c["pairs"])
