"""-m gpu: one-to-one matches per pair and the registration on them, on the device -- gms_match_unique_device on the
hand-made lists of tests/match_unique_cases.py and on registration cases with redirected train indices against the numpy statement
(tests/match_unique_ref.py), byte for byte on keep and counts; gms_sfm_register_keep_device against register_keep as the registration
itself is held to its statement; a null plane against the existing entry point; the one-shots; MatchUnique -> SfmRegister -> SfmBundle
in one captured graph; the pipeline with unique=True; the four photographs; and the refusals of the C ABI."""
import importlib
import os

import numpy as np
import pytest
import torch

import match_unique_cases as ucases
import match_unique_ref as U
import sfm_ba_cases as bcases
import sfm_register_cases as rcases
import sfm_register_ref as R
from test_gpu_sfm_ba import statement_and_tolerance
from test_gpu_sfm_register import same_registration
from test_sfm_ba_ref import same_result
from test_sfm_register_ref import truth_scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILL = 7                                                       # what d_keep holds before a call: a slot the call does not write shows
REGISTER_ARRAYS = ("plan", "views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")
UNTOUCHED = ("views", "registration", "points_world")


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def pipeline():
    return importlib.import_module("sfm-gms_amd.pipeline")


def redirected(name):
    c = U.redirect_trains(rcases.case(name), 0.3, 77)
    return dict(c, total_m=c.get("total_m", len(c["mask"])))


def unique_job(ctx, batch, c):
    """A loaded batch.MatchUnique on a case; d_keep filled with FILL. A case with `host_pairs` (the misfits: the host sizes its buffers
    by sane records) puts the case's records on the device through d_pairs; one without `host_pairs` whose records do not fit sizes
    the buffers by the case's total_m."""
    host = c.get("host_pairs", c["pairs"])
    d_pairs = None
    if host is not c["pairs"]:
        d_pairs = torch.from_numpy(np.ascontiguousarray(c["pairs"]).view(np.uint8).reshape(-1)).to(f"cuda:{ctx.device}")
    job = batch.MatchUnique(ctx, c["frame_off"], host, d_pairs=d_pairs, total_m=c["total_m"])
    assert job.total_m == c["total_m"]
    job.load(c["matches"][:job.total_m], None if c["mask"] is None else c["mask"][:job.total_m], c["tv"])
    job.d_keep.fill_(FILL)
    torch.cuda.synchronize(job.device)
    return job


def statement_with_fill(c):
    """The statement's keep with FILL in the slots of no fitting pair -- what the device call leaves of a plane that held FILL."""
    keep, counts = U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"], c["total_m"])
    out = np.full(c["total_m"], FILL, np.uint8)
    for p in c["pairs"]:
        if R.pair_fits(p, c["frame_off"], c["total_m"]):
            off, m = int(p["match_off"]), int(p["m"])
            out[off:off + m] = keep[off:off + m]
    return out, counts


def sane_host_pairs(c):
    """For the rule case `misfits`: records of the same count whose ranges the host can size its buffers by (the fitting pair's)."""
    host = c["pairs"].copy()
    host[:] = c["pairs"][0]
    host["match_off"][-1], host["m"][-1] = c["total_m"] - 1, 1   # (the arrays' length, as the case states it)
    return host


def gpu_case(name):
    c = ucases.case(name)
    return dict(c, host_pairs=sane_host_pairs(c)) if name == "misfits" else c


# ---- the keep plane -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ucases.CASES))
def test_hand_made_lists_equal_the_statement(ctx, batch, name):
    c = gpu_case(name)
    job = unique_job(ctx, batch, c)
    job.run()
    keep, counts = job.results()
    want_keep, want_counts = statement_with_fill(c)
    assert keep.tobytes() == want_keep.tobytes() and counts.tobytes() == want_counts.tobytes(), (name, counts.tolist(), want_counts.tolist())
    for i, ks in c["expect"].items():                         # and the winners the case states
        off, m = int(c["pairs"][i]["match_off"]), int(c["pairs"][i]["m"])
        assert np.nonzero(keep[off:off + m] == 1)[0].tolist() == ks, (name, i)


@pytest.mark.parametrize("name", ["chain_roles", "tiles_past_256", "chain_300", "misfit_records"])
def test_registration_cases_with_redirected_trains_equal_the_statement(ctx, batch, name):
    c = redirected(name)
    job = unique_job(ctx, batch, c)
    seen = set()
    for _ in range(2):                                         # integer minima: the same bytes run after run
        job.d_keep.fill_(FILL)
        job.run()
        keep, counts = job.results()
        seen.add(keep.tobytes() + counts.tobytes())
    want_keep, want_counts = statement_with_fill(c)
    assert keep.tobytes() == want_keep.tobytes() and counts.tobytes() == want_counts.tobytes(), name
    assert len(seen) == 1 and (counts[:, 1] < counts[:, 0]).any()


def test_one_shots_equal_the_device_call(ctx, batch, pkg):
    for name in ("equal_distances", "two_view_cuts", "no_mask_no_tv", "star", "empty_pair", "no_pairs"):
        c = ucases.case(name)
        want_keep, want_counts = batch.unique_matches(ctx, c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"])
        lib = pkg.load_library()
        keep, counts = np.full(c["total_m"], FILL, np.uint8), np.full((len(c["pairs"]), 2), FILL, np.int32)
        ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
        assert lib.gms_match_unique(c["frame_off"].ctypes.data, len(c["frame_off"]) - 1, ptr(c["pairs"]), len(c["pairs"]), ptr(c["matches"]),
                                    ptr(c["mask"]), ptr(c["tv"]), keep.ctypes.data, counts.ctypes.data) == 0
        n = len(want_keep)                                     # (the one-shot's arrays end with the last pair's range)
        assert keep[:n].tobytes() == want_keep.tobytes() and counts.tobytes() == want_counts.tobytes(), name
        assert (keep[n:] == FILL).all()
        s_keep, s_counts = U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"], c["total_m"])
        assert keep[:n].tobytes() == s_keep[:n].tobytes() and counts.tobytes() == s_counts.tobytes(), name
    c = ucases.case("equal_distances")
    off, m = int(c["pairs"][0]["match_off"]), int(c["pairs"][0]["m"])
    keep, (live, kept) = pkg.uniqueMatches(c["matches"][off:off + m], 8, 9, c["mask"][off:off + m])
    assert np.nonzero(keep)[0].tolist() == c["expect"][0] and (live, kept) == (7, 4)
    keep, (live, kept) = pkg.uniqueMatches(c["matches"][off:off + m], 8, 9)
    assert np.nonzero(keep)[0].tolist() == c["expect"][0]


# ---- the registration on a plane ----------------------------------------------------------------------------------------------------
def register_on(ctx, batch, c, keep):
    """batch.SfmRegister on a registration case, as test_gpu_sfm_register.job_of loads it, with a host keep plane (None: without)."""
    d_pairs = None
    if "host_pairs" in c:
        d_pairs = torch.from_numpy(np.ascontiguousarray(c["pairs"]).view(np.uint8).reshape(-1)).to(f"cuda:{ctx.device}")
    job = batch.SfmRegister(ctx, c["frame_off"], c.get("host_pairs", c["pairs"]), c["root"], c["min_links"], c.get("cloud_cap"), d_pairs=d_pairs,
                            keep=None if keep is None else True)
    if "plan" in c:
        job.plan = c["plan"].copy()
        job.d_plan.copy_(torch.from_numpy(np.ascontiguousarray(c["plan"]).view(np.uint8).reshape(-1)))
    job.load(c["matches"], c["mask"], c["points3d"], c["tv"], keep)
    torch.cuda.synchronize(job.device)
    job.run()
    return job.results()


def statement_on(c, keep):
    kw = {k: c[k] for k in ("plan", "total_m") if k in c}
    return U.register_keep(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], keep=keep, **kw)


@pytest.mark.parametrize("name", ["chain_roles", "tiles_past_256", "chain_300", "misfit_records", "lowest_k_wins"])
def test_registration_on_the_plane_equals_the_statement(ctx, batch, name):
    c = redirected(name)
    job = unique_job(ctx, batch, c)
    job.run()
    keep, counts = job.results()
    got, plain = register_on(ctx, batch, c, keep), register_on(ctx, batch, c, None)
    want = statement_on(c, keep)
    same_registration(got, want, name)
    for k in UNTOUCHED:                                        # the plane is not read for them: the bytes of the call without
        assert got[k].tobytes() == plain[k].tobytes(), (name, k)
    ok = got["registration"]["status"] == 0
    assert got["summary"]["n_points"][0] == counts[ok, 1].sum() == (got["track"] >= 0).sum() < plain["summary"]["n_points"][0]
    if "plan" not in c:                                        # the library's own plan: a tree
        assert got["summary"]["n_multi"][0] == 0 < plain["summary"]["n_multi"][0]


def test_a_null_plane_gives_the_existing_entry_points_bytes(ctx, batch, pkg):
    c = redirected("chain_roles")
    plain = register_on(ctx, batch, c, None)
    job = batch.SfmRegister(ctx, c["frame_off"], c["pairs"], c["root"], c["min_links"])
    job.load(c["matches"], c["mask"], c["points3d"], c["tv"])
    d_m, d_mask, d_pts, d_tv = job._own_inputs()
    outs = (job.d_views, job.d_reg, job.d_world, job.d_track, job.d_cloud, job.d_cloud_id, job.d_cloud_obs, job.d_cloud_est, job.d_cloud_spread,
            job.d_summary)
    args = [job.d_frame_off.data_ptr(), job.n_frames, job.total_kp, job.d_pairs.data_ptr(), job.d_plan.data_ptr(), job.n_pairs, job.max_m,
            job.total_m, d_m.data_ptr(), d_mask.data_ptr(), d_pts.data_ptr(), d_tv.data_ptr(), job.root, job.min_links, job.d_ws.data_ptr(),
            job.ws_bytes] + [t.data_ptr() for t in outs[:4]] + [job.cloud_cap] + [t.data_ptr() for t in outs[4:]]
    lib = pkg.load_library()
    torch.cuda.synchronize()
    assert lib.gms_sfm_register_keep_device(ctx._h, *args, None) == 0
    null = job.results()
    for k in REGISTER_ARRAYS:
        assert null[k].tobytes() == plain[k].tobytes(), k
    one = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    for k in REGISTER_ARRAYS:
        assert one[k].tobytes() == plain[k].tobytes(), k
    # a plane of ones changes nothing either, and the one-shots with a plane equal the device call with it
    keep, _ = batch.unique_matches(ctx, c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"])
    ones = register_on(ctx, batch, c, np.ones(len(c["mask"]), np.uint8))
    for k in REGISTER_ARRAYS:
        assert ones[k].tobytes() == plain[k].tobytes(), k
    want = register_on(ctx, batch, c, keep)
    for got in (pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], keep=keep),
                batch.register_pairs(ctx, c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], keep=keep)):
        for k in REGISTER_ARRAYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert want["track"].tobytes() != plain["track"].tobytes()


# ---- a captured graph ---------------------------------------------------------------------------------------------------------------
def test_unique_register_bundle_in_one_captured_graph(ctx, batch):
    """MatchUnique -> SfmRegister on its plane -> SfmBundle, captured once over three_chain's pair list and replayed on its matches with
    train indices redirected two ways and on the first again: each input's own result, equal to the uncaptured calls."""
    base = bcases.case("three_chain")
    inputs = [U.redirect_trains(base, 0.2, seed) for seed in (3, 4)]
    inputs.append(inputs[0])
    cam = base["camera"]
    uq = batch.MatchUnique(ctx, base["frame_off"], base["pairs"])
    reg = batch.SfmRegister(ctx, base["frame_off"], base["pairs"], base["root"], base["min_links"], keep=uq.d_keep)
    ba = batch.SfmBundle(ctx, base["frame_off"], base["pairs"], reg.cloud_cap, cam[:4], cam[4:], n_iters=3)
    dev = reg.device
    d_kp = torch.from_numpy(np.ascontiguousarray(base["kp"]).view(np.uint8).reshape(-1)).to(dev)
    reg.load(base["matches"], base["mask"], base["points3d"], base["tv"])
    d_m, d_mask, d_pts, d_tv = reg._own_inputs()

    def chain():
        uq.run(d_m, d_mask, d_tv)
        reg.run()
        ba.run(reg, d_kp, d_m, d_mask)

    def read():
        keep, counts = uq.results()
        r = reg.results()
        return dict(r, keep=keep, counts=counts, **ba.results(len(r["cloud_id"])))
    plain = []
    for c in inputs[:2]:                                       # the uncaptured calls
        reg.load(c["matches"], c["mask"], c["points3d"], c["tv"])
        torch.cuda.synchronize()
        chain()
        plain.append(read())
    plain.append(plain[0])
    assert plain[0]["keep"].tobytes() != plain[1]["keep"].tobytes()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(stream):
            chain()                                           # warm-up
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            chain()
        for which, c in enumerate(inputs):
            reg.load(c["matches"], c["mask"], c["points3d"], c["tv"])
            for t in (uq.d_keep, uq.d_counts, reg.d_views, reg.d_reg, reg.d_world, reg.d_track, reg.d_cloud, reg.d_cloud_id, reg.d_cloud_obs,
                      reg.d_cloud_est, reg.d_cloud_spread, reg.d_summary, ba.d_views_out, ba.d_cloud_out, ba.d_status, ba.d_summary):
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = read()
            for k in plain[which]:
                assert np.asarray(got[k]).tobytes() == np.asarray(plain[which][k]).tobytes(), (which, k)
            keep, counts = U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"])
            assert got["keep"].tobytes() == keep[:len(got["keep"])].tobytes() and got["counts"].tobytes() == counts.tobytes()
            same_registration(got, statement_on(c, keep), f"replay {which}")
    finally:
        ctx.set_stream(None)


# ---- through the pipeline -----------------------------------------------------------------------------------------------------------
def test_pipeline_with_unique_on_the_five_view_scene(ctx, pkg, synth, pipeline):
    """The five-view synthetic scene (keypoints and putative matches, 20 % of the train indices wrong, half a pixel of noise) through
    run_dataset -- the entry point that takes keypoints; the scene has no pixels -- with unique, register and bundle: integers equal to
    the numpy chain on the GPU's own records, doubles under test_gpu_sfm_ba's tolerance rule; unique=False is the dict without."""
    io = importlib.import_module("sfm-gms_amd.io")
    _, _, pairs, matches, _, _, _ = truth_scene(synth, None)
    sc = synth.make_multi_view_scene(7, 5, n_kp=400, noise_px=0.5)
    ds = io.Dataset(sc["frames"], sc["sizes"], None, -1, pairs, matches)
    kw = dict(thresholdFactor=0.5, camera=sc["camera"], match=False, register=True, bundle=True)
    got = pipeline.run_dataset(ctx, ds, unique=True, **kw)
    plain = pipeline.run_dataset(ctx, ds, **kw)
    spelt = pipeline.run_dataset(ctx, ds, unique=False, **kw)
    assert sorted(set(got) - set(plain)) == ["keep", "unique_counts"] and sorted(spelt) == sorted(plain)
    for k in plain:
        assert np.asarray(spelt[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    for k in ("pairs", "matches", "out", "results", "two_view", "coords1", "coords2", "mask", "points3d", "register_plan") + UNTOUCHED:
        assert np.asarray(got[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    frame_off = np.arange(6, dtype=np.int64) * 400
    keep, counts = U.unique(frame_off, got["pairs"], got["out"], got["mask"], got["two_view"])
    assert got["keep"].tobytes() == keep.tobytes() and got["unique_counts"].tobytes() == counts.tobytes()
    want = U.register_keep(frame_off, got["pairs"], got["out"], got["mask"], got["points3d"], got["two_view"], keep=keep)
    same_registration(dict(got, plan=got["register_plan"]), want, "run_dataset")
    xy = np.concatenate([np.stack([fr["x"], fr["y"]], 1) for fr in sc["frames"]]).astype(np.float32)
    want_ba, tol = statement_and_tolerance(got, frame_off, xy, tuple(sc["camera"]) + (0.0,) * 5)
    same_result(got, want_ba, tol, "run_dataset")
    s, s0 = got["ba_summary"][0], plain["ba_summary"][0]
    print("five views, unique: n_multi", plain["summary"]["n_multi"][0], "->", got["summary"]["n_multi"][0], "tracks used", s0["n_tracks_used"], "->",
          s["n_tracks_used"], "rms", s["rms0_px"], "->", s["rms_px"])
    assert got["summary"]["n_multi"][0] == 0 and s["n_tracks_multi"] == 0 and s["n_tracks_used"] >= s0["n_tracks_used"]
    with pytest.raises(ValueError):
        pipeline.run_dataset(ctx, ds, unique=True, thresholdFactor=0.5, camera=sc["camera"], match=False)
    with pytest.raises(ValueError):
        pipeline.run_images(None, np.zeros((2, 64, 64), np.uint8), camera=sc["camera"], unique=True)


def test_four_photographs_with_unique_equal_the_statement_on_the_gpus_own_records(ctx, pkg, pipeline):
    """Views 1, 2, 3, 4 of the reference's scene, the chain (0,1), (1,2), (2,3) with "gms" at 2000 keypoints through run_images with
    unique, register and bundle: keep, counts and the registration against the statement fed the GPU's two-view records, the bundle
    adjustment under the measured tolerance, and no track with two keypoints of a frame."""
    a, b = np.load(os.path.join(GOLDEN, "image_sfm_pair_1008x756.npz")), np.load(os.path.join(GOLDEN, "image_sfm_more_1008x756.npz"))
    images = np.stack([a["left"], b["second"], b["third"], a["right"]])
    kw = dict(method="gms", pairs=[(0, 1), (1, 2), (2, 3)], max_keypoints=2000, withRotation=True, withScale=True, register=True, bundle=True)
    got = pipeline.run_images(ctx, images, tuple(a["camera"]), unique=True, keep_tables=True, **kw)
    frames = got["tables"][0]
    frame_off = frames.frame_off_host
    keep, counts = U.unique(frame_off, got["pairs"], got["out"], got["mask"], got["two_view"])
    assert got["keep"].tobytes() == keep.tobytes() and got["unique_counts"].tobytes() == counts.tobytes()
    want = U.register_keep(frame_off, got["pairs"], got["out"], got["mask"], got["points3d"], got["two_view"], keep=keep)
    same_registration(dict(got, plan=got["register_plan"]), want, "photographs")
    kp = frames.d_kp.cpu().numpy().view(pkg.KEYPOINT_DTYPE)[:int(frame_off[-1])]
    want_ba, tol = statement_and_tolerance(got, frame_off, bcases.xy_of(kp), tuple(a["camera"]) + (0.0,) * 5)
    same_result(got, want_ba, tol, "photographs")
    s = got["ba_summary"][0]
    print("photographs, unique: counts", counts.tolist(), "summary", got["summary"][0].tolist(), "ba", s, "camera 3",
          R.camera_centres(got["views"])[3].tolist(), "->", R.camera_centres(got["views_ba"])[3].tolist())
    assert got["summary"]["n_multi"][0] == 0 and s["n_tracks_multi"] == 0
    multi = pkg.structureFromMotionMulti(images, tuple(a["camera"]), ctx=ctx, max_keypoints=2000, bundle=True, unique=True)
    for k in ("keep", "unique_counts", "track", "summary", "views_ba", "cloud_ba", "track_status", "ba_summary"):
        assert np.asarray(multi[k]).tobytes() == np.asarray(got[k]).tobytes(), k


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(ctx, pkg, batch):
    """GMS_ERR_BAD_ARG and nothing run: the outputs keep their fill."""
    c = ucases.case("star")
    job = unique_job(ctx, batch, c)
    job.d_counts.fill_(FILL)
    torch.cuda.synchronize()
    d_m, d_mask, d_tv = job._own
    good = [job.d_frame_off.data_ptr(), job.n_frames, job.total_kp, job.d_pairs.data_ptr(), job.n_pairs, job.max_m, job.total_m, d_m.data_ptr(),
            d_mask.data_ptr(), d_tv.data_ptr(), job.d_ws.data_ptr(), job.ws_bytes, job.d_keep.data_ptr(), job.d_counts.data_ptr()]
    bad = {"workspace one byte short": (11, job.ws_bytes - 1), "workspace off its alignment": (10, job.d_ws.data_ptr() + 16), "no frames": (1, 0),
           "negative pairs": (4, -1), "negative max_m": (5, -1), "max_m 2^24": (5, 1 << 24), "negative matches": (6, -1),
           "too many keypoints": (2, 2 ** 31 - 1)}
    for i in (0, 3, 7, 10, 12, 13):
        bad[f"null pointer {i}"] = (i, None)
    lib = pkg.load_library()
    for what, (i, v) in bad.items():
        args = list(good)
        args[i] = v
        assert lib.gms_match_unique_device(ctx._h, *args) == -1, what
    assert lib.gms_match_unique_device(None, *good) == -1
    with pytest.raises(pkg.GmsError):
        ctx.match_unique_device(*(good[:11] + [0] + good[12:]))
    ctx.synchronize()
    assert bool((job.d_keep == FILL).all()) and bool((job.d_counts == FILL).all())
    # the keep-plane registration refuses what the registration refuses
    r = rcases.case("lowest_k_wins")
    reg = batch.SfmRegister(ctx, r["frame_off"], r["pairs"], r["root"], r["min_links"], keep=True)
    reg.load(r["matches"], r["mask"], r["points3d"], r["tv"], np.ones(len(r["mask"]), np.uint8))
    rm, rmask, rpts, rtv = reg._own_inputs()
    outs = (reg.d_views, reg.d_reg, reg.d_world, reg.d_track, reg.d_cloud, reg.d_cloud_id, reg.d_cloud_obs, reg.d_cloud_est, reg.d_cloud_spread,
            reg.d_summary)
    rgood = [reg.d_frame_off.data_ptr(), reg.n_frames, reg.total_kp, reg.d_pairs.data_ptr(), reg.d_plan.data_ptr(), reg.n_pairs, reg.max_m,
             reg.total_m, rm.data_ptr(), rmask.data_ptr(), rpts.data_ptr(), rtv.data_ptr(), reg.root, reg.min_links, reg.d_ws.data_ptr(),
             reg.ws_bytes] + [t.data_ptr() for t in outs[:4]] + [reg.cloud_cap] + [t.data_ptr() for t in outs[4:]] + [reg.d_keep.data_ptr()]
    for i, v in ((12, -1), (13, 0), (15, reg.ws_bytes - 1), (14, reg.d_ws.data_ptr() + 16), (0, None), (16, None), (26, None)):
        args = list(rgood)
        args[i] = v
        assert lib.gms_sfm_register_keep_device(ctx._h, *args) == -1, i
    # and the unchanged arguments run, null mask and two-view records included
    assert lib.gms_match_unique_device(ctx._h, *good) == 0
    ctx.synchronize()
    assert job.results()[1].tolist() == [[80, 40]] * 3
    args = list(good)
    args[8] = args[9] = None
    assert lib.gms_match_unique_device(ctx._h, *args) == 0
    ctx.synchronize()
    assert job.results()[1].tolist() == [[80, 40]] * 3
    assert lib.gms_sfm_register_keep_device(ctx._h, *rgood) == 0
    ctx.synchronize()
    assert int(reg.results()["summary"]["n_ok_pairs"][0]) == 2
