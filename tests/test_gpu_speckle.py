"""GPU: gms_filter_speckles_device, gms_filter_speckles, the dense stage's speckle option and their Python faces against the `literal`
statement of tests/speckle_ref.py, byte for byte: every case of tests/speckle_cases.py, the matcher's map of the
committed 450 x 375 pair, a batch of three maps, the one-shot on host arrays and device tensors, repeated runs, one graph capture
replayed on a new map, DensePairs(speckle=) on the rendered plane against the numpy chain, the fusion over filtered runs, and the
refused arguments."""
import importlib

import numpy as np
import pytest

import dense_fuse_cases as fc
import dense_fuse_ref as fr
import rectify_cases as rc
import rectify_ref as rr
import speckle_cases as sc
import speckle_ref as sr
import stereo_bm_ref
import stereo_sgm_cases

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in sc.all_cases()}


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def types():
    return importlib.import_module("sfm-gms_amd.types")


def _filter(ctx, batch, torch, maps, new_val, size, diff):
    """gms_filter_speckles_device on n maps over a workspace and a count that hold a fill pattern -> (maps, removed) on the host."""
    job = batch.SpeckleFilter(ctx, len(maps), (maps.shape[2], maps.shape[1]))
    job.d_ws.fill_(0xA5)
    job.d_removed.fill_(-7)
    d = torch.from_numpy(np.array(maps, dtype=np.int16, order="C")).cuda()     # (a copy: the cases are read-only)
    torch.cuda.synchronize()
    assert job.run(d, new_val, size, diff) is d
    ctx.synchronize()
    return d.cpu().numpy(), job.d_removed.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_literal_statement(ctx, batch, name):
    import torch
    case = CASES[name]
    for k, (size, diff, stated) in enumerate(case["runs"]):
        want, n_want = sc.expected(name, k)
        got, removed = _filter(ctx, batch, torch, case["disp"][None], case["new_val"], size, diff)
        assert removed.tolist() == [n_want] and (stated is None or n_want == stated), (name, k, removed, n_want)
        assert got[0].tobytes() == want.tobytes(), (name, k, int((got[0] != want).sum()))


def test_the_matchers_map_of_the_committed_pair(pkg):
    """sgm_map: the 450 x 375 pair through the stereoSGM under test with the reference's parameters (min_disparity -39, so FILTERED is
    -640), then (100, 32) with new_val = FILTERED."""
    left, right, _ = stereo_sgm_cases.golden_pair()
    filtered = stereo_bm_ref.filtered_value(stereo_bm_ref.make_params())
    assert filtered == -640
    disp = pkg.stereoSGM(left, right)
    assert disp.shape == (375, 450) and disp.dtype == np.int16 and (disp == filtered).any()
    want, n_want = sr.literal(disp, filtered, 100, 32)
    got, removed = pkg.filterSpeckles(disp, filtered, 100, 32, return_removed=True)
    print(f"sgm_map: {int((disp != filtered).sum())} valued pixels, {n_want} removed by (100, 32)")
    assert removed == n_want and 0 < n_want < int((disp != filtered).sum()) and got.tobytes() == want.tobytes()
    assert got is not disp and (disp != got).sum() == n_want       # a host array gives a new host array


def test_batch_of_three_different_maps(ctx, batch):
    import torch
    maps = np.stack([sc.random_map(70 + i, 131, 67) for i in range(3)])
    maps[1, :, :] = sc.plus_on_lattice()["disp"]
    want = [sr.literal(m, sc.NV, 13, 16) for m in maps]
    got, removed = _filter(ctx, batch, torch, maps, sc.NV, 13, 16)
    assert removed.tolist() == [w[1] for w in want] and removed[1] == 13 * 21 and len(set(removed.tolist())) == 3
    for i in range(3):
        assert got[i].tobytes() == want[i][0].tobytes(), i
    again = batch.filter_speckles_batch(maps, sc.NV, 13, 16, ctx=ctx, return_removed=True)      # host arrays in, new host arrays out
    assert again[0].tobytes() == got.tobytes() and again[1].tolist() == removed.tolist()


def test_one_shot_on_host_arrays_and_on_a_device_tensor(pkg):
    import torch
    disp = sc.random_map(5, 259, 131)
    want, n_want = sr.literal(disp, sc.NV, 20, 16)
    host, n_host = pkg.filterSpeckles(disp, sc.NV, 20, 16, return_removed=True)
    d = torch.from_numpy(disp.copy()).cuda()
    dev, n_dev = pkg.filterSpeckles(d, sc.NV, 20, 16, return_removed=True)
    assert dev is d and n_host == n_dev == n_want                    # a device tensor is filtered in place and returned
    assert host.tobytes() == want.tobytes() == dev.cpu().numpy().tobytes()
    assert pkg.filterSpeckles(disp, sc.NV, 20, 16).tobytes() == want.tobytes()
    unchanged, n0 = pkg.filterSpeckles(disp, sc.NV, 0, 16, return_removed=True)     # max_speckle_size 0: the map comes back unchanged
    assert n0 == 0 and unchanged.tobytes() == disp.tobytes()


def test_two_runs_give_equal_bytes(ctx, batch):
    import torch
    maps = np.stack([sc.random_map(90 + i, 259, 131) for i in range(2)])
    first = _filter(ctx, batch, torch, maps, sc.NV, 200, 0)
    second = _filter(ctx, batch, torch, maps, sc.NV, 200, 0)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tolist() == second[1].tolist() and first[1].min() > 0


def test_captured_graph_follows_a_new_map(ctx, batch):
    import torch
    old, new = sc.random_map(31, 131, 67), sc.random_map(32, 131, 67)
    job = batch.SpeckleFilter(ctx, 1, (131, 67))
    d = torch.from_numpy(old.copy()[None]).cuda()
    torch.cuda.synchronize()
    job.run(d, sc.NV, 20, 16)                                      # (first use outside the capture)
    ctx.synchronize()
    assert d[0].cpu().numpy().tobytes() == sr.literal(old, sc.NV, 20, 16)[0].tobytes()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):                   # one stream, no parallel branches
            job.run(d, sc.NV, 20, 16)
        d.copy_(torch.from_numpy(new[None]))
        job.d_removed.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want, n_want = sr.literal(new, sc.NV, 20, 16)
        assert d[0].cpu().numpy().tobytes() == want.tobytes() and job.d_removed.tolist() == [n_want] and n_want > 0
    finally:
        ctx.set_stream(None)


def _scene_stack(torch, n):
    img1, img2 = rc.scene()
    return torch.from_numpy(np.stack([img1] * n)).cuda(), torch.from_numpy(np.stack([img2] * n)).cuda()


def _bytes(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def _scene_run(ctx, batch, types, torch, speckle, registered=False):
    """The rendered plane as two pairs of one DensePairs run (the second pair the first again); with a registration, frames 0 and 1."""
    d1, d2 = _scene_stack(torch, 2)
    run = batch.DensePairs(ctx, 2, rc.SCENE_SIZE, rc.SCENE_SIZE, rc.SCENE_CAMERA, None, 1, params=rc.SCENE_SGM, speckle=speckle)
    tv = np.zeros(2, types.TWO_VIEW_DTYPE)
    for i in range(2):
        tv["R"][i], tv["t"][i], tv["status"][i] = rc.SCENE_R, rc.SCENE_T, 0
    run.set_two_view(tv)
    keep = None
    if registered:
        pairs = np.zeros(2, types.PAIR_DTYPE)
        pairs["frame_a"], pairs["frame_b"] = [0, 1], [1, 2]
        regs = np.zeros(2, types.SFM_PAIR_REG_DTYPE)
        regs["S"], regs["status"] = 1.0, 0
        views = np.zeros(3, types.SFM_VIEW_DTYPE)
        R3, t3 = rc.SCENE_R @ rc.SCENE_R, rc.SCENE_R @ rc.SCENE_T + rc.SCENE_T
        for i, (R, t, ok) in enumerate((fc.SCENE_VIEWS[0], fc.SCENE_VIEWS[1], (R3.reshape(9), t3, 1))):
            views["R"][i], views["t"][i], views["registered"][i], views["pair"][i] = np.asarray(R).reshape(3, 3), t, ok, -1
        keep = [_bytes(torch, pairs), _bytes(torch, regs), _bytes(torch, views)]
        run.set_registration(keep[0], keep[1], keep[2], 3)
    torch.cuda.synchronize()
    run.run(d1, d2)
    ctx.synchronize()
    return run


@pytest.fixture(scope="module")
def scene_chain():
    return rc.scene_chain()


def test_dense_pairs_with_the_speckle_option(ctx, pkg, batch, types, scene_chain):
    import torch
    P, r1, r2, v1, disp, (xyz, colors, pixel) = scene_chain
    plain = _scene_run(ctx, batch, types, torch, None)
    # speckle=None equals the parent's bytes: the numpy chain that the parent's test pins
    assert plain.d_removed is None and np.array_equal(plain.d_disp16[0].cpu().numpy(), disp)
    k = int(plain.d_count[0])
    assert k == len(xyz) and plain.d_xyz[0, :k].cpu().numpy().tobytes() == xyz.tobytes()
    for speckle in ((100, 32), (100, 1)):
        run = _scene_run(ctx, batch, types, torch, speckle)
        want, n_want = sr.literal(disp, -16, *speckle)
        removed = run.d_removed.cpu().numpy()
        print(f"scene: speckle {speckle} removes {n_want} of {int((disp != -16).sum())} valued pixels; points {len(xyz)} -> {int(run.d_count[0])}")
        for j in range(2):
            got = run.d_disp16[j].cpu().numpy()
            assert got.tobytes() == want.tobytes() and removed[j] == n_want
            assert got.tobytes() == pkg.filterSpeckles(plain.d_disp16[j].cpu().numpy(), -16, *speckle).tobytes()
            wx, wc, wp = rr.cloud(want, v1, r1, P, -16, 16)          # the numpy chain on the filtered map
            k = int(run.d_count[j])
            assert k == len(wx) and run.d_xyz[j, :k].cpu().numpy().tobytes() == wx.tobytes()
            assert np.array_equal(run.d_pixel[j, :k].cpu().numpy(), wp) and np.array_equal(run.d_cloud_color[j, :k, 0].cpu().numpy(), wc)
        assert np.array_equal(run.d_rect1.cpu().numpy(), plain.d_rect1.cpu().numpy()) and np.array_equal(run.d_valid.cpu().numpy(), plain.d_valid.cpu().numpy())
    assert sr.literal(disp, -16, 100, 1)[1] == 199 and sr.literal(disp, -16, 100, 32)[1] == 1     # both settings change this map


def test_dense_stereo_one_shot_with_the_speckle_option(pkg, scene_chain):
    import torch
    P, r1, _, v1, disp, (xyz, _, _) = scene_chain
    img1, img2 = rc.scene()
    plain = pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, **rc.SCENE_SGM)
    assert "removed" not in plain and np.array_equal(plain["disp16"], disp) and plain["points"].tobytes() == xyz.tobytes()
    want, n_want = sr.literal(disp, -16, 100, 1)
    wx = rr.cloud(want, v1, r1, P, -16, 16)[0]
    host = pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, speckle=(100, 1), **rc.SCENE_SGM)
    dev = pkg.denseStereo(torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda(), rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T,
                          speckle=(100, 1), **rc.SCENE_SGM)
    assert host["removed"] == dev["removed"] == n_want and host["count"] == dev["count"] == len(wx)
    assert host["disp16"].tobytes() == want.tobytes() == dev["disp16"].cpu().numpy().tobytes()
    assert host["points"].tobytes() == wx.tobytes() == dev["points"].cpu().numpy().tobytes()
    with pytest.raises(pkg.GmsError):
        pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, speckle=(-1, 0), **rc.SCENE_SGM)


def test_fusion_over_filtered_runs_reads_the_filtered_maps(ctx, batch, types):
    import torch
    run = _scene_run(ctx, batch, types, torch, (100, 1), registered=True)
    plans, counts = run.plans(), run.d_count.cpu().numpy()
    srcs = [fr.source(run.d_disp16[j].cpu().numpy(), run.d_valid[j].cpu().numpy(), plans[j:j + 1], run.d_xyz[j].cpu().numpy(), count=int(counts[j]),
                      color=run.d_cloud_color[j].cpu().numpy(), filtered16=-16, min_disp16=16, view=fc.SCENE_VIEWS[j], reg=(1.0, 0)) for j in range(2)]
    assert int(run.d_removed[0]) > 0
    want = fr.fuse(srcs)
    got = batch.fuse_dense(ctx, [run])
    assert np.array_equal(got["counts"], want["counts"]) and want["counts"][-1] > 1000
    for key in ("points", "source", "index", "support", "conflict"):
        assert np.ascontiguousarray(got[key]).tobytes() == np.ascontiguousarray(want[key]).tobytes(), key


def test_bad_arguments_are_refused_before_any_launch(ctx, pkg, batch):
    import torch
    disp = sc.random_map(3, 131, 67)
    d = torch.from_numpy(disp.copy()[None]).cuda()
    job = batch.SpeckleFilter(ctx, 1, (131, 67))
    job.d_removed.fill_(-7)
    torch.cuda.synchronize()
    ws, nb, p = job.d_ws.data_ptr(), job.ws_bytes, d.data_ptr()
    good = dict(d_disp16=p, n=1, width=131, height=67, new_val=sc.NV, max_speckle_size=20, max_diff=16, d_ws=ws, ws_bytes=nb,
                d_removed=job.d_removed.data_ptr())
    bad = [dict(width=0), dict(height=0), dict(width=8193), dict(n=0), dict(n=65536), dict(new_val=32768), dict(new_val=-32769),
           dict(max_speckle_size=-1), dict(max_diff=-1), dict(max_diff=2 ** 31), dict(d_disp16=None), dict(d_ws=None), dict(d_ws=ws + 128),
           dict(ws_bytes=nb - 1), dict(d_disp16=p + 1), dict(d_removed=job.d_removed.data_ptr() + 2)]
    for kw in bad:
        with pytest.raises(pkg.GmsError) as e:
            ctx.filter_speckles_device(**dict(good, **kw))
        assert e.value.code == -1, kw
    ctx.synchronize()
    assert d[0].cpu().numpy().tobytes() == disp.tobytes() and job.d_removed.tolist() == [-7]      # nothing ran
    for kw in (dict(n=0, size=(131, 67)), dict(n=1, size=(8193, 67)), dict(n=65536, size=(4, 4))):
        with pytest.raises(pkg.GmsError):
            batch.SpeckleFilter(ctx, **kw)
    with pytest.raises(ValueError):
        job.run(d[0], sc.NV, 20, 16)                                # the wrong shape
    with pytest.raises(ValueError):
        job.run(d.to(torch.int32), sc.NV, 20, 16)
    with pytest.raises(pkg.GmsError):
        batch.DensePairs(ctx, 1, rc.SCENE_SIZE, rc.SCENE_SIZE, rc.SCENE_CAMERA, None, 1, params=rc.SCENE_SGM, speckle=(5, -1))
    ctx.filter_speckles_device(**good)                              # and the good call runs
    ctx.synchronize()
    assert d[0].cpu().numpy().tobytes() == sr.literal(disp, sc.NV, 20, 16)[0].tobytes()
