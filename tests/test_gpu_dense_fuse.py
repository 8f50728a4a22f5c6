"""GPU: gms_dense_fuse_device, gms_dense_fuse and their Python faces against tests/dense_fuse_ref.py, byte for byte:
the hand-made cases of tests/dense_fuse_cases.py through the device call and the one-shot, the rendered plane in three cameras from
pixels to the fused cloud, sources past the 256 blocks of one scan pass, 32 neighbours, one graph capture replayed on new maps and a
new view, repeated runs, the pipeline's keywords and the refused arguments."""
import importlib
import os

import numpy as np
import pytest

import dense_fuse_cases as fc
import dense_fuse_ref as fr
import rectify_cases as rc

pytestmark = pytest.mark.gpu
KEYS = ("points", "colors", "source", "index", "support", "conflict")
FILL = dict(points=-7.0, colors=0xA5, source=-7, index=-7, support=0xA5, conflict=0xA5)


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def types():
    return importlib.import_module("sfm-gms_amd.types")


@pytest.fixture(scope="module")
def cases():
    return fc.hand_cases()


def _bytes(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def _view_rec(types, view):
    G = np.zeros(1, types.SFM_VIEW_DTYPE)
    G["R"][0], G["t"][0], G["registered"], G["pair"] = np.asarray(view[0]).reshape(3, 3), view[1], view[2], -1
    return G


def _reg_rec(types, reg):
    r = np.zeros(1, types.SFM_PAIR_REG_DTYPE)
    r["S"], r["status"] = reg
    return r


def _device_source(torch, types, s, channels):
    """A dense_fuse_ref source -> the dict of device tensors batch.DenseFuse takes (a source without points still gets one row)."""
    cap = len(s["xyz"])
    xyz = np.zeros((max(cap, 1), 3), np.float32)
    xyz[:cap] = s["xyz"]
    d = dict(d_disp16=torch.from_numpy(s["disp16"].copy()).cuda(), d_valid=torch.from_numpy(s["valid"].copy()).cuda(), d_plan=_bytes(torch, s["plan"]),
             d_xyz=torch.from_numpy(xyz).cuda(), d_count=torch.tensor([s["count"]], dtype=torch.int32, device="cuda"), cap=cap,
             filtered16=s["filtered16"], min_disp16=s["min_disp16"])
    if s["color"] is not None:
        col = np.zeros((max(cap, 1), channels), np.uint8)
        col[:cap] = s["color"].reshape(cap, channels)
        d["d_color"] = torch.from_numpy(col).cuda()
    if s["view"] is not None:
        d["d_view"] = _bytes(torch, _view_rec(types, s["view"]))
    if s["reg"] is not None:
        d["d_reg"] = _bytes(torch, _reg_rec(types, s["reg"]))
    return d


def _fill(job):
    job.d_xyz.fill_(FILL["points"])
    job.d_source.fill_(FILL["source"])
    job.d_index.fill_(FILL["index"])
    for t in (job.d_color, job.d_support, job.d_conflict):
        t.fill_(0xA5)
    job.d_counts.fill_(-7)
    job.d_ws.fill_(0xA5)


def _raw(job):
    """Every output in full, past the count too."""
    job.ctx.synchronize()
    return dict(points=job.d_xyz.cpu().numpy(), colors=job.d_color.cpu().numpy(), source=job.d_source.cpu().numpy(), index=job.d_index.cpu().numpy(),
                support=job.d_support.cpu().numpy(), conflict=job.d_conflict.cpu().numpy(), counts=job.d_counts.cpu().numpy())


def _assert_equal(got, want, name, fused_cap=None):
    """got: _raw's arrays; want: the statement's. Bytes up to min(total, cap); the fill behind."""
    assert np.array_equal(got["counts"], want["counts"]), (name, got["counts"], want["counts"])
    k = len(want["points"])
    assert k == (int(want["counts"][-1]) if fused_cap is None else min(int(want["counts"][-1]), fused_cap))
    for key in KEYS:
        w = np.ascontiguousarray(want[key])
        assert got[key][:k].tobytes() == w.tobytes(), (name, key)
        assert (got[key][k:] == FILL[key]).all(), (name, key, "written past the end")


def _run_case(ctx, batch, types, torch, case):
    srcs = [_device_source(torch, types, s, case["channels"]) for s in case["sources"]]
    cap = sum(len(s["xyz"]) for s in case["sources"]) if case["fused_cap"] is None else case["fused_cap"]
    job = batch.DenseFuse(ctx, srcs, case["neighbors"], case["channels"], case["tol16"], case["min_support"], cap)
    _fill(job)
    torch.cuda.synchronize()
    job.run()
    return job


def _statement(case):
    return fr.fuse(case["sources"], case["neighbors"], case["channels"], case["tol16"], case["min_support"], case["fused_cap"])


def test_hand_made_cases_through_the_device_call(ctx, batch, types, cases):
    import torch
    for case in cases:
        want = _statement(case)
        job = _run_case(ctx, batch, types, torch, case)
        _assert_equal(_raw(job), want, case["name"], case["fused_cap"])
        res = job.result()
        assert res["points"].tobytes() == want["points"].tobytes() and len(res["source"]) == len(want["source"])


def _host_source(s, channels):
    d = dict(disp16=s["disp16"], valid=s["valid"], plan=np.asarray(s["plan"]), points=s["xyz"], count=s["count"], filtered16=s["filtered16"],
             min_disp16=s["min_disp16"])
    if s["color"] is not None:
        d["colors"] = s["color"].reshape(len(s["xyz"]), channels)
    if s["view"] is not None:
        d["view"] = s["view"]
    if s["reg"] is not None:
        d["reg"] = s["reg"]
    return d


def test_hand_made_cases_through_the_one_shot(pkg, cases):
    for case in cases:
        want = _statement(case)
        c = case["channels"]
        got = pkg.denseFuse([_host_source(s, c) for s in case["sources"]], case["neighbors"], case["tol16"], case["min_support"], case["fused_cap"])
        assert np.array_equal(got["counts"], want["counts"]), case["name"]
        for key in KEYS:
            w = want[key] if key != "colors" or c == 3 else want[key][:, 0]
            assert got[key].tobytes() == np.ascontiguousarray(w).tobytes(), (case["name"], key)


def _scene_run(ctx, batch, types, torch):
    """DensePairs on the three rendered images as the pairs (0, 1) and (1, 2), with hand-made two-view, registration and view records."""
    imgs = fc.scene3()
    d1 = torch.from_numpy(np.stack([imgs[0], imgs[1]])).cuda()
    d2 = torch.from_numpy(np.stack([imgs[1], imgs[2]])).cuda()
    run = batch.DensePairs(ctx, 2, rc.SCENE_SIZE, rc.SCENE_SIZE, rc.SCENE_CAMERA, None, 1, params=rc.SCENE_SGM)
    tv = np.zeros(2, types.TWO_VIEW_DTYPE)
    for i in range(2):
        tv["R"][i], tv["t"][i], tv["status"][i] = rc.SCENE_R, rc.SCENE_T, 0
    run.set_two_view(tv)
    pairs = np.zeros(2, types.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [0, 1], [1, 2]
    regs = np.concatenate([_reg_rec(types, (1.0, 0))] * 2)
    R3, t3 = rc.SCENE_R @ rc.SCENE_R, rc.SCENE_R @ rc.SCENE_T + rc.SCENE_T
    views = np.concatenate([_view_rec(types, fc.SCENE_VIEWS[0]), _view_rec(types, fc.SCENE_VIEWS[1]), _view_rec(types, (R3.reshape(9), t3, 1))])
    keep = [_bytes(torch, pairs), _bytes(torch, regs), _bytes(torch, views)]
    run.set_registration(keep[0], keep[1], keep[2], 3)
    torch.cuda.synchronize()
    run.run(d1, d2)
    ctx.synchronize()
    return run


def _sources_of_run(run):
    """The statement's sources from the GPU's own maps, plans, points and counts."""
    plans, counts = run.plans(), run.d_count.cpu().numpy()
    f16 = (rc.SCENE_SGM["min_disparity"] - 1) * 16
    return [fr.source(run.d_disp16[j].cpu().numpy(), run.d_valid[j].cpu().numpy(), plans[j:j + 1], run.d_xyz[j].cpu().numpy(), count=int(counts[j]),
                      color=run.d_cloud_color[j].cpu().numpy(), filtered16=f16, min_disp16=16, view=fc.SCENE_VIEWS[j], reg=(1.0, 0)) for j in range(2)]


def test_scene_from_pixels_to_the_fused_cloud(ctx, batch, types):
    import torch
    run = _scene_run(ctx, batch, types, torch)
    job = batch.DenseFuse(ctx, [run])
    _fill(job)
    torch.cuda.synchronize()
    job.run()
    got = _raw(job)
    srcs = _sources_of_run(run)
    want = fr.fuse(srcs)
    _assert_equal(got, want, "scene")
    a, b, c, d = fc.scene_figures(srcs, want)
    print(f"scene on the GPU's maps: (a) {a:.4f} (b) {b:.4f} (c) {c:.4f} (d) {d}; counts {want['counts'].tolist()}")
    assert want["counts"][-1] > 4000 and (want["support"] == 2).sum() > 3000
    # the same through fuse_dense, which builds, runs and reads back
    again = batch.fuse_dense(ctx, [run])
    assert all(np.ascontiguousarray(again[k]).tobytes() == np.ascontiguousarray(want[k] if k != "colors" else want[k][:, 0]).tobytes() for k in KEYS)


def _big_sources():
    """Three sources: 512 x 520 maps with every pixel a point (266 240 points, 260 blocks of 1024 each), the first with a count that is
    no multiple of 1024, an empty source between them; the third map differs from the first by 0, 10, 16, 17 or 40 sixteenths."""
    w, h = 512, 520
    rng = np.random.default_rng(5)
    P = fc.hand_plan(w, h, fx=400.0, cx=256.0, cy=260.0)
    d0 = rng.integers(64, 600, (h, w)).astype(np.int16)
    d2 = (d0 + rng.choice(np.array([0, 10, -16, 17, -40], np.int16), (h, w))).astype(np.int16)
    a = fc.map_source(d0, plan=P, color_seed=50)
    a["count"] = w * h - 555
    z = fc.map_source(fc.empty_map()[0])
    z["count"] = 0
    b = fc.map_source(d2, plan=P, color_seed=51)
    assert len(a["xyz"]) == len(b["xyz"]) == 266240 and len(z["xyz"]) == 0
    return [a, z, b]


def test_past_one_scan_pass(ctx, batch, types):
    import torch
    srcs = _big_sources()
    full = fr.fuse(srcs)                                           # the statement once; a cap only cuts it
    total = full["counts"]
    assert total[0] == 266240 - 555 and total[1] == 0 and 50000 < total[2] < 200000
    inside_block_258_of_source_0 = 257 * 1024 + 333
    for cap in (int(total[-1]) + 5, inside_block_258_of_source_0, int(total[0]) + 1024 * 3 + 1):
        case = fc._case("big", srcs, fused_cap=cap)
        want = dict({k: full[k][:cap] for k in KEYS}, counts=total)
        job = _run_case(ctx, batch, types, torch, case)
        first = _raw(job)
        _assert_equal(first, want, f"big cap {cap}", cap)
        job.run()                                                  # two runs give equal bytes
        second = _raw(job)
        assert all(first[k].tobytes() == second[k].tobytes() for k in first)


def test_32_neighbours_of_33_sources(ctx, batch, types):
    import torch
    srcs = []
    for i in range(33):
        m = fc.empty_map()[0]
        m[2:5, 3:7] = 64                       # seen by all 33
        m[9 + i // 20, i % 20] = 32            # seen by source i alone
        srcs.append(fc.map_source(m, color_seed=60 + i))
    case = fc._case("33", srcs)
    assert case["neighbors"].shape == (33, 32)
    want = _statement(case)
    assert want["counts"].tolist() == [13] + [1] * 32 + [45] and want["support"][:12].tolist() == [33] * 12
    _assert_equal(_raw(_run_case(ctx, batch, types, torch, case)), want, "33")
    with pytest.raises(ValueError):
        batch.DenseFuse(ctx, [_device_source(torch, types, s, 1) for s in srcs + srcs[:1]])   # 34 sources need neighbors=


def _replay_sources(seed, view):
    rng = np.random.default_rng(seed)
    m = rng.integers(48, 200, (fc.H, fc.W)).astype(np.int16)
    m[rng.integers(0, 4, m.shape) == 0] = fc.F16
    m2 = m.copy()
    m2[rng.integers(0, 3, m.shape) == 0] += 40
    return [fc.map_source(m, color_seed=seed, view=view, reg=(1.25, 0)), fc.map_source(m2, color_seed=seed + 1, view=view, reg=(1.25, 0))]


def test_captured_graph_follows_new_maps_and_a_new_view(ctx, batch, types):
    import torch
    view_a = (rc.rot((0, 1, 0), 4.0).reshape(9), np.array([0.1, 0.0, -0.2]), 1)
    view_b = (rc.rot((1, 0.5, 0), -7.0).reshape(9), np.array([-0.4, 0.3, 0.6]), 1)
    old, new = _replay_sources(70, view_a), _replay_sources(80, view_b)
    cap = fc.W * fc.H

    def padded(s):                                                 # the tensors keep one size while the data changes
        xyz, col = np.zeros((cap, 3), np.float32), np.zeros((cap, 1), np.uint8)
        xyz[:len(s["xyz"])], col[:len(s["xyz"])] = s["xyz"], s["color"]
        return dict(s, xyz=xyz, color=col)

    old, new = [padded(s) for s in old], [padded(s) for s in new]
    case_old, case_new = fc._case("old", old), fc._case("new", new)
    assert not np.array_equal(_statement(case_old)["counts"], _statement(case_new)["counts"])
    job = _run_case(ctx, batch, types, torch, case_old)            # (first use outside the capture)
    _assert_equal(_raw(job), _statement(case_old), "old", 2 * cap)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):                   # one stream, no parallel branches
            job.run()
        for d, s in zip(job.sources, new):                         # new maps, points, counts and view, in the tensors the table points to
            d["d_disp16"].copy_(torch.from_numpy(s["disp16"]))
            d["d_valid"].copy_(torch.from_numpy(s["valid"]))
            d["d_xyz"].copy_(torch.from_numpy(s["xyz"]))
            d["d_color"].copy_(torch.from_numpy(s["color"]))
            d["d_count"].fill_(s["count"])
            d["d_view"].copy_(torch.from_numpy(_view_rec(types, s["view"]).view(np.uint8).reshape(-1)))
        _fill(job)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(_raw(job), _statement(case_new), "new", 2 * cap)
    finally:
        ctx.set_stream(None)


def test_pipeline_keywords(ctx, pkg):
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "image_sfm_pair_1008x756.npz"))
    imgs = [np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])]
    cam = tuple(float(v) for v in z["camera"])
    kw = dict(method="gms", max_keypoints=4000, register=True, dense=True, dense_cap=200000)
    base = pipeline.run_images(ctx, imgs, cam, None, **kw)
    off = pipeline.run_images(ctx, imgs, cam, None, fuse=False, **kw)
    assert "dense_fused" not in base and sorted(base) == sorted(off)

    def same(a, b):
        if isinstance(a, dict):
            return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, np.ndarray):
            return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        return a is b or a == b

    assert all(same(base[k], off[k]) for k in base)
    on = pipeline.run_images(ctx, imgs, cam, None, fuse=True, **kw)
    assert all(same(base[k], on[k]) for k in base)                 # `dense` itself is unchanged
    f, d = on["dense_fused"], on["dense"][0]
    assert sorted(f) == ["colors", "conflict", "counts", "index", "points", "source", "support"]
    if d is None:                                                  # the recovered pose is outside what the plan rectifies: nothing to fuse
        assert f["counts"].tolist() == [0, 0] and len(f["points"]) == 0
        return
    k = len(d["points"])                                           # one pair: every point is kept, seen by its own pair alone
    print(f"pipeline: {k} dense points of the pair, fused counts {f['counts'].tolist()}")
    assert f["counts"].tolist() == [k, k] and f["points"].tobytes() == d["points"].tobytes() and np.array_equal(f["colors"], d["colors"])
    assert (f["source"] == 0).all() and np.array_equal(f["index"], np.arange(k)) and (f["support"] == 1).all() and not f["conflict"].any()


def test_value_errors_and_refused_arguments(ctx, pkg, batch, types, cases):
    import torch
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    img = np.zeros((2, 64, 64), np.uint8)
    for kw in (dict(dense=True), dict(register=True), dict()):
        with pytest.raises(ValueError):
            pipeline.run_images(ctx, img, (50.0, 50.0, 32.0, 32.0), None, fuse=True, **kw)
    with pytest.raises(ValueError):
        pkg.structureFromMotionMulti(img, (50.0, 50.0, 32.0, 32.0), fuse=True)
    with pytest.raises(ValueError):
        types.dense_fuse_neighbors(34)
    with pytest.raises(ValueError):
        types.dense_fuse_neighbors(3, np.zeros((3, 33), np.int32))
    case = cases[2]
    srcs = [_device_source(torch, types, s, 1) for s in case["sources"]]
    job = batch.DenseFuse(ctx, srcs)
    good = dict(d_src=job.d_src.data_ptr(), n_src=job.n, max_cap=job.max_cap, d_neighbors=job.d_neighbors.data_ptr(), n_nb=job.n_nb, channels=1, tol16=16,
                min_support=1, d_ws=job.d_ws.data_ptr(), ws_bytes=job.ws_bytes, fused_cap=job.fused_cap, d_xyz=job.d_xyz.data_ptr(),
                d_color=job.d_color.data_ptr(), d_source=job.d_source.data_ptr(), d_index=job.d_index.data_ptr(), d_support=job.d_support.data_ptr(),
                d_conflict=job.d_conflict.data_ptr(), d_counts=job.d_counts.data_ptr())
    _fill(job)
    torch.cuda.synchronize()
    for bad in (dict(n_nb=0), dict(n_nb=33), dict(channels=2), dict(channels=0), dict(min_support=0), dict(tol16=-1), dict(max_cap=0),
                dict(max_cap=8192 * 8192 + 1), dict(n_src=0), dict(n_src=65536), dict(fused_cap=-1), dict(d_ws=job.d_ws.data_ptr() + 64),
                dict(ws_bytes=job.ws_bytes - 1), dict(d_src=0), dict(d_neighbors=0), dict(d_counts=0), dict(d_xyz=0)):
        with pytest.raises(types.GmsError) as e:
            ctx.dense_fuse_device(**dict(good, **bad))
        assert e.value.code == -1, bad
    ctx.synchronize()
    assert (job.d_counts.cpu().numpy() == -7).all() and (job.d_ws.cpu().numpy() == 0xA5).all()   # refused before any launch
    assert ctx.dense_fuse_workspace_bytes(0, 10) == 0 and ctx.dense_fuse_workspace_bytes(3, 0) == 0 and ctx.dense_fuse_workspace_bytes(65535, 65536) == 0
    for kw in (dict(min_support=0), dict(tol16=-1), dict(fused_cap=-1)):
        with pytest.raises(types.GmsError):
            pkg.denseFuse([_host_source(s, 1) for s in case["sources"]], **kw)
    ctx.dense_fuse_device(**good)                                  # and the same arguments unchanged are accepted
    _assert_equal(_raw(job), _statement(case), "accepted")
