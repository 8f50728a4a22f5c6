"""GPU: gms_dense_cloud_device, gms_dense_pairs_device and their Python faces against tests/rectify_ref.py, byte for byte (DESIGN.md
§4.13): the cloud kernels on hand-made int16 planes (no matcher involved; also past the 256 blocks of one scan pass), the whole stage on a rendered plane against the numpy
chain, a failed pair inside a batch, one graph capture replayed on new poses, the committed 450 x 375 pair, the interface and the
refused arguments."""
import importlib
import os

import numpy as np
import pytest

import rectify_cases as rc
import rectify_ref as rr
import stereo_sgm_cases

pytestmark = pytest.mark.gpu
FILTERED = -16


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def types():
    return importlib.import_module("sfm-gms_amd.types")


@pytest.fixture(scope="module")
def scene_chain():
    return rc.scene_chain()


def _dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _hand_made_map(seed, h, w):
    """FILTERED codes, zeros, negative values, values below 16 and valid zeros among ordinary disparities."""
    rng = np.random.default_rng(seed)
    disp = rng.integers(16, 600, (h, w)).astype(np.int16)
    kind = rng.integers(0, 8, (h, w))
    disp[kind == 0] = FILTERED
    disp[kind == 1] = 0
    disp[kind == 2] = -rng.integers(1, 300, (h, w)).astype(np.int16)[kind == 2]
    disp[kind == 3] = rng.integers(1, 16, (h, w)).astype(np.int16)[kind == 3]
    valid = (rng.integers(0, 4, (h, w)) != 0).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    for k in range(4):
        assert (kind == k).any()
    assert (valid == 0).any()
    return disp, valid


def _run_cloud(ctx, torch, disp, valid, image, plans, min16, cap, reg=None):
    """gms_dense_cloud_device on n maps -> (xyz, color, pixel, count) host arrays; untouched entries hold the fill pattern."""
    n, h, w = disp.shape
    c = 0 if image is None else (1 if image.ndim == 3 else 3)
    ws_bytes = ctx.dense_cloud_workspace_bytes(w, h, n)
    assert ws_bytes > 0
    d_ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    d_disp, d_valid = torch.from_numpy(disp).cuda(), torch.from_numpy(valid).cuda()
    d_img = None if image is None else torch.from_numpy(np.ascontiguousarray(image)).cuda()
    d_plans = _dev(torch, np.concatenate(plans))
    d_xyz = torch.full((n, max(cap, 1), 3), -7.0, dtype=torch.float32, device="cuda")
    d_col = torch.full((n, max(cap, 1), max(c, 1)), 0xA5, dtype=torch.uint8, device="cuda")
    d_pix = torch.full((n, max(cap, 1)), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    kw = {}
    if reg is not None:
        pairs, regs, views = reg
        keep = [_dev(torch, pairs), _dev(torch, regs), _dev(torch, views)]
        kw = dict(d_pairs=keep[0].data_ptr(), d_reg=keep[1].data_ptr(), d_views=keep[2].data_ptr(), n_frames=len(views))
    torch.cuda.synchronize()
    ctx.dense_cloud_device(d_disp.data_ptr(), d_valid.data_ptr(), None if d_img is None else d_img.data_ptr(), c, c * w, n, w, h,
                           d_plans.data_ptr(), FILTERED, min16, d_ws.data_ptr(), ws_bytes, cap, d_xyz.data_ptr(),
                           None if d_img is None else d_col.data_ptr(), d_pix.data_ptr(), d_cnt.data_ptr(), **kw)
    ctx.synchronize()
    return d_xyz.cpu().numpy(), d_col.cpu().numpy(), d_pix.cpu().numpy(), d_cnt.cpu().numpy()


def _plan(size, name="rot10_x"):
    cam, dist, R, t, _, _ = rc.plan_inputs(name)
    return rr.make_plan(cam, dist, R, t, size)


@pytest.mark.parametrize("w,h", [(19, 13), (70, 40)])      # 70 x 40: more than one scan block of 1024 pixels per pair
@pytest.mark.parametrize("channels", [1, 3])
def test_cloud_batch_of_three_on_hand_made_planes(ctx, w, h, channels):
    import torch
    maps = [_hand_made_map(w + i, h, w) for i in range(3)]
    disp, valid = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    valid[1] = 0                                                 # a pair with no point
    image = rc.noise(3, 3, h, w) if channels == 1 else rc.noise(3, 3, h, w, 3)
    plans = [_plan((w, h), "rot10_x"), _plan((w, h), "rot10_z"), _plan((w, h), "t_plus_y")]
    for min16 in (16, 1, 200):
        want = [rr.cloud(disp[i], valid[i], image[i], plans[i], FILTERED, min16) for i in range(3)]
        full = max(len(x[0]) for x in want)
        assert full > (500 if w == 70 else 30) * (min16 != 200) and len(want[1][0]) == 0
        for cap in (full + 3, full // 2, 0):                     # room for all; fewer than the count; none
            xyz, col, pix, cnt = _run_cloud(ctx, torch, disp, valid, image, plans, min16, cap)
            for i in range(3):
                wx, wc, wp = want[i]
                k = min(len(wx), cap)
                assert cnt[i] == len(wx), (min16, cap, i)        # the count states all, also beyond cap
                assert xyz[i, :k].tobytes() == wx[:k].tobytes() and np.array_equal(pix[i, :k], wp[:k])
                assert np.array_equal(col[i, :k].reshape(wc[:k].shape), wc[:k])
                assert (np.diff(pix[i, :k]) > 0).all()           # raster order
                assert (xyz[i, k:] == -7.0).all() and (pix[i, k:] == -7).all() and (col[i, k:] == 0xA5).all()   # nothing past cap or count


def test_cloud_past_256_scan_blocks(ctx):
    """Two hand-made 512 x 520 maps: 260 blocks of 1024 pixels each, past one pass of cloud_scan_kernel, whose second pass adds the
    carry of the first 256. A cap above both counts, and one that ends inside block 258 of the first map: the counts, the bytes in
    raster order, and the fill behind the cap or the count."""
    import torch
    w, h = 512, 520
    maps = [_hand_made_map(900 + i, h, w) for i in range(2)]
    disp, valid = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    plans = [_plan((w, h), "rot10_x"), _plan((w, h), "rot10_z")]
    want = [rr.cloud(disp[i], valid[i], None, plans[i], FILTERED, 16) for i in range(2)]
    assert -(-w * h // 1024) == 260 and all((x[2] >= 257 * 1024).sum() > 1000 for x in want)     # points in the blocks behind the first pass
    inside = int(np.searchsorted(want[0][2], 258 * 1024)) + 100
    assert want[0][2][inside - 1] // 1024 == 258 == want[0][2][inside] // 1024
    for cap in (max(len(x[0]) for x in want) + 3, inside):
        xyz, _, pix, cnt = _run_cloud(ctx, torch, disp, valid, None, plans, 16, cap)
        for i in range(2):
            wx, _, wp = want[i]
            k = min(len(wx), cap)
            assert cnt[i] == len(wx), (cap, i)
            assert xyz[i, :k].tobytes() == wx[:k].tobytes() and np.array_equal(pix[i, :k], wp[:k]) and (np.diff(pix[i, :k]) > 0).all()
            assert (xyz[i, k:] == -7.0).all() and (pix[i, k:] == -7).all()


def test_cloud_with_a_registration_failed_pairs_and_no_image(ctx, types):
    import torch
    w, h = 70, 40
    maps = [_hand_made_map(40 + i, h, w) for i in range(4)]
    disp, valid = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    plans = [_plan((w, h), "rot10_x"), _plan((w, h), "rot10_y"), rr.zero_plan(), _plan((w, h), "rot10_z")]
    pairs = np.zeros(4, types.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [0, 1, 2, 7], [1, 2, 0, 1]          # the last pair names a frame that does not exist
    regs = np.zeros(4, types.SFM_PAIR_REG_DTYPE)
    regs["S"], regs["status"] = [1.0, 1.75, 2.0, 1.5], [0, 0, 0, 0]
    views = np.zeros(3, types.SFM_VIEW_DTYPE)
    views["R"][0], views["registered"] = np.eye(3), 1
    views["R"][1], views["t"][1] = rc.rot((1, 2, 3), 25), (0.3, -0.2, 1.5)
    views["R"][2], views["t"][2] = rc.rot((0, 1, 0), -40), (-2.0, 0.1, 0.4)
    for status1 in (0, 1, -8):                                               # GMS_OK, GMS_SFM_SKIPPED, GMS_ERR_NO_MODEL
        regs["status"][1] = status1
        xyz, _, pix, cnt = _run_cloud(ctx, torch, disp, valid, None, plans, 16, w * h, reg=(pairs, regs, views))
        for i in range(4):
            G = views[pairs["frame_a"][i]] if pairs["frame_a"][i] < 3 else None
            ok = plans[i]["status"][0] == 0 and G is not None and regs["status"][i] == 0
            wx, _, wp = rr.cloud(disp[i], valid[i], None, plans[i] if ok else rr.zero_plan(), FILTERED, 16, float(regs["S"][i]),
                                 None if G is None else (G["R"], G["t"]))
            assert cnt[i] == len(wx) and (len(wx) > 500) == bool(ok), (status1, i)
            assert xyz[i, :len(wx)].tobytes() == wx.tobytes() and np.array_equal(pix[i, :len(wx)], wp)
    # without the registration the same maps are in camera 1's frame
    xyz, _, pix, cnt = _run_cloud(ctx, torch, disp, valid, None, plans, 16, w * h)
    for i in (0, 1, 3):
        wx = rr.cloud(disp[i], valid[i], None, plans[i], FILTERED, 16)[0]
        assert cnt[i] == len(wx) and xyz[i, :len(wx)].tobytes() == wx.tobytes()
    assert cnt[2] == 0


def _scene_stack(torch, n):
    img1, img2 = rc.scene()
    return torch.from_numpy(np.stack([img1] * n)).cuda(), torch.from_numpy(np.stack([img2] * n)).cuda()


def _two_view(types, poses, statuses):
    tv = np.zeros(len(poses), types.TWO_VIEW_DTYPE)
    for i, (R, t) in enumerate(poses):
        tv["R"][i], tv["t"][i], tv["status"][i] = R, t, statuses[i]
    return tv


def _check_against_chain(run, j, chain):
    P, r1, r2, v1, disp, (xyz, colors, pixel) = chain
    assert run.plans()[j:j + 1].tobytes() == P.tobytes()
    assert np.array_equal(run.d_rect1[j].cpu().numpy(), r1) and np.array_equal(run.d_rect2[j].cpu().numpy(), r2)
    assert np.array_equal(run.d_valid[j].cpu().numpy(), v1) and np.array_equal(run.d_disp16[j].cpu().numpy(), disp)
    k = int(run.d_count[j])
    assert k == len(xyz) and run.d_xyz[j, :k].cpu().numpy().tobytes() == xyz.tobytes()
    assert np.array_equal(run.d_pixel[j, :k].cpu().numpy(), pixel) and np.array_equal(run.d_cloud_color[j, :k, 0].cpu().numpy(), colors)


def test_stage_on_the_scene_equals_the_numpy_chain_and_a_failed_pair_leaves_zeros(ctx, batch, types, scene_chain):
    import torch
    d1, d2 = _scene_stack(torch, 3)
    run = batch.DensePairs(ctx, 3, rc.SCENE_SIZE, rc.SCENE_SIZE, rc.SCENE_CAMERA, None, 1, params=rc.SCENE_SGM)
    refused = (np.diag([-1.0, -1.0, 1.0]), np.array([-1.0, 0.0, 0.0]))
    run.set_two_view(_two_view(types, [(rc.SCENE_R, rc.SCENE_T), (rc.SCENE_R, rc.SCENE_T), refused], [0, -8, 0]))
    for t in (run.d_rect1, run.d_rect2, run.d_valid, run.d_plans):
        t.fill_(0xA5)
    torch.cuda.synchronize()
    run.run(d1, d2)
    ctx.synchronize()
    _check_against_chain(run, 0, scene_chain)
    assert rc.scene_depth_error_share(run.d_xyz[0, :int(run.d_count[0])].cpu().numpy()) >= rc.SCENE_SHARE_MEASURED - rc.SCENE_SHARE_MARGIN
    for j in (1, 2):                                               # a failed two-view status; a pair that is not rectifiable
        assert run.plans()[j:j + 1].tobytes() == rr.zero_plan().tobytes()
        assert int(run.d_count[j]) == 0
        for t in (run.d_rect1, run.d_rect2, run.d_valid):
            assert not t[j].any()


def test_stage_bgr_input_colours_the_cloud(ctx, batch, types, scene_chain):
    import torch
    img1, img2 = rc.scene()
    bgr1 = np.stack([img1, img1, img1], axis=-1)                  # equal channels: the grey image is the channel, whatever the weights
    bgr2 = np.stack([img2, img2, img2], axis=-1)
    bgr1c = bgr1.copy()
    run = batch.DensePairs(ctx, 1, rc.SCENE_SIZE, rc.SCENE_SIZE, rc.SCENE_CAMERA, None, 3, params=rc.SCENE_SGM)
    run.set_two_view(_two_view(types, [(rc.SCENE_R, rc.SCENE_T)], [0]))
    torch.cuda.synchronize()
    run.run(torch.from_numpy(bgr1c[None]).cuda(), torch.from_numpy(bgr2[None]).cuda())
    ctx.synchronize()
    P, r1, r2, v1, disp, (xyz, colors, pixel) = scene_chain
    grey = run.d_rect1[0].cpu().numpy()
    if np.array_equal(grey, r1):                                   # (gms_bgr_to_gray_device of equal channels returns the channel)
        assert np.array_equal(run.d_disp16[0].cpu().numpy(), disp) and int(run.d_count[0]) == len(xyz)
    k = int(run.d_count[0])
    color = run.d_color[0].cpu().numpy()
    assert np.array_equal(color, np.stack([r1] * 3, axis=-1))
    assert k > 3000 and np.array_equal(run.d_cloud_color[0, :k].cpu().numpy(), color.reshape(-1, 3)[run.d_pixel[0, :k].cpu().numpy()])


def test_capture_and_replay_follows_new_poses(ctx, batch, types, scene_chain):
    import torch
    d1, d2 = _scene_stack(torch, 1)
    run = batch.DensePairs(ctx, 1, rc.SCENE_SIZE, rc.SCENE_SIZE, rc.SCENE_CAMERA, None, 1, params=rc.SCENE_SGM)
    other = (rc.rot((0, 0, 1), 3.0), np.array([-1.0, 0.1, 0.0]))
    run.set_two_view(_two_view(types, [other], [0]))
    torch.cuda.synchronize()
    run.run(d1, d2)                                                # (first use outside the capture)
    ctx.synchronize()
    first = run.d_rect2.cpu().numpy().copy()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):                   # one stream, no parallel branches
            run.run(d1, d2)
        run.set_two_view(_two_view(types, [(rc.SCENE_R, rc.SCENE_T)], [0]))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _check_against_chain(run, 0, scene_chain)
        assert not np.array_equal(run.d_rect2.cpu().numpy(), first)
        run.set_two_view(_two_view(types, [other], [0]))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(run.d_rect2.cpu().numpy(), first)
    finally:
        ctx.set_stream(None)


def test_fixture_450x375_identity_plan_reference_parameters(pkg, types):
    left, right, _ = stereo_sgm_cases.golden_pair()
    h, w = left.shape
    f = 400.0
    cam = (f, f, (w - 1) / 2.0, (h - 1) / 2.0)
    ref = types.STEREO_BM_REFERENCE
    r = pkg.denseStereo(left, right, cam, None, np.eye(3), (-1.0, 0.0, 0.0), num_disparities=ref["num_disparities"],
                        min_disparity=ref["min_disparity"])
    plan = r["plan"]
    assert plan["turn"] == 0 and np.array_equal(plan["R1"], np.eye(3)) and plan["B"] == 1.0 and plan["fx"] == f
    assert np.array_equal(r["rect1"], left) and np.array_equal(r["rect2"], right)
    assert np.array_equal(r["disp16"], pkg.stereoSGM(left, right))               # the matcher's own map of the pair
    d16 = r["disp16"].reshape(-1)[r["pixel"]].astype(np.float64)
    assert r["count"] == len(r["points"]) > 1000 and (d16 >= 16).all()
    assert np.array_equal(r["points"][:, 2], (f * 1.0 * 16.0 / d16).astype(np.float32))   # Z = f' B 16 / d16
    u, v = r["pixel"] % w, r["pixel"] // w
    assert np.array_equal(r["points"][:, 0], ((u - cam[2]) * (f * 16.0 / d16) / f).astype(np.float32))
    assert np.array_equal(r["points"][:, 1], ((v - cam[3]) * (f * 16.0 / d16) / f).astype(np.float32))
    want = rr.cloud(r["disp16"], r["valid"], left, plan.record, (ref["min_disparity"] - 1) * 16, 16)
    assert r["points"].tobytes() == want[0].tobytes() and np.array_equal(r["colors"], want[1]) and np.array_equal(r["pixel"], want[2])


def test_dense_stereo_host_arrays_and_device_tensors_give_the_same_bytes(pkg, scene_chain):
    import torch
    img1, img2 = rc.scene()
    P, r1, r2, v1, disp, (xyz, colors, pixel) = scene_chain
    host = pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, **rc.SCENE_SGM)
    dev = pkg.denseStereo(torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda(), rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T,
                          **rc.SCENE_SGM)
    for r, get in ((host, np.asarray), (dev, lambda t: t.cpu().numpy())):
        assert r["plan"].record.tobytes() == P.tobytes() and r["count"] == len(xyz)
        assert get(r["points"]).tobytes() == xyz.tobytes() and np.array_equal(get(r["pixel"]), pixel) and np.array_equal(get(r["colors"]), colors)
        assert np.array_equal(get(r["disp16"]), disp) and np.array_equal(get(r["rect1"]), r1) and np.array_equal(get(r["rect2"]), r2)
        assert np.array_equal(get(r["valid"]), v1)
    capped = pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, cap=100, **rc.SCENE_SGM)
    assert capped["count"] == len(xyz) and capped["points"].tobytes() == xyz[:100].tobytes()
    types = importlib.import_module("sfm-gms_amd.types")
    with pytest.raises(types.GmsError) as e:
        pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, np.diag([-1.0, -1.0, 1.0]), rc.SCENE_T, **rc.SCENE_SGM)
    assert e.value.code == -8
    with pytest.raises(types.GmsError) as e:
        pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, None, rc.SCENE_R, rc.SCENE_T, min_disp16=0, **rc.SCENE_SGM)
    assert e.value.code == -1


def test_structure_from_motion_dense_entry(pkg):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "image_sfm_pair_1008x756.npz"))
    img1, img2 = np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])
    cam = tuple(float(v) for v in z["camera"])
    base = pkg.structureFromMotion(img1, img2, cam, None, method="gms", max_keypoints=4000)
    assert "dense" not in base
    r = pkg.structureFromMotion(img1, img2, cam, None, method="gms", max_keypoints=4000, dense=True, dense_cap=200000)
    assert np.array_equal(r["R"], base["R"]) and np.array_equal(r["points3D"], base["points3D"])
    d = r["dense"]
    if d is None:                                                  # the recovered pose is outside what the plan rectifies
        plan = pkg.stereoRectify(cam, None, r["R"], r["t"], (img1.shape[1], img1.shape[0]))
        assert not plan.ok
        return
    plan = pkg.stereoRectify(cam, None, r["R"], r["t"], (img1.shape[1], img1.shape[0]))
    assert d["plan"].tobytes() == plan.record.tobytes()
    k = min(d["count"], 200000)
    assert d["points"].shape == (k, 3) and d["points"].dtype == np.float32 and len(d["pixel"]) == k and len(d["colors"]) == k
    assert (np.diff(d["pixel"]) > 0).all()


def test_bad_arguments_rejected_before_any_launch(ctx, types):
    import torch
    w, h = 70, 40
    disp, valid = _hand_made_map(1, h, w)
    d_disp, d_valid = torch.from_numpy(disp).cuda(), torch.from_numpy(valid).cuda()
    d_plans = _dev(torch, _plan((w, h)))
    ws_bytes = ctx.dense_cloud_workspace_bytes(w, h, 1)
    d_ws = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device="cuda")
    d_xyz = torch.full((w * h, 3), -7.0, dtype=torch.float32, device="cuda")
    d_pix = torch.full((w * h,), -7, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_col = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    base = dict(disp=d_disp.data_ptr(), valid=d_valid.data_ptr(), image=None, c=0, pitch=0, n=1, w=w, h=h, plans=d_plans.data_ptr(), min16=16,
                ws=d_ws.data_ptr(), ws_bytes=ws_bytes, cap=w * h, xyz=d_xyz.data_ptr(), col=None, pix=d_pix.data_ptr(), cnt=d_cnt.data_ptr(),
                pairs=None, reg=None, views=None, n_frames=0)
    bad = [dict(disp=None), dict(valid=None), dict(plans=None), dict(ws=None), dict(cnt=None), dict(xyz=None), dict(pix=None), dict(min16=0),
           dict(min16=-5), dict(cap=-1), dict(w=0), dict(h=8193), dict(n=-1), dict(n=65536), dict(ws=d_ws.data_ptr() + 64),
           dict(ws_bytes=ws_bytes - 1), dict(image=d_col.data_ptr(), c=2, pitch=2 * w), dict(image=d_col.data_ptr(), c=3, pitch=3 * w - 1),
           dict(col=d_col.data_ptr()), dict(pairs=d_pix.data_ptr()), dict(reg=d_pix.data_ptr(), views=d_pix.data_ptr()),
           dict(pairs=d_pix.data_ptr(), reg=d_pix.data_ptr(), views=d_pix.data_ptr(), n_frames=0)]
    for kw in bad:
        a = dict(base)
        a.update(kw)
        with pytest.raises(types.GmsError) as e:
            ctx.dense_cloud_device(a["disp"], a["valid"], a["image"], a["c"], a["pitch"], a["n"], a["w"], a["h"], a["plans"], FILTERED, a["min16"],
                                   a["ws"], a["ws_bytes"], a["cap"], a["xyz"], a["col"], a["pix"], a["cnt"], d_pairs=a["pairs"], d_reg=a["reg"],
                                   d_views=a["views"], n_frames=a["n_frames"])
        assert e.value.code == -1, kw
    assert ctx.dense_cloud_workspace_bytes(0, h, 1) == 0 and ctx.dense_cloud_workspace_bytes(w, h, 0) == 0
    assert ctx.dense_pairs_workspace_bytes(w, h, 2, w, h, 1) == 0 and ctx.dense_pairs_workspace_bytes(w, h, 1, 8193, h, 1) == 0
    assert ctx.dense_pairs_workspace_bytes(w, h, 1, w, h, 1, dict(num_disparities=24)) == 0
    # the stage: every refusal before any launch
    batch = importlib.import_module("sfm-gms_amd.batch")
    run = batch.DensePairs(ctx, 1, (w, h), (w, h), rc.CAMERA_SMALL, rc.DIST_ALL, 1, params=dict(num_disparities=16))
    d_img = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    for t in (run.d_rect1, run.d_plans):
        t.fill_(0xA5)
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr()
    sbase = dict(img1=ptr(d_img), img2=ptr(d_img), n=1, sw=w, sh=h, c=1, tv=ptr(run.d_tv), ow=w, oh=h, min16=16, ws=ptr(run.d_ws), wsb=run.ws_bytes,
                 plans=ptr(run.d_plans), r1=ptr(run.d_rect1), r2=ptr(run.d_rect2), valid=ptr(run.d_valid), color=None, disp=ptr(run.d_disp16),
                 cap=run.cap, xyz=ptr(run.d_xyz), cc=ptr(run.d_cloud_color), pix=ptr(run.d_pixel), cnt=ptr(run.d_count))
    sbad = [dict(img1=None), dict(img2=None), dict(tv=None), dict(ws=None), dict(plans=None), dict(r1=None), dict(r2=None), dict(valid=None),
            dict(disp=None), dict(cnt=None), dict(xyz=None), dict(c=2), dict(c=3), dict(sw=0), dict(sh=8193), dict(ow=0), dict(oh=8193), dict(n=0),
            dict(min16=0), dict(cap=-1), dict(ws=ptr(run.d_ws) + 8), dict(wsb=run.ws_bytes - 1)]
    for kw in sbad:
        a = dict(sbase)
        a.update(kw)
        with pytest.raises(types.GmsError) as e:
            ctx.dense_pairs_device(run.camera, run.params, a["img1"], a["img2"], a["n"], a["sw"], a["sh"], a["c"], a["tv"], a["ow"], a["oh"], a["min16"],
                                   a["ws"], a["wsb"], a["plans"], a["r1"], a["r2"], a["valid"], a["color"], a["disp"], a["cap"], a["xyz"], a["cc"],
                                   a["pix"], a["cnt"])
        assert e.value.code == -1, kw
    ctx.synchronize()
    assert (d_xyz.cpu().numpy() == -7.0).all() and int(d_cnt[0]) == -7 and (run.d_rect1.cpu().numpy() == 0xA5).all()
    assert (run.d_plans.cpu().numpy() == 0xA5).all()
    with pytest.raises(types.GmsError):
        batch.DensePairs(ctx, 1, (w, h), (w, h), rc.CAMERA_SMALL, None, 2)
