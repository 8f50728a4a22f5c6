"""GPU: gms_rectify_plan_device, gms_rectify_device and their Python faces against tests/rectify_ref.py, byte for byte (DESIGN.md
§4.13), at the smallest shapes at which the kernels can go wrong: every plan case from two-view records on the device, images narrower
than a tile and wider than one, odd pitches that put rows at every byte alignment, 1 and 3 channels, plans that throw part of the
picture outside and rays that point away from the source; one graph capture replayed on new plans; the refused arguments."""
import importlib

import numpy as np
import pytest

import rectify_cases as rc
import rectify_ref as rr
import stereo_sgm_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def types():
    return importlib.import_module("sfm-gms_amd.types")


def _dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _plans_on_device(ctx, types, torch, camera, dist, poses, statuses, size, out_size):
    tv = np.zeros(len(poses), types.TWO_VIEW_DTYPE)
    for i, (R, t) in enumerate(poses):
        tv["R"][i], tv["t"][i], tv["status"][i] = np.asarray(R).reshape(3, 3), t, statuses[i]
    d_tv = _dev(torch, tv)
    d_plans = torch.full((len(poses) * 200,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.rectify_plan_device(types.make_camera(camera, dist), d_tv.data_ptr(), len(poses), size[0], size[1], out_size[0], out_size[1],
                            d_plans.data_ptr())
    ctx.synchronize()
    return d_plans.cpu().numpy().view(rr.PLAN_DTYPE)


@pytest.mark.parametrize("out_size", [(0, 0), (50, 31)])
def test_plan_kernel_every_case_and_a_failed_record(ctx, types, out_size):
    import torch
    groups = {}
    for name in rc.PLAN_CASES:
        cam, dist, R, t, _, _ = rc.plan_inputs(name)
        groups.setdefault((cam, dist), []).append((name, R, t))
    for (cam, dist), cases in groups.items():
        poses = [(R, t) for _, R, t in cases] + [(np.eye(3), np.array([-1.0, 0.0, 0.0]))]   # the last record: a good pose with a failed status
        statuses = [0] * len(cases) + [-8]
        got = _plans_on_device(ctx, types, torch, cam, dist, poses, statuses, rc.SIZE_SMALL, out_size)
        for i, (name, R, t) in enumerate(cases):
            want = rr.make_plan(cam, dist, R, t, rc.SIZE_SMALL, out_size)
            assert got[i:i + 1].tobytes() == want.tobytes(), (name, got[i], want)
        assert got[-1:].tobytes() == rr.zero_plan().tobytes()
        assert rr.make_plan(cam, dist, *poses[-1], rc.SIZE_SMALL, out_size)["status"][0] == 0


def test_plan_kernel_random_poses_more_than_one_block(ctx, types):
    import torch
    rng = np.random.default_rng(7)
    poses = [(rc.rot(rng.normal(size=3), rng.uniform(0, 100)), rng.normal(size=3)) for _ in range(300)]
    got = _plans_on_device(ctx, types, torch, rc.CAMERA_SMALL, rc.DIST_ALL, poses, [0] * 300, (67, 45), (0, 0))
    want = np.concatenate([rr.make_plan(rc.CAMERA_SMALL, rc.DIST_ALL, R, t, (67, 45)) for R, t in poses])
    assert 30 < int((want["status"] == 0).sum()) < 300
    assert got.tobytes() == want.tobytes()


def _pitched(torch, imgs, pitch, fill):
    n, h = imgs.shape[:2]
    row = imgs.reshape(n, h, -1)
    buf = np.full((n, h, pitch), fill, np.uint8)
    buf[:, :, :row.shape[2]] = row
    return torch.from_numpy(buf).cuda()


def _three_plans(size):
    """Three plans of one output size for images of `size`: a gentle pose, one that throws much of the picture outside, and a plan
    made by hand whose rays point away from the source over part of the picture."""
    cam, dist = rc.CAMERA_SMALL, rc.DIST_ALL
    out = (size[0] + 6, size[1] + 3)
    a = rr.make_plan(cam, dist, rc.rot((0, 0, 1), 10), (-1.0, 0.1, 0.05), size, out)
    b = rr.make_plan(cam, dist, rc.rot((0.2, 1, 0), 35), (-1.0, -0.4, 0.3), size, out)
    c = rr.identity_plan(cam, out)
    c["R1"][0] = rc.rot((0, 1, 0), 80).reshape(9)
    c["R2"][0] = rc.rot((1, 0, 0), -85).reshape(9)
    assert a["status"][0] == 0 and b["status"][0] == 0
    return [a, b, c], out


@pytest.mark.parametrize("w,h", [(37, 29), (67, 45)])
@pytest.mark.parametrize("channels", [1, 3])
def test_rectify_pitched_batch_three_plans_and_one_shared(ctx, types, w, h, channels):
    import torch
    imgs = rc.noise(w + channels, 3, h, w, channels)
    plans, (dw, dh) = _three_plans((w, h))
    sp, dp = channels * w + 5, channels * dw + 3          # odd pitches: rows start at every byte alignment
    d_src = _pitched(torch, imgs, sp, 7)
    cam = types.make_camera(rc.CAMERA_SMALL, rc.DIST_ALL)
    ims = imgs if channels == 3 else imgs[..., 0]
    seen_outside = seen_behind = False
    for which in (1, 2):
        for shared in (None, 0, 1, 2):
            use = plans if shared is None else [plans[shared]]
            d_plans = _dev(torch, np.concatenate(use))
            d_dst = torch.full((3, dh, dp), 0xA5, dtype=torch.uint8, device="cuda")
            d_valid = torch.full((3, dh, dw), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.rectify_device(cam, d_src.data_ptr(), 3, w, h, channels, sp, d_plans.data_ptr(), len(use), which, d_dst.data_ptr(), dw, dh, dp,
                               d_valid.data_ptr())
            ctx.synchronize()
            got, gv = d_dst.cpu().numpy(), d_valid.cpu().numpy()
            assert (got[:, :, channels * dw:] == 0xA5).all()
            for i in range(3):
                P = use[i if shared is None else 0]
                want, valid = rr.rectify(ims[i], rc.CAMERA_SMALL, rc.DIST_ALL, P, which, (dw, dh))
                assert np.array_equal(got[i, :, :channels * dw].reshape(want.shape), want), (which, shared, i)
                assert np.array_equal(gv[i], valid), (which, shared, i)
                front = rr.source_positions(rc.CAMERA_SMALL, rc.DIST_ALL, P, which, (dw, dh))[4]
                seen_outside |= bool(valid.any() and (valid == 0).any() and want.any())
                seen_behind |= bool((~front).any() and front.any())
    assert seen_outside and seen_behind


def test_failed_plan_gives_zeros_and_valid_is_optional(ctx, types):
    import torch
    w, h = 37, 29
    imgs = rc.noise(1, 2, h, w)
    good = rr.make_plan(rc.CAMERA_SMALL, rc.DIST_ALL, rc.rot((0, 0, 1), 10), (-1.0, 0.1, 0.05), (w, h))
    d_plans = _dev(torch, np.concatenate([rr.zero_plan(), good]))
    d_src = torch.from_numpy(imgs).cuda()
    d_dst = torch.full((2, h, w), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.rectify_device(types.make_camera(rc.CAMERA_SMALL, rc.DIST_ALL), d_src.data_ptr(), 2, w, h, 1, w, d_plans.data_ptr(), 2, 1,
                       d_dst.data_ptr(), w, h, w, None)
    ctx.synchronize()
    got = d_dst.cpu().numpy()
    assert not got[0].any()
    assert np.array_equal(got[1], rr.rectify(imgs[1], rc.CAMERA_SMALL, rc.DIST_ALL, good, 1)[0])


@pytest.mark.parametrize("shape", [(29, 37), (45, 67, 3)])
def test_python_faces_host_arrays_and_device_tensors(pkg, shape):
    import torch
    im = rc.noise(5, *shape)
    size = (shape[1], shape[0])
    for name in ("rot10_y", "t_plus_y"):
        cam, dist, R, t, _, _ = rc.plan_inputs(name)
        plan = pkg.stereoRectify(cam, dist, R, t, size)
        ref = rr.make_plan(cam, dist, R, t, size)
        assert plan.ok and plan.record.tobytes() == ref.tobytes()
        assert pkg.rectifyQ(plan).tobytes() == rr.plan_q(ref).tobytes()
        for which in (1, 2):
            want, valid = rr.rectify(im, cam, dist, ref, which)
            got, gv = pkg.rectify(im, plan, which, return_valid=True)
            assert np.array_equal(got, want) and np.array_equal(gv, valid)
            d = pkg.rectify(torch.from_numpy(im).cuda(), plan, which)
            assert torch.is_tensor(d) and d.is_cuda and np.array_equal(d.cpu().numpy(), want)
            assert np.array_equal(pkg.rectify(im, plan.record, which, camera=cam, dist=dist), want)
    und = rr.undistort(im, rc.CAMERA_SMALL, rc.DIST_ALL)
    assert np.array_equal(pkg.undistort(im, rc.CAMERA_SMALL, rc.DIST_ALL), und) and not np.array_equal(und, im)
    assert np.array_equal(pkg.undistort(torch.from_numpy(im).cuda(), rc.CAMERA_SMALL, rc.DIST_ALL).cpu().numpy(), und)
    assert np.array_equal(pkg.undistort(im, rc.CAMERA_SMALL, None), rr.undistort(im, rc.CAMERA_SMALL, None))


def test_fixture_450x375_under_the_identity_plan(pkg):
    left = stereo_sgm_cases.golden_pair()[0]
    h, w = left.shape
    cam = (400.0, 400.0, (w - 1) / 2.0, (h - 1) / 2.0)
    plan = pkg.stereoRectify(cam, None, np.eye(3), (-1.0, 0.0, 0.0), (w, h))
    assert plan.ok and plan["turn"] == 0 and np.array_equal(plan["R1"], np.eye(3)) and np.array_equal(plan["R2"], np.eye(3))
    assert (plan["cx"], plan["cy"], plan["B"]) == (cam[2], cam[3], 1.0)
    for which in (1, 2):
        got, valid = pkg.rectify(left, plan, which, return_valid=True)
        assert np.array_equal(got, left)
        assert valid[:-1, :-1].all() and not valid[-1].any() and not valid[:, -1].any()


def test_capture_and_replay_follows_new_plans(ctx, batch, types):
    import torch
    n, w, h = 2, 67, 41
    imgs = rc.noise(19, n, h, w, 3)
    d = torch.from_numpy(imgs).cuda()
    cam, dist = rc.CAMERA_SMALL, rc.DIST_ALL
    run = batch.Rectify(ctx, n, (w, h), (80, 50), types.make_camera(cam, dist), channels=3, n_plans=n)
    sets = [[rr.make_plan(cam, dist, rc.rot(axis, a), t, (w, h), (80, 50)) for axis, a, t in s] for s in (
        [((0, 0, 1), 10, (-1.0, 0.1, 0.0)), ((1, 0, 0), 5, (-1.0, 0.0, 0.2))],
        [((0, 1, 0), 20, (1.0, 0.3, 0.0)), ((1, 1, 0), 8, (-0.2, 1.0, 0.0))],
        [((0, 0, 1), 121, (-1.0, 0.0, 0.0)), ((1, 0, 1), 15, (-1.0, -0.5, 0.1))])]       # the last set: a refused pair
    assert sets[2][0]["status"][0] == -8
    run.set_plans(sets[0])
    torch.cuda.synchronize()
    run.run(d, 1)
    ctx.synchronize()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            run.run(d, 1)
        for plans in sets[1:] + sets[:1]:
            run.set_plans(plans)
            run.d_dst.fill_(0xA5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got, gv = run.d_dst.cpu().numpy(), run.d_valid.cpu().numpy()
            for i in range(n):
                want, valid = rr.rectify(imgs[i], cam, dist, plans[i], 1, (80, 50))
                assert np.array_equal(got[i], want) and np.array_equal(gv[i], valid)
    finally:
        ctx.set_stream(None)


def test_bad_arguments_rejected_and_nothing_written(ctx, pkg, types):
    import torch
    w, h = 16, 8
    d_src = torch.zeros(4 * h * w * 3, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((4 * h * w * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    d_plans = _dev(torch, np.concatenate([rr.identity_plan(rc.CAMERA_SMALL, (w, h))] * 3))
    d_tv = torch.zeros(232, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cam = types.make_camera(rc.CAMERA_SMALL, rc.DIST_ALL)
    s, o, p = d_src.data_ptr(), d_dst.data_ptr(), d_plans.data_ptr()
    bad = [dict(channels=2), dict(channels=4), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(sw=8193), dict(dh=8193), dict(n=0),
           dict(n=65536), dict(sp=3 * w - 1), dict(dp=3 * w - 1), dict(dst=s), dict(dst=s + 5), dict(src=None), dict(dst=None), dict(plans=None),
           dict(plans=p + 4), dict(n_plans=2), dict(n_plans=0), dict(which=0), dict(which=3)]
    for kw in bad:
        a = dict(src=s, n=3, sw=w, sh=h, channels=3, sp=3 * w, plans=p, n_plans=3, which=1, dst=o, dw=w, dh=h, dp=3 * w)
        a.update(kw)
        with pytest.raises(types.GmsError) as e:
            ctx.rectify_device(cam, a["src"], a["n"], a["sw"], a["sh"], a["channels"], a["sp"], a["plans"], a["n_plans"], a["which"], a["dst"],
                               a["dw"], a["dh"], a["dp"])
        assert e.value.code == -1, kw
    for kw in (dict(n=-1), dict(n=65536), dict(w=0), dict(h=8193), dict(ow=8193), dict(tv=None), dict(out=None)):
        a = dict(tv=d_tv.data_ptr(), n=1, w=w, h=h, ow=0, oh=0, out=o)
        a.update(kw)
        with pytest.raises(types.GmsError) as e:
            ctx.rectify_plan_device(cam, a["tv"], a["n"], a["w"], a["h"], a["ow"], a["oh"], a["out"])
        assert e.value.code == -1, kw
    ctx.synchronize()
    assert (d_dst.cpu().numpy() == 0xA5).all()
    for call in (lambda: pkg.rectify(np.zeros((h, w, 2), np.uint8), pkg.stereoRectify(rc.CAMERA_SMALL, None, np.eye(3), (-1, 0, 0), (w, h)), 1),
                 lambda: pkg.rectify(np.zeros((h, w), np.uint8), pkg.stereoRectify(rc.CAMERA_SMALL, None, np.eye(3), (0, 0, 1), (w, h)), 1),
                 lambda: pkg.rectify(np.zeros((h, w), np.uint8), rr.identity_plan(rc.CAMERA_SMALL, (w, h)), 1),
                 lambda: pkg.undistort(np.zeros((h, w, 4), np.uint8), rc.CAMERA_SMALL, None)):
        with pytest.raises((ValueError, types.GmsError)):
            call()
