"""-m gpu: semi-global matching on StereoBM's costs (gms_stereo_sgm_device, gms_stereo_sgm) -- the int16 map and the
cost byte for byte against the CPU statement tests/stereo_sgm_ref.py: the committed pair with 8 and 4 paths, the named cases of
tests/stereo_sgm_cases.py (whose content the CPU suite asserts), batches, a padded pitch (two pairs at block size 5, three at 9), an
exact workspace with guard bytes, zero penalties against gms_stereo_bm_device on the device, graph replay, the one-shot calls on host
arrays and device tensors, and rejected parameters. On a difference a test names the first differing pixel."""
import importlib

import numpy as np
import pytest

import stereo_bm_ref as B
import stereo_sgm_cases as C
import stereo_sgm_ref as R

pytestmark = pytest.mark.gpu


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def _assert_same(got, want, what):
    """Byte for byte, and on a mismatch the first differing pixel."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        ys, xs = np.nonzero(got != want)
        y, x = int(ys[0]), int(xs[0])
        raise AssertionError(f"{what}: {len(ys)} of {got.size} pixels differ, the first at (y, x) = ({y}, {x}): got {got[y, x]}, want {want[y, x]}")


@pytest.mark.parametrize("n_paths", [8, 4])
def test_committed_pair_equals_statement(pkg, n_paths):
    left, right, _ = C.golden_pair()
    want_d, want_c = C.golden_expected(n_paths)
    got_d, got_c = pkg.stereoSGM(left, right, return_cost=True, n_paths=n_paths)
    _assert_same(got_c, want_c, ("pair", n_paths, "cost"))
    _assert_same(got_d, want_d, ("pair", n_paths, "disparity"))


@pytest.mark.parametrize("name", C.NAMES)
def test_named_cases_equal_statement(pkg, name):
    left, right, kw = C.case(name)
    want_d, want_c = C.expected(name)
    got_d, got_c = pkg.stereoSGM(left, right, return_cost=True, **kw)
    _assert_same(got_c, want_c, (name, "cost"))
    _assert_same(got_d, want_d, (name, "disparity"))


@pytest.mark.parametrize("name", ["const", "lr_0", "rofs_5"])
def test_eight_bit_map(pkg, name):
    left, right, kw = C.case(name)
    want = B.normalize_u8(C.expected(name)[0])
    _assert_same(pkg.stereo_match_sgm(left, right, **kw), want, name)
    assert want.tobytes() == R.stereo_match_sgm(left, right, **kw).tobytes()


def test_two_pairs_in_one_batch(ctx, pkg):
    """Different content side by side in blockIdx.y of the path kernels, with the costs and the 8-bit maps."""
    names = ["md_negative", "md_zero"]
    pairs = [C.case(n) for n in names]
    kw = pairs[0][2]
    lefts, rights = np.stack([pairs[0][0], pairs[1][1]]), np.stack([pairs[0][1], pairs[1][0]])   # the second pair swapped: other content
    want = [C.expected(names[0]), R.stereo_sgm(lefts[1], rights[1], **kw)]
    d, c, d8 = _batch().stereo_sgm_batch(lefts, rights, kw, ctx, return_cost=True, eight_bit=True)
    assert d[0].tobytes() != d[1].tobytes()
    for i in range(2):
        _assert_same(c[i], want[i][1], (i, "cost"))
        _assert_same(d[i], want[i][0], (i, "disparity"))
        _assert_same(d8[i], B.normalize_u8(want[i][0]), (i, "8-bit"))


def test_padded_pitch(ctx):
    """pitch = W + 37 through gms_stereo_sgm_device: the statement's bytes, with and without the cost map, whatever the padding holds."""
    import torch
    left, right, kw = C.case("lr_2")
    H, W = left.shape
    pad = 37
    want = [C.expected("lr_2"), R.stereo_sgm(right, left, **kw)]
    rng = np.random.default_rng(3)
    rows_l = rng.integers(0, 256, (2, H, W + pad)).astype(np.uint8)
    rows_r = rng.integers(0, 256, (2, H, W + pad)).astype(np.uint8)
    rows_l[0, :, :W], rows_r[0, :, :W] = left, right
    rows_l[1, :, :W], rows_r[1, :, :W] = right, left
    d_l, d_r = torch.from_numpy(rows_l).cuda(), torch.from_numpy(rows_r).cuda()
    ws_bytes = ctx.stereo_sgm_workspace_bytes(W, H, 2, kw)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    for with_cost in (True, False):
        d_disp = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
        d_cost = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.stereo_sgm_device(kw, d_l.data_ptr(), d_r.data_ptr(), 2, W, H, W + pad, ws.data_ptr(), ws_bytes, d_disp.data_ptr(),
                              d_cost.data_ptr() if with_cost else None)
        ctx.synchronize()
        for i in range(2):
            _assert_same(d_disp[i].cpu().numpy(), want[i][0], ("pitch", with_cost, i, "disparity"))
            if with_cost:
                _assert_same(d_cost[i].cpu().numpy(), want[i][1], ("pitch", i, "cost"))
        assert with_cost or not bool(d_cost.any())      # no cost map asked for: none written


def test_three_pairs_at_block_9_with_padded_pitch(ctx):
    """bs9_seams' parameters through gms_stereo_sgm_device with n = 3 and pitch = W + 37: the case, the case with left and right
    exchanged, and the case upside down, side by side in the cost kernel's blockIdx.z over random padding."""
    import torch
    left, right, kw = C.case("bs9_seams")
    H, W = left.shape
    pad = 37
    pairs = [(left, right), (right, left), (np.ascontiguousarray(left[::-1]), np.ascontiguousarray(right[::-1]))]
    want = [C.expected("bs9_seams")] + [R.stereo_sgm(l, r, **kw) for l, r in pairs[1:]]
    assert len({w[0].tobytes() for w in want}) == 3
    rng = np.random.default_rng(9)
    rows_l = rng.integers(0, 256, (3, H, W + pad)).astype(np.uint8)
    rows_r = rng.integers(0, 256, (3, H, W + pad)).astype(np.uint8)
    for i, (l, r) in enumerate(pairs):
        rows_l[i, :, :W], rows_r[i, :, :W] = l, r
    d_l, d_r = torch.from_numpy(rows_l).cuda(), torch.from_numpy(rows_r).cuda()
    ws_bytes = ctx.stereo_sgm_workspace_bytes(W, H, 3, kw)
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    d_disp = torch.zeros((3, H, W), dtype=torch.int16, device="cuda")
    d_cost = torch.zeros((3, H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.stereo_sgm_device(kw, d_l.data_ptr(), d_r.data_ptr(), 3, W, H, W + pad, ws.data_ptr(), ws_bytes, d_disp.data_ptr(), d_cost.data_ptr())
    ctx.synchronize()
    for i in range(3):
        _assert_same(d_cost[i].cpu().numpy(), want[i][1], ("block 9", i, "cost"))
        _assert_same(d_disp[i].cpu().numpy(), want[i][0], ("block 9", i, "disparity"))


@pytest.mark.parametrize("name", ["widest", "nd_512", "diag_tall", "bs51_nd512", "rofs_5"])
def test_workspace_exact(ctx, name):
    """A workspace of exactly gms_stereo_sgm_workspace_bytes with 256 guard bytes behind it, filled with a pattern before the run."""
    import torch
    GUARD, FILL = 256, 0xA5
    left, right, kw = C.case(name)
    H, W = left.shape
    ws_bytes = ctx.stereo_sgm_workspace_bytes(W, H, 1, kw)
    assert ws_bytes > ctx.stereo_bm_workspace_bytes(W, H, 1, {k: v for k, v in kw.items() if k in B.PARAM_NAMES}) > 0
    buf = torch.full((ws_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    d_l, d_r = torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda()
    d_disp = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    d_cost = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.stereo_sgm_device(kw, d_l.data_ptr(), d_r.data_ptr(), 1, W, H, W, buf.data_ptr(), ws_bytes, d_disp.data_ptr(), d_cost.data_ptr())
    ctx.synchronize()
    assert bool((buf[ws_bytes:] == FILL).all()), "the entry point wrote behind its workspace"
    want_d, want_c = C.expected(name)
    _assert_same(d_cost.cpu().numpy(), want_c, (name, "cost"))
    _assert_same(d_disp.cpu().numpy(), want_d, (name, "disparity"))


@pytest.mark.parametrize("name,n_paths", [("diag_wide", 8), ("md_positive", 4), ("stripes64", 8), ("bs7_seams", 8), ("bs21", 8), ("rofs_5", 4),
                                          ("bs51_nd512_four", 4)])
def test_zero_penalties_equal_stereo_bm_on_the_device(ctx, name, n_paths):
    """p1 = p2 = 0, uniqueness_ratio = 0: gms_stereo_bm_device's map byte for byte, and n_paths times its cost."""
    left, right, kw = C.case(name)
    kw = dict({k: v for k, v in kw.items() if k in B.PARAM_NAMES}, uniqueness_ratio=0)
    batch = _batch()
    lefts, rights = left[None].copy(), right[None].copy()
    bd, bc = batch.stereo_bm_batch(lefts, rights, kw, ctx, return_cost=True)
    sd, sc = batch.stereo_sgm_batch(lefts, rights, dict(kw, p1=0, p2=0, n_paths=n_paths), ctx, return_cost=True)
    _assert_same(sd, bd, (name, "disparity"))
    _assert_same(sc, np.where(bc >= 0, n_paths * bc, -1).astype(np.int32), (name, "cost"))
    assert (bd != B.filtered_value(B.make_params(**kw))).any()


def test_graph_replay_on_new_images(ctx):
    """One capture; the replay runs on new images written into the same tensors."""
    import torch
    batch = _batch()
    first = C.case("lr_0")
    kw = first[2]
    H, W = first[0].shape
    swapped = (np.ascontiguousarray(first[0][::-1]), np.ascontiguousarray(first[1][::-1]))     # new content: both images upside down
    want_first, want_second = C.expected("lr_0"), R.stereo_sgm(*swapped, **kw)
    dl, dr = torch.from_numpy(first[0][None].copy()).cuda(), torch.from_numpy(first[1][None].copy()).cuda()
    run = batch.StereoSGM(ctx, 1, W, H, kw)
    run.run(dl, dr, eight_bit=True)
    ctx.synchronize()
    _assert_same(run.d_disp[0].cpu().numpy(), want_first[0], "before capture")
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            run.run(dl, dr, eight_bit=True)
        dl.copy_(torch.from_numpy(swapped[0][None].copy()))
        dr.copy_(torch.from_numpy(swapped[1][None].copy()))
        for t in (run.d_disp, run.d_cost, run.d_out8):
            t.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _assert_same(run.d_cost[0].cpu().numpy(), want_second[1], "replay, cost")
        _assert_same(run.d_disp[0].cpu().numpy(), want_second[0], "replay, disparity")
        _assert_same(run.d_out8[0].cpu().numpy(), B.normalize_u8(want_second[0]), "replay, 8-bit")
        assert want_second[0].tobytes() != want_first[0].tobytes()
    finally:
        ctx.set_stream(None)


def test_one_shot_on_host_arrays_and_device_tensors(pkg):
    import torch
    left, right, kw = C.case("p1_zero")
    want_d, want_c = C.expected("p1_zero")
    d = pkg.stereoSGM(left, right, **kw)
    assert isinstance(d, np.ndarray)
    _assert_same(d, want_d, "host arrays")
    td, tc = pkg.stereoSGM(torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda(), return_cost=True, **kw)
    assert td.is_cuda and tc.is_cuda
    _assert_same(td.cpu().numpy(), want_d, "device tensors, disparity")
    _assert_same(tc.cpu().numpy(), want_c, "device tensors, cost")
    t8 = pkg.stereo_match_sgm(torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda(), **kw)
    _assert_same(t8.cpu().numpy(), B.normalize_u8(want_d), "device tensors, 8-bit")


def test_bad_params_rejected_before_launch(ctx, pkg):
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    img = np.zeros((40, 64), np.uint8)
    for kw in (dict(p1=-1), dict(p1=801), dict(n_paths=5), dict(n_paths=2), dict(pre_filter_cap=63, p2=5042), dict(speckle_window_size=100),
               dict(block_size=6), dict(num_disparities=24), dict(block_size=11)):     # (block 11: 8 (121 * 122 + 3872) is past 65535)
        with pytest.raises(types.GmsError) as e:
            pkg.stereoSGM(img, img, **kw)
        assert e.value.code == -1, kw
        assert ctx.stereo_sgm_workspace_bytes(64, 40, 1, kw) == 0, kw
    assert ctx.stereo_sgm_workspace_bytes(64, 40, 1, dict(pre_filter_cap=63, p2=5041)) > 0
    # block 9 with the default cap and penalties: 8 (81 * 122 + 2592) is past 65535; with cap 31 it is 60 912
    with pytest.raises(types.GmsError) as e:
        pkg.stereoSGM(img, img, block_size=9)
    assert e.value.code == -1
    assert ctx.stereo_sgm_workspace_bytes(64, 40, 1, dict(block_size=9)) == 0
    assert ctx.stereo_sgm_workspace_bytes(64, 40, 1, dict(block_size=9, pre_filter_cap=31)) > 0
    # block 51 at cap 1 with 8 paths: 8 (2601 * 2 + 2989) = 65 528 is the last accepted p2
    tall = np.zeros((60, 64), np.uint8)
    at = dict(block_size=51, pre_filter_cap=1, p1=200, p2=2989)
    assert ctx.stereo_sgm_workspace_bytes(64, 60, 1, at) > 0
    assert pkg.stereoSGM(tall, tall, **at).shape == tall.shape
    with pytest.raises(types.GmsError) as e:
        pkg.stereoSGM(tall, tall, **dict(at, p2=2990))
    assert e.value.code == -1
    assert ctx.stereo_sgm_workspace_bytes(64, 60, 1, dict(at, p2=2990)) == 0
    assert ctx.stereo_sgm_workspace_bytes(8192, 2 ** 31 - 1, 65535) == 0          # beyond size_t
    d = torch.zeros(64 * 40 * 2, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(ctx.stereo_sgm_workspace_bytes(64, 40, 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(types.GmsError) as e:  # pitch below the width
        ctx.stereo_sgm_device(None, d.data_ptr(), d.data_ptr(), 1, 64, 40, 63, ws.data_ptr(), ws.numel(), d.data_ptr())
    assert e.value.code == -1
    with pytest.raises(types.GmsError) as e:  # workspace too small
        ctx.stereo_sgm_device(None, d.data_ptr(), d.data_ptr(), 1, 64, 40, 64, ws.data_ptr(), ws.numel() - 256, d.data_ptr())
    assert e.value.code == -1
