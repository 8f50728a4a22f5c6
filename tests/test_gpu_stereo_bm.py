"""-m gpu: StereoBM block matching (gms_stereo_bm_device, gms_stereo_bm, gms_stereo_bm_normalize_device) -- the int16
map and the cost byte for byte against the CPU statement tests/stereo_bm_ref.py on the reference's pair and over a seeded parameter
sweep, a batch against the one-shot calls, the reference's 8-bit map, graph replay and rejected parameters."""
import importlib
import os

import numpy as np
import pytest

import stereo_bm_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_stereo_pair_450x375.npz")


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def _pair(rng, h, w, shift):
    base = rng.integers(0, 256, (h, w + 48)).astype(np.int32)
    base = (base + np.roll(base, 1, axis=1) + np.roll(base, 1, axis=0)) // 3
    left = base[:, 48:]
    right = base[:, 48 - shift:w + 48 - shift] + rng.integers(-3, 4, (h, w))
    return left.astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8)


def test_reference_pair_equals_statement(pkg):
    z = np.load(GOLDEN)
    want_d, want_c = R.stereo_bm(z["left"], z["right"])
    got_d, got_c = pkg.stereoBM(z["left"], z["right"], return_cost=True)
    assert got_d.tobytes() == want_d.tobytes()
    assert got_c.tobytes() == want_c.tobytes()


def test_stereo_match_equals_statement(pkg):
    z = np.load(GOLDEN)
    assert pkg.stereo_match(z["left"], z["right"]).tobytes() == R.stereo_match(z["left"], z["right"]).tobytes()


# blockSize, nd, md, cap, textureThreshold, uniquenessRatio, disp12MaxDiff, (H, W)
SWEEP = [
    (5, 16, 0, 61, 0, 0, 1, (40, 64)),
    (5, 224, -39, 61, 507, 0, 1, (61, 300)),
    (7, 32, -5, 15, 0, 15, 0, (47, 97)),
    (9, 48, 7, 31, 507, 0, -1, (52, 131)),
    (21, 64, 0, 63, 0, 15, 4, (64, 150)),
    (5, 96, -100, 61, 0, 0, 1, (33, 200)),
    (7, 128, 10, 15, 507, 15, 1, (45, 211)),
    (9, 256, -20, 31, 0, 0, 0, (38, 333)),
    (5, 512, -3, 63, 0, 0, 1, (29, 640)),
    (5, 112, 0, 61, 0, 0, 1, (20, 100)),     # width1 < 1: all FILTERED
    (51, 80, -30, 61, 100, 5, 2, (70, 190)),
    (5, 16, -8, 1, 0, 0, -1, (6, 7)),
]


@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_sweep_equals_statement(pkg, case):
    bs, nd, md, cap, tex, ur, dmd, (h, w) = SWEEP[case]
    rng = np.random.default_rng(40 + case)
    left, right = _pair(rng, h, w, int(rng.integers(0, 12)))
    kw = dict(block_size=bs, num_disparities=nd, min_disparity=md, pre_filter_cap=cap, texture_threshold=tex, uniqueness_ratio=ur,
              disp12_max_diff=dmd)
    want_d, want_c = R.stereo_bm(left, right, **kw)
    got_d, got_c = pkg.stereoBM(left, right, return_cost=True, **kw)
    assert got_d.tobytes() == want_d.tobytes(), kw
    assert got_c.tobytes() == want_c.tobytes(), kw


def test_batch_equals_one_shot(ctx, pkg):
    batch = _batch()
    rng = np.random.default_rng(9)
    pairs = [_pair(rng, 75, 180, s) for s in (0, 3, 7, 11, 20)]
    pairs.append((pairs[0][0], pairs[0][0]))
    lefts = np.stack([p[0] for p in pairs])
    rights = np.stack([p[1] for p in pairs])
    kw = dict(num_disparities=64, min_disparity=-4, texture_threshold=100, uniqueness_ratio=10)
    d, c, d8 = batch.stereo_bm_batch(lefts, rights, kw, ctx, return_cost=True, eight_bit=True)
    for i, (l, r) in enumerate(pairs):
        one_d, one_c = pkg.stereoBM(l, r, return_cost=True, **kw)
        assert d[i].tobytes() == one_d.tobytes()
        assert c[i].tobytes() == one_c.tobytes()
        assert d8[i].tobytes() == pkg.stereo_match(l, r, **kw).tobytes() == R.normalize_u8(one_d).tobytes()


def test_graph_replay(ctx, pkg):
    import torch
    batch = _batch()
    z = np.load(GOLDEN)
    dl = torch.from_numpy(np.stack([z["left"], z["right"]])).cuda()
    dr = torch.from_numpy(np.stack([z["right"], z["left"]])).cuda()
    run = batch.StereoBM(ctx, 2, z["left"].shape[1], z["left"].shape[0])
    run.run(dl, dr, eight_bit=True)
    ctx.synchronize()
    first = [t.cpu().numpy().tobytes() for t in (run.d_disp, run.d_cost, run.d_out8)]
    assert first[0] == R.stereo_bm(z["left"], z["right"])[0].tobytes() + R.stereo_bm(z["right"], z["left"])[0].tobytes()
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            run.run(dl, dr, eight_bit=True)
        for _ in range(2):
            for t in (run.d_disp, run.d_cost, run.d_out8):
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert [t.cpu().numpy().tobytes() for t in (run.d_disp, run.d_cost, run.d_out8)] == first
    finally:
        ctx.set_stream(None)


def test_bad_params_rejected_before_launch(ctx, pkg):
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    img = np.zeros((40, 64), np.uint8)
    for kw in (dict(block_size=6), dict(block_size=53), dict(num_disparities=24), dict(num_disparities=528), dict(pre_filter_cap=0),
               dict(pre_filter_cap=64), dict(speckle_window_size=100), dict(pre_filter_type=0), dict(block_size=41),
               dict(uniqueness_ratio=-1), dict(texture_threshold=-1), dict(min_disparity=-2048)):
        with pytest.raises(types.GmsError) as e:
            pkg.stereoBM(img, img, **kw)
        assert e.value.code == -1, kw
        assert ctx.stereo_bm_workspace_bytes(64, 40, 1, kw) == 0
    d = torch.zeros(64 * 40 * 2, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(ctx.stereo_bm_workspace_bytes(64, 40, 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(types.GmsError) as e:  # pitch below the width
        ctx.stereo_bm_device(None, d.data_ptr(), d.data_ptr(), 1, 64, 40, 63, ws.data_ptr(), ws.numel(), d.data_ptr())
    assert e.value.code == -1
    with pytest.raises(types.GmsError) as e:  # workspace too small
        ctx.stereo_bm_device(None, d.data_ptr(), d.data_ptr(), 1, 64, 40, 64, ws.data_ptr(), ws.numel() - 256, d.data_ptr())
    assert e.value.code == -1
    with pytest.raises(types.GmsError) as e:
        pkg.stereoBM(np.zeros((40, 8193), np.uint8), np.zeros((40, 8193), np.uint8))
    assert e.value.code == -1
