"""-m gpu: the pyramid keypoint source (gms_detect_pyramid_batch_device / gms_pyramid_build_device) against its
numpy statement tests/pyramid_ref.py -- keypoints, rows, counts and per-level counts byte for byte --, against the single-scale call
at n_levels = 1, captured into a graph, and in front of the matcher, matchGMS and LOGOS on a photograph and its 0.6 x copy."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logos_ref  # noqa: E402
import pyramid_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STEREO = os.path.join(GOLDEN, "image_stereo_pair_450x375.npz")
MAIN = os.path.join(GOLDEN, "image_main_scenario_1080p.npz")


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def _check(ctx, oracle, imgs, threshold, max_kp, n_levels):
    kps, rows, lc = _batch().detect_images_pyramid(ctx, imgs, threshold, max_kp, n_levels)
    assert lc.shape == (len(imgs), n_levels)
    for i, img in enumerate(imgs):
        want_kp, want_rows, want_lc = pyramid_ref.detect(oracle, img, threshold, max_kp, n_levels)
        assert lc[i].tolist() == want_lc.tolist(), (i, lc[i], want_lc)
        assert len(kps[i]) == len(want_kp) and kps[i].tobytes() == want_kp.tobytes(), i
        assert rows[i].tobytes() == want_rows.tobytes(), i
    return kps, rows, lc


# (threshold, max_keypoints, n_levels): room for everything; quotas that cut inside a score's ties on several levels; fewer keypoints
# than levels (quota 0 on most levels); one keypoint; one level; sixteen levels asked for (the stop rule ends them)
STEREO_CASES = [(20, 10000, 8), (8, 700, 8), (5, 4000, 5), (20, 5, 8), (20, 1, 8), (12, 3000, 1), (30, 2500, 16), (254, 50, 4)]


@pytest.mark.parametrize("threshold,max_kp,n_levels", STEREO_CASES)
def test_stereo_pair_equals_statement(ctx, oracle, threshold, max_kp, n_levels):
    z = np.load(STEREO)
    kps, _, lc = _check(ctx, oracle, np.stack([z["left"], z["right"]]), threshold, max_kp, n_levels)
    if (threshold, max_kp, n_levels) == (20, 10000, 8):
        assert (lc > 0).all() and len(np.unique(kps[0]["size"])) == 8


@pytest.mark.parametrize("threshold,max_kp,n_levels", [(20, 10000, 8), (10, 2000, 8), (20, 4000, 3)])
def test_1080p_pair_equals_statement(ctx, oracle, threshold, max_kp, n_levels):
    z = np.load(MAIN)
    _check(ctx, oracle, np.stack([z["left"], z["right"]]), threshold, max_kp, n_levels)


@pytest.mark.parametrize("w,h", [(33, 33), (97, 65), (64, 48), (130, 200), (641, 479), (1030, 50)])
def test_odd_sizes_noise_and_ties(ctx, oracle, w, h):
    """A batch of three images: noise, two grey levels (every score ties, so every quota cuts inside a tie), sparse dots."""
    rng = np.random.default_rng(w * 1000 + h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    blocks = (np.kron(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), dtype=np.int64))[:h, :w] * 90 + 60).astype(np.uint8)
    sparse = np.full((h, w), 40, dtype=np.uint8)
    sparse[rng.integers(0, h, 60), rng.integers(0, w, 60)] = 200
    imgs = np.stack([noise, blocks, sparse])
    for threshold, max_kp, n_levels in ((10, 10000, 8), (30, 37, 8), (0, 5, 16), (10, 300, 2)):
        _, _, lc = _check(ctx, oracle, imgs, threshold, max_kp, n_levels)
        assert (lc[:, len(pyramid_ref.level_sizes(w, h, n_levels)):] == 0).all()
    if (w, h) == (33, 33):
        assert len(ctx.pyramid_level_sizes(w, h, 8)) == 1


def test_level_sizes_equal_statement(ctx):
    for w, h in ((1920, 1080), (450, 375), (33, 33), (97, 65), (1030, 50), (65535, 40), (4000, 3000)):
        for n_levels in (1, 2, 8, 16):
            assert ctx.pyramid_level_sizes(w, h, n_levels) == pyramid_ref.level_sizes(w, h, n_levels)


@pytest.mark.parametrize("w,h,n", [(450, 375, 2), (97, 65, 3), (641, 479, 1), (1030, 50, 3), (1921, 1083, 2), (130, 200, 5)])
def test_build_pyramid_equals_numpy_resize(ctx, w, h, n):
    """gms_pyramid_build_device alone. Odd widths put the rows of the levels at every byte alignment."""
    if (w, h) == (450, 375):
        z = np.load(STEREO)
        imgs = np.stack([z["left"], z["right"]])
    else:
        imgs = np.random.default_rng(w + h).integers(0, 256, (n, h, w), dtype=np.uint8)
    got = _batch().build_pyramid(ctx, imgs, 16)
    want = [pyramid_ref.build(img, 16) for img in imgs]
    assert len(got) == len(want[0]) >= 2
    for l in range(len(got)):
        assert got[l].shape == (n,) + want[0][l].shape
        for i in range(n):
            assert np.array_equal(got[l][i], want[i][l]), (l, i)


def test_one_level_equals_the_single_scale_call(ctx):
    batch = _batch()
    z = np.load(STEREO)
    imgs = np.stack([z["left"], z["right"]])
    for threshold, max_kp in ((20, 10000), (8, 700), (20, 1)):
        kps, rows, lc = batch.detect_images_pyramid(ctx, imgs, threshold, max_kp, 1)
        want_kp, want_rows = batch.detect_images(ctx, imgs, threshold, max_kp)
        for i in range(2):
            assert kps[i].tobytes() == want_kp[i].tobytes() and rows[i].tobytes() == want_rows[i].tobytes() and lc[i, 0] == len(want_kp[i])


def test_argument_checks(ctx, pkg):
    import torch
    d = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    nb = ctx.detect_pyramid_workspace_bytes(100, 100, 1, 10, 8)
    assert 0 < nb <= 1 << 22
    out = [torch.zeros(1024, dtype=torch.uint8, device="cuda:0") for _ in range(4)]     # keypoints, rows, counts, level counts
    img = torch.zeros(100 * 100, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.detect_pyramid_batch_device(img.data_ptr(), 1, 100, 100, 20, 10, 8, p, nb, *[t.data_ptr() for t in out])   # exactly enough
    ctx.synchronize()
    with pytest.raises(pkg.GmsError):
        ctx.detect_pyramid_batch_device(p, 1, 100, 100, 20, 10, 8, p, nb - 1, p, p, p, p)       # workspace one byte short
    for n_levels in (0, 17):
        with pytest.raises(pkg.GmsError):
            ctx.detect_pyramid_batch_device(p, 1, 100, 100, 20, 10, n_levels, p, 1 << 22, p, p, p, p)
        with pytest.raises(pkg.GmsError):
            ctx.pyramid_build_device(p, 1, 100, 100, n_levels, p, 1 << 22)
        with pytest.raises(pkg.GmsError):
            ctx.pyramid_level_sizes(100, 100, n_levels)
        assert ctx.detect_pyramid_workspace_bytes(100, 100, 1, 10, n_levels) == 0
    with pytest.raises(pkg.GmsError):
        ctx.detect_pyramid_batch_device(p, 1, 100, 100, 255, 10, 8, p, 1 << 22, p, p, p, p)     # threshold
    with pytest.raises(pkg.GmsError):
        ctx.detect_pyramid_batch_device(p, 1, 32, 100, 20, 10, 8, p, 1 << 22, p, p, p, p)       # no room for a keypoint
    with pytest.raises(pkg.GmsError):
        ctx.detect_pyramid_batch_device(p, 1, 100, 100, 20, 10, 8, p, 1 << 22, p, p, p, None)   # no per-level counts
    with pytest.raises(pkg.GmsError):
        ctx.pyramid_build_device(p, 1, 100, 100, 8, p, 100)                                       # no room for the levels
    ctx.detect_pyramid_batch_device(p, 0, 100, 100, 20, 10, 8, None, 0, None, None, None, None)  # nothing to do
    ctx.pyramid_build_device(None, 0, 100, 100, 8, None, 0)


def test_graph_replay_on_new_pixels(ctx, oracle):
    import torch
    batch = _batch()
    z = np.load(STEREO)
    first, second = np.stack([z["left"], z["right"]]), np.stack([z["right"][::-1].copy(), z["left"][:, ::-1].copy()])
    h, w = z["left"].shape
    d_imgs = torch.from_numpy(first).cuda()
    run = batch.DetectPyramid(ctx, 2, w, h, 12, 1500, 8)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(stream):
            run.run(d_imgs)                                   # warm-up
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            run.run(d_imgs)
        for imgs in (second, first):
            d_imgs.copy_(torch.from_numpy(imgs))
            for t in (run.d_kp, run.d_desc, run.d_counts, run.d_level_counts):
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = run.results()
            with torch.cuda.stream(stream):
                run.run(d_imgs)                               # the direct call on the same pixels
            stream.synchronize()
            direct = run.results()
            for i in range(2):
                want_kp, want_rows, want_lc = pyramid_ref.detect(oracle, imgs[i], 12, 1500, 8)
                for kps, rows, lc in (got, direct):
                    assert kps[i].tobytes() == want_kp.tobytes() and rows[i].tobytes() == want_rows.tobytes() and lc[i].tolist() == want_lc.tolist()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        g.reset()      # released here, not when a failure's traceback lets go of it at interpreter exit


def _pipeline(ctx, pkg, oracle, kps, rows, sizes, sx, sy):
    """keypoints + rows of (left, right) -> Hamming matches -> matchGMS(rotation, scale). Returns (survivors, correct survivors)."""
    batch = _batch()
    table = batch.FrameTable(ctx, kps, sizes)
    dt = batch.DescriptorTable(ctx, table, rows, pkg.GMS_DESC_HAMMING256)
    pairs = np.zeros(1, dtype=pkg.PAIR_DTYPE)
    pairs[0] = (0, 1, len(kps[0]), 0, 0)
    matches = batch.match_pairs(ctx, dt, pairs)
    assert matches.tobytes() == oracle.bf_match(rows[0], rows[1], True).tobytes()
    out, res, _ = batch.filter_pairs(ctx, table, pairs, matches, True, True, 6.0)
    rc, want, _, _ = oracle.match(sizes[0], sizes[1], kps[0], kps[1], matches, True, True, 6.0)
    n = int(res["n_inliers"][0])
    assert rc == 0 and res["status"][0] == 0 and n == len(want) and out[:n].tobytes() == want.tobytes()
    q, t = kps[0][out["queryIdx"][:n]], kps[1][out["trainIdx"][:n]]
    ex, ey = (q["x"] + 0.5) * sx - 0.5, (q["y"] + 0.5) * sy - 0.5
    return n, int((np.hypot(t["x"] - ex, t["y"] - ey) <= 3.0).sum())


def test_pipeline_on_a_shrunk_copy(ctx, pkg, oracle):
    """1080p left against its 0.6 x copy: pyramid keypoints -> the Hamming matcher -> matchGMS(with_rotation, with_scale) equals the
    oracle filter on the same inputs, and the share of survivors that are correct (within 3 pixels of where the shrink puts the left
    keypoint) is above the single-scale pipeline's. One LOGOS call on a subset of the same keypoints equals tests/logos_ref.py: the
    varying size goes through."""
    batch = _batch()
    left = np.load(MAIN)["left"]
    h, w = left.shape
    wr, hr = 1152, 648
    right = pyramid_ref.resize(left, wr, hr)
    sizes = [(w, h), (wr, hr)]
    kps, rows = [], []
    for img in (left, right):
        k, r, _ = batch.detect_images_pyramid(ctx, img, 20, 4000, 8)
        want_kp, want_rows, _ = pyramid_ref.detect(oracle, img, 20, 4000, 8)
        assert k[0].tobytes() == want_kp.tobytes() and r[0].tobytes() == want_rows.tobytes()
        kps.append(k[0])
        rows.append(r[0])
    n_pyr, ok_pyr = _pipeline(ctx, pkg, oracle, kps, rows, sizes, wr / w, hr / h)
    single = [batch.detect_images(ctx, img, 20, 4000) for img in (left, right)]
    n_one, ok_one = _pipeline(ctx, pkg, oracle, [s[0][0] for s in single], [s[1][0] for s in single], sizes, wr / w, hr / h)
    print(f"\n0.6 x: pyramid {len(kps[0])}/{len(kps[1])} keypoints, {n_pyr} survivors, {ok_pyr} correct; "
          f"single scale {len(single[0][0][0])}/{len(single[1][0][0])} keypoints, {n_one} survivors, {ok_one} correct")
    assert n_pyr > 0 and ok_pyr > ok_one
    assert ok_pyr / n_pyr > (ok_one / n_one if n_one else 0.0)
    # LOGOS: every third keypoint of both frames, words from a dictionary of 40 of the left rows
    sub = [k[::3].copy() for k in kps]
    sub_rows = [r[::3] for r in rows]
    assert len(np.unique(sub[0]["size"])) > 4
    dictionary = sub_rows[0][:: max(len(sub_rows[0]) // 40, 1)][:40]
    words = batch.logos_words(ctx, sub_rows, dictionary, pkg.GMS_DESC_HAMMING256)
    table = batch.LogosTable(ctx, sub, words, len(dictionary))
    got, lres = batch.logos_pairs(ctx, table, [(0, 1)])
    a4 = [np.stack([k["x"], k["y"], k["size"], k["angle"]], axis=1) for k in sub]
    want = np.asarray(logos_ref.match(a4[0], a4[1], words[0], words[1])).reshape(-1, 2)
    assert lres["status"][0] == 0 and len(got[0]) == len(want) > 0
    assert np.array_equal(got[0]["queryIdx"], want[:, 0]) and np.array_equal(got[0]["trainIdx"], want[:, 1])
