"""-m gpu: the reference's bruteForceMatch on resident frames (gms_bf_select_device, gms_bf_match_select) --
byte-exact against the numpy restatement tests/bf_select_ref.py (oracle matcher -> OpenCV's one-sided cross-check -> MSVC sort
prefix -> ratio / size prune) through every matcher kernel, at frame sizes around the matcher's tiles, with duplicate rows,
empty frames, bad arguments, capacity overflow, more than 1024 pairs, graph replay, the one-shot call, detector rows and the
two-view chain."""
import importlib
import os

import numpy as np
import pytest

import bf_select_ref
import sfm_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 63, 64, 65, 511, 513, 1025]


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def _rows(kind, n, rng, dup_pool=None, integer=True):
    """n descriptor rows; dup_pool: draw from that many distinct rows (ties in the matcher and in the sort)."""
    m = n if dup_pool is None else dup_pool
    if kind == 0:
        base = rng.integers(0, 256, (max(m, 1), 32), dtype=np.uint8)
    elif integer:
        base = np.where(rng.uniform(size=(max(m, 1), 128)) < 0.4, rng.integers(0, 40, (max(m, 1), 128)), 0).astype(np.float32)
    else:
        base = (rng.uniform(size=(max(m, 1), 128)) * 3.0).astype(np.float32)
    if dup_pool is None:
        return base[:n].copy()
    return base[rng.integers(0, m, n)].copy()


def _tables(ctx, pkg, rows, kind):
    batch = _batch()
    kps = [np.zeros(len(r), pkg.KEYPOINT_DTYPE) for r in rows]
    frames = batch.FrameTable(ctx, kps, [(640, 480)] * len(rows))
    return batch.DescriptorTable(ctx, frames, rows, kind)


def _want(rows, a, b, kind, cross, coef, max_size, cache):
    key = (a, b, cross)
    if key not in cache:
        cache[key] = bf_select_ref.candidates(rows[a], rows[b], kind == 0, cross) if len(rows[a]) and len(rows[b]) else None
    c = cache[key]
    if c is None:
        return None, None
    q, t, d = c
    out, n_ratio, dm = bf_select_ref.select(q, t, d, coef, max_size)
    return out, (len(d), n_ratio, len(out), dm)


def _check(got, res, rows, fp, kind, cross, coef, max_size, cache):
    for k, (a, b) in enumerate(fp):
        want, stats = _want(rows, a, b, kind, cross, coef, max_size, cache)
        if want is None:
            assert int(res["status"][k]) == -2 and len(got[k]) == 0
            continue
        assert int(res["status"][k]) == 0, (a, b)
        assert got[k].tobytes() == want.tobytes(), (a, b, cross, coef, max_size)
        assert (int(res["n_candidates"][k]), int(res["n_ratio"][k]), int(res["n_out"][k])) == stats[:3]
        assert res["d_min"][k] == stats[3]


# ---- 1. every matcher kernel, sizes around the tiles, duplicates, cross-check on / off, coef and max_size --------------------------
VARIANTS = [("hamming_mfma", 0, True, True), ("hamming_valu", 0, False, True), ("l2_int", 1, True, True), ("l2_float", 1, True, False)]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_kernels_sizes_and_parameters(ctx, pkg, variant):
    _, kind, prepared, integer = variant
    batch = _batch()
    rng = np.random.default_rng(7 + kind * 3 + int(prepared) + 5 * int(integer))
    rows = [_rows(kind, n, rng, integer=integer) for n in SIZES]
    rows += [_rows(kind, 300, rng, dup_pool=20, integer=integer), _rows(kind, 700, rng, dup_pool=5, integer=integer)]
    descs = _tables(ctx, pkg, rows, kind)
    nf = len(rows)
    fp = [(a, (a * 3 + 1) % nf) for a in range(nf)] + [((a * 5 + 2) % nf, a) for a in range(nf)] + [(nf - 2, nf - 1), (nf - 1, nf - 2)]
    cache = {}
    for cross in (True, False):
        for coef, max_size in ((4.0, 500), (1.0, 500), (1e30, 1), (1e30, 0), (1e30, 5000), (4.0, 3)):
            got, res = batch.bf_select_pairs(ctx, descs, fp, cross, coef, max_size, use_prepared=prepared)
            _check(got, res, rows, fp, kind, cross, coef, max_size, cache)


@pytest.mark.parametrize("kind", [0, 1], ids=["hamming", "l2_int"])
def test_ten_thousand_rows(ctx, pkg, kind):
    """Pairs of 10 000 and 12 000 rows: a frame of 12 000 query rows takes the workspace path of the merge (slots beyond the 10 240
    LDS records), and of the sort without cross-check. The 12 000-row frame draws its rows from 3 000 distinct ones, so they repeat
    across many 32-row blocks: ties in the matcher, in the merge and in the sort."""
    batch = _batch()
    rng = np.random.default_rng(90 + kind)
    a = _rows(kind, 10000, rng)
    b = a.copy()
    noisy = rng.uniform(size=len(b)) < 0.3
    b[noisy] = _rows(kind, int(noisy.sum()), rng)
    c = _rows(kind, 12000, rng, dup_pool=3000)
    rows = [a, b, c]
    descs = _tables(ctx, pkg, rows, kind)
    fp = [(0, 1), (1, 0), (2, 0), (0, 2)]
    cache = {}
    for cross in (True, False):
        for coef, max_size in ((4.0, 500), (1e30, 20000)):
            got, res = batch.bf_select_pairs(ctx, descs, fp, cross, coef, max_size)
            _check(got, res, rows, fp, kind, cross, coef, max_size, cache)


# ---- 2. empty frames, bad arguments, overflow with canaries -----------------------------------------------------------------------
def test_empty_bad_and_overflow(ctx, pkg):
    import torch
    batch = _batch()
    types = importlib.import_module("sfm-gms_amd.types")
    rng = np.random.default_rng(3)
    rows = [_rows(0, 200, rng), _rows(0, 0, rng), _rows(0, 150, rng, dup_pool=10)]
    descs = _tables(ctx, pkg, rows, 0)
    recs = np.zeros(7, pkg.PAIR_DTYPE)
    recs["frame_a"] = [0, 1, 0, 5, 0, 2, 0]
    recs["frame_b"] = [2, 0, 1, 0, 2, 0, 2]
    recs["m"] = [500, 500, 500, 500, 3, 500, -1]
    recs["match_off"] = [0, 600, 1200, 1800, 2400, 2500, 3100]
    run = batch.BfSelect(ctx, descs, recs, True, 1e30, 500)
    run.d_out.fill_(0xAB)
    torch.cuda.synchronize()
    run.run()
    ctx.synchronize()
    out, res, pres = run.results()
    assert res["status"].tolist() == [0, -2, -2, -1, -5, 0, -1]
    assert pres["status"].tolist() == res["status"].tolist()
    want0, _ = _want(rows, 0, 2, 0, True, 1e30, 500, {})
    want5, _ = _want(rows, 2, 0, 0, True, 1e30, 500, {})
    assert int(res["n_out"][4]) == len(want0) > 3  # the count the overflowing pair needs
    raw = out.view(np.uint8).reshape(-1)
    written = np.zeros(len(raw), bool)
    for p, w in ((0, want0), (5, want5)):
        o = int(recs["match_off"][p])
        assert out[o:o + len(w)].tobytes() == w.tobytes()
        written[16 * o:16 * (o + len(w))] = True
    assert (raw[~written] == 0xAB).all()  # nothing of the overflowing, empty or bad pairs, nothing beyond each range
    assert pres["n_inliers"].tolist() == [len(want0), 0, 0, 0, 0, len(want5), 0]
    assert (pres["best_scale"] == -1).all() and (pres["best_rot"] == -1).all()
    # call-level argument errors: nothing runs
    for coef, ms in ((0.5, 500), (float("inf"), 500), (float("nan"), 500), (4.0, -1)):
        with pytest.raises(types.GmsError) as e:
            batch.BfSelect(ctx, descs, recs[:1], True, coef, ms).run()
        assert e.value.code == -1
    # a workspace too small for the matcher rows of the last pairs: those pairs alone get GMS_ERR_BAD_ARG
    small = batch.BfSelect(ctx, descs, recs[[0, 5]], True, 1e30, 500)
    small.ws_bytes = ctx.bf_select_workspace_bytes(2, small.max_rows, 160)
    small.run()
    ctx.synchronize()
    _, res2, _ = small.results()
    assert res2["status"].tolist() == [0, -1]


def test_pairs_short_of_room_are_run_again(ctx, pkg):
    """bf_select_pairs with room that two of three pairs exceed: those two are run a second time with the count they reported, and
    every pair's survivors and record equal those of the call with the default room, and the restatement's."""
    batch = _batch()
    rng = np.random.default_rng(29)
    rows = [_rows(0, n, rng) for n in (40, 70, 33)]
    descs = _tables(ctx, pkg, rows, 0)
    fp = [(0, 1), (1, 2), (2, 0)]
    first, res1 = batch.bf_select_pairs(ctx, descs, fp)
    n_out = [int(k) for k in res1["n_out"]]
    assert n_out[1] >= 1 and n_out[2] > 1   # (so that the room below is short for pairs 1 and 2)
    second, res2 = batch.bf_select_pairs(ctx, descs, fp, capacity=[n_out[0], n_out[1] - 1, 1])
    assert [a.tobytes() for a in second] == [a.tobytes() for a in first]
    assert res2.tobytes() == res1.tobytes()
    _check(second, res2, rows, fp, 0, True, 4.0, 500, {})


# ---- 3. more than 1024 pairs ----------------------------------------------------------------------------------------------------
def test_more_than_1024_pairs(ctx, pkg):
    batch = _batch()
    rng = np.random.default_rng(41)
    n_frames = 36
    rows = [_rows(0, int(rng.integers(20, 120)), rng, dup_pool=int(rng.integers(5, 60))) for _ in range(n_frames)]
    descs = _tables(ctx, pkg, rows, 0)
    fp = [(a, b) for a in range(n_frames) for b in range(n_frames)]
    fp = [fp[k] for k in rng.permutation(len(fp))]
    assert len(fp) > 1024
    got, res = batch.bf_select_pairs(ctx, descs, fp, True, 4.0, 500)
    _check(got, res, rows, fp, 0, True, 4.0, 500, {})


# ---- 4. graph capture, replayed twice -------------------------------------------------------------------------------------------
def test_graph_replay(ctx, pkg):
    import torch
    batch = _batch()
    rng = np.random.default_rng(17)
    rows = [_rows(1, n, rng) for n in (300, 513, 64, 1025)]
    descs = _tables(ctx, pkg, rows, 1)
    fp = [(0, 1), (1, 2), (3, 0), (2, 3)]
    recs = batch.bf_select_table(descs, fp)
    run = batch.BfSelect(ctx, descs, recs)
    run.run()
    ctx.synchronize()
    first = [a.tobytes() for a in run.results()]
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            run.run()
        for _ in range(2):
            run.d_out.zero_()
            run.d_res.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert [a.tobytes() for a in run.results()] == first
    finally:
        ctx.set_stream(None)
    got, _ = batch.bf_select_pairs(ctx, descs, fp)
    out = run.results()[0]
    for k in range(len(fp)):
        o = int(recs["match_off"][k])
        assert out[o:o + len(got[k])].tobytes() == got[k].tobytes()


# ---- 5. the one-shot call equals the batched call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_one_shot_equals_batched(ctx, pkg, kind):
    batch = _batch()
    rng = np.random.default_rng(23 + kind)
    rows = [_rows(kind, 700, rng, dup_pool=200), _rows(kind, 513, rng), _rows(kind, 0, rng)]
    descs = _tables(ctx, pkg, rows, kind)
    fp = [(0, 1), (1, 0)]
    for cross, coef, ms in ((True, 4.0, 500), (False, 1e30, 100), (True, 1.0, 1)):
        got, res = batch.bf_select_pairs(ctx, descs, fp, cross, coef, ms)
        for k, (a, b) in enumerate(fp):
            one, r1 = pkg.bruteForceMatch(rows[a], rows[b], kind, cross, coef, ms, detail=True)
            assert one.tobytes() == got[k].tobytes()
            assert r1.tobytes() == res[k].tobytes()
    types = importlib.import_module("sfm-gms_amd.types")
    with pytest.raises(types.GmsError) as e:
        pkg.bruteForceMatch(rows[0], rows[2], kind)
    assert e.value.code == -2


# ---- 6. detector rows of the 1080p fixture pair ------------------------------------------------------------------------------------
def test_detector_rows_1080p(ctx, pkg):
    batch = _batch()
    z = np.load(os.path.join(ROOT, "tests", "golden", "image_main_scenario_1080p.npz"))
    kps, rows = batch.detect_images(ctx, np.stack([z["left"], z["right"]]))
    assert min(len(r) for r in rows) > 100
    frames = batch.FrameTable(ctx, kps, [(1920, 1080)] * 2)
    descs = batch.DescriptorTable(ctx, frames, rows, 0)
    fp = [(0, 1), (1, 0)]
    cache = {}
    for cross in (True, False):
        got, res = batch.bf_select_pairs(ctx, descs, fp, cross, 4.0, 500)
        _check(got, res, rows, fp, 0, cross, 4.0, 500, cache)
        assert (res["n_out"] > 0).all()


# ---- 7. run_dataset(method="bf") through the two-view stage -----------------------------------------------------------------------
def test_run_dataset_bf_two_view(ctx, pkg, oracle):
    io = importlib.import_module("sfm-gms_amd.io")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    rng = np.random.default_rng(61)
    camera = (1400.0, 1380.0, 960.0, 540.0)
    n = 900
    ang = np.deg2rad(6.0)
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    t = np.array([-0.6, 0.02, 0.05])
    X = np.stack([rng.uniform(-2.2, 2.2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(4, 9, n)], axis=1)
    K = np.array([[camera[0], 0, camera[2]], [0, camera[1], camera[3]], [0, 0, 1.0]])
    frames, descs = [], []
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for v in range(3):
        P = (X @ np.linalg.matrix_power(R, v).T + v * t) @ K.T
        uv = (P[:, :2] / P[:, 2:3] + rng.normal(0, 0.3, (n, 2))).astype(np.float32)
        kp = np.zeros(n, pkg.KEYPOINT_DTYPE)
        kp["x"], kp["y"] = uv[:, 0], uv[:, 1]
        d = base.copy()
        flip = rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8) & \
            rng.integers(0, 256, (n, 32), dtype=np.uint8)  # about 1 bit in 8 flipped
        d ^= flip
        wrong = rng.uniform(size=n) < 0.25
        d[wrong] = rng.integers(0, 256, (int(wrong.sum()), 32), dtype=np.uint8)
        frames.append(kp)
        descs.append(d)
    pairs = np.zeros(3, pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [0, 1, 0], [1, 2, 2]
    ds = io.Dataset(frames, [(1920, 1080)] * 3, descs, pkg.GMS_DESC_HAMMING256, pairs=pairs, matches=np.zeros(0, pkg.DMATCH_DTYPE))
    r = pipeline.run_dataset(ctx, ds, method="bf", camera=camera)
    tv = r["two_view"]
    for i in range(3):
        a, b = int(pairs["frame_a"][i]), int(pairs["frame_b"][i])
        want, _, _, _ = bf_select_ref.bf_match_select(descs[a], descs[b], True)
        o, k = int(r["pairs"]["match_off"][i]), len(want)
        assert int(r["results"]["status"][i]) == 0 and int(r["results"]["n_inliers"][i]) == k
        assert r["out"][o:o + k].tobytes() == want.tobytes()
        _, w1, w2 = oracle.gather(frames[a], frames[b], want)
        assert int(tv["n_points"][i]) == k
        assert r["coords1"][o:o + k].tobytes() == w1.tobytes() and r["coords2"][o:o + k].tobytes() == w2.tobytes()
        ref = sfm_ref.two_view(w1, w2, camera, None, 0.7, 1.0)
        e = tv[i]
        assert ref["E"] is not None and int(e["status"]) == 0
        assert int(e["n_ransac"]) == ref["n_ransac"] and int(e["ransac_iters"]) == ref["iters"]
        assert np.abs(e["E"] - ref["E"]).max() < 1e-9 and np.abs(e["R"] - ref["R"]).max() < 1e-9 and np.abs(e["t"] - ref["t"]).max() < 1e-9
        assert int(e["n_pose"]) == ref["n_pose"] and np.array_equal(r["mask"][o:o + k], ref["mask"])
        assert abs(e["sum_sq_err1"] - ref["sum_sq_err1"]) <= 1e-8 * ref["sum_sq_err1"] + 1e-14
        assert abs(e["sum_sq_err2"] - ref["sum_sq_err2"]) <= 1e-8 * ref["sum_sq_err2"] + 1e-14
        assert (want["queryIdx"] == want["trainIdx"]).mean() > 0.9
