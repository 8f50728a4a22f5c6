"""-m gpu: LOGOS on resident frames (gms_logos_prepare_device / gms_logos_filter_device / gms_logos_words_device)
against the one-shot gms_logos_match, the reference DLL's fixture (tests/golden/refdll_logos.npz), the numpy restatements
tests/logos_ref.py and tests/logos_words_ref.py, and through the two-view consumer."""
import importlib
import os

import numpy as np
import pytest

import logos_ref
import logos_words_ref
from logos_gpu import GMS_ERR_BAD_ARG, GMS_ERR_CAPACITY, GMS_ERR_DOMAIN
from logos_gpu import device_run as _device_run, kp_records as _kp, oneshot as _oneshot, want_dmatch as _want_dmatch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("sfm-gms_amd")
Z = np.load(os.path.join(ROOT, "tests", "golden", "refdll_logos.npz"))
NAMES = sorted(k[: -len("_matches")] for k in Z.files if k.endswith("_matches"))


def _moved(kp, theta, scale, t):
    c, s = np.cos(theta), np.sin(theta)
    out = kp.copy()
    out[:, 0] = scale * (c * kp[:, 0] - s * kp[:, 1]) + t[0]
    out[:, 1] = scale * (s * kp[:, 0] + c * kp[:, 1]) + t[1]
    out[:, 2] = kp[:, 2] * scale
    out[:, 3] = np.mod(kp[:, 3] - np.degrees(theta), 360.0)
    return out.astype(np.float32)


def _sequence(seed, n_frames, n, n_words, noise=0.2, integer=False):
    """Seeded frames: each the previous one moved by a rotation and a scale, with label noise (a4 arrays and word arrays)."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 640, (n, 2)) if integer else rng.uniform(0, 640, (n, 2))
    a4 = np.concatenate([xy, rng.uniform(2, 20, (n, 1)), rng.uniform(0, 360, (n, 1))], 1).astype(np.float32)
    w = rng.integers(0, n_words, n)
    frames, words = [a4], [w]
    for _ in range(n_frames - 1):
        a4 = _moved(a4, rng.uniform(-0.6, 0.6), rng.uniform(0.8, 1.25), rng.uniform(-20, 20, 2))
        if integer:
            a4[:, :2] = np.round(a4[:, :2])
        w = w.copy()
        flip = rng.random(n) < noise
        w[flip] = rng.integers(0, n_words, int(flip.sum()))
        frames.append(a4)
        words.append(w)
    return frames, words


# ---- 1. every fixture case in one batch, each pair twice, shuffled --------------------------------------------------------------
def test_fixture_cases_in_one_batch(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    frames, words = [], []
    for name in NAMES:
        frames += [_kp(Z[name + "_kp1"]), _kp(Z[name + "_kp2"])]
        words += [Z[name + "_nn1"], Z[name + "_nn2"]]
    table = batch.LogosTable(ctx, frames, words, 50)
    order = np.random.default_rng(7).permutation(2 * len(NAMES)) % len(NAMES)
    got, lres = batch.logos_pairs(ctx, table, [(2 * c, 2 * c + 1) for c in order])
    for k, c in enumerate(order):
        name = NAMES[c]
        assert got[k].tobytes() == _want_dmatch(Z[name + "_matches"]).tobytes(), name
        _, want = _oneshot(frames[2 * c], frames[2 * c + 1], words[2 * c], words[2 * c + 1])
        assert lres[k].tobytes() == want.tobytes(), name


# ---- 2. a seeded sequence: (a, b), (b, a), (a, a) of shared frames ---------------------------------------------------------------
@pytest.mark.parametrize("seed,n,n_words,integer", [(1, 300, 20, False), (2, 2000, 50, True), (3, 5000, 100, False),
                                                     (4, 10000, 50, False), (5, 400, 1, False)])
def test_seeded_sequence_equals_oneshot(ctx, seed, n, n_words, integer):
    batch = importlib.import_module("sfm-gms_amd.batch")
    a4s, ws = _sequence(seed, 4, n, n_words, integer=integer)
    frames = [_kp(a) for a in a4s]
    table = batch.LogosTable(ctx, frames, ws, n_words)
    fp = [(0, 1), (1, 0), (1, 1), (2, 3), (3, 2), (0, 0), (3, 1)]
    got, lres = batch.logos_pairs(ctx, table, fp)
    total = 0
    for k, (a, b) in enumerate(fp):
        want, wres = _oneshot(frames[a], frames[b], ws[a], ws[b])
        assert got[k].tobytes() == want.tobytes(), (a, b)
        assert lres[k].tobytes() == wres.tobytes(), (a, b)
        total += len(want)
        if n <= 400:
            assert got[k].tobytes() == _want_dmatch(logos_ref.match(a4s[a], a4s[b], ws[a], ws[b])).tobytes()
    assert total > 0


# ---- 3. capacity: nothing written past or inside a pair that does not fit; neighbours exact; logos_pairs reruns ----------------
def test_capacity_overflow_writes_nothing(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    a4s, ws = _sequence(11, 3, 1500, 20)
    frames = [_kp(a) for a in a4s]
    table = batch.LogosTable(ctx, frames, ws, 20)
    want = [_oneshot(frames[a], frames[b], ws[a], ws[b]) for a, b in ((0, 1), (1, 2), (2, 0))]
    need = len(want[1][0])
    assert need > 10
    pairs = np.zeros(3, pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [0, 1, 2], [1, 2, 0]
    pairs["m"] = [len(want[0][0]), need - 1, len(want[2][0]) + 5]
    # a canary record between the ranges: pair 1's range ends one record before pair 2's starts
    pairs["match_off"] = [0, len(want[0][0]), len(want[0][0]) + need]
    out, lres, pres = _device_run(ctx, table, pairs, extra=4)
    assert lres["status"].tolist() == [0, GMS_ERR_CAPACITY, 0]
    assert int(lres["n_out"][1]) == need
    assert (lres["n_candidates"][1], lres["n_supported"][1], lres["peak_bin"][1]) == (
        want[1][1]["n_candidates"], want[1][1]["n_supported"], want[1][1]["peak_bin"])
    rec = out.view(pkg.DMATCH_DTYPE)
    for p in (0, 2):
        o = int(pairs["match_off"][p])
        assert rec[o:o + len(want[p][0])].tobytes() == want[p][0].tobytes()
        assert pres["n_inliers"][p] == len(want[p][0]) and pres["status"][p] == 0
    o1 = int(pairs["match_off"][1])
    assert (out[o1 * 16:(o1 + need) * 16] == 0x5A).all()     # pair 1's range and the canary record after it
    o2 = int(pairs["match_off"][2]) + len(want[2][0])
    assert (out[o2 * 16:] == 0x5A).all()                       # past pair 2's survivors
    assert pres["n_inliers"][1] == 0 and pres["status"][1] == GMS_ERR_CAPACITY
    assert (pres["best_scale"] == -1).all() and (pres["best_rot"] == -1).all()
    got, lres2 = batch.logos_pairs(ctx, table, [(0, 1), (1, 2), (2, 0)], capacity=[need, need - 1, 3])
    assert (lres2["status"] == 0).all()
    for k in range(3):
        assert got[k].tobytes() == want[k][0].tobytes()


# ---- 4. a word out of range marks its frame ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [20, -1])
def test_bad_word_marks_frame(ctx, bad):
    batch = importlib.import_module("sfm-gms_amd.batch")
    a4s, ws = _sequence(21, 4, 600, 20)
    ws[2] = ws[2].copy()
    ws[2][317] = bad
    frames = [_kp(a) for a in a4s]
    table = batch.LogosTable(ctx, frames, ws, 20)
    fp = [(0, 1), (1, 2), (2, 3), (3, 0), (2, 2), (1, 0)]
    got, lres = batch.logos_pairs(ctx, table, fp)
    for k, (a, b) in enumerate(fp):
        if 2 in (a, b):
            assert lres["status"][k] == GMS_ERR_DOMAIN and len(got[k]) == 0
        else:
            want, wres = _oneshot(frames[a], frames[b], ws[a], ws[b])
            assert lres[k].tobytes() == wres.tobytes() and got[k].tobytes() == want.tobytes()
    # a frame index out of range is a bad argument of that pair alone
    pairs = batch.logos_pair_table(table, [(0, 1), (0, 9)], capacity=2000)
    _, lres, pres = _device_run(ctx, table, pairs)
    assert lres["status"].tolist() == [0, GMS_ERR_BAD_ARG] and pres["status"].tolist() == [0, GMS_ERR_BAD_ARG]


# ---- 5. the filter is capturable, and a replay sees inputs changed in place ---------------------------------------------------
def test_filter_graph_capture(ctx):
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    a4s, ws = _sequence(31, 4, 3000, 50)
    frames = [_kp(a) for a in a4s]
    table = batch.LogosTable(ctx, frames, ws, 50)
    pairs = batch.logos_pair_table(table, [(0, 1), (1, 2), (2, 3), (3, 3)], capacity=6000)
    dev = table.device
    n = len(pairs)
    ws_bytes = ctx.logos_workspace_bytes(0, n, 3000)
    d_pairs = batch._to_dev(pairs, dev)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(int(pairs["m"].sum()) * 16, dtype=torch.uint8, device=dev)
    d_lres = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    ctx.set_stream(s.cuda_stream)
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            table.filter_device(d_pairs.data_ptr(), n, d_ws.data_ptr(), ws_bytes, d_out.data_ptr(), d_lres.data_ptr())
        # change the inputs in place: other keypoints / words in the same table, another pair order
        a4n, wn = _sequence(32, 4, 3000, 50)
        fresh = batch.LogosTable(ctx, [_kp(a) for a in a4n], wn, 50)
        table.d_table.copy_(fresh.d_table)
        pairs2 = pairs.copy()
        pairs2["frame_a"], pairs2["frame_b"] = [3, 2, 1, 0], [2, 1, 0, 0]
        d_pairs.copy_(batch._to_dev(pairs2, dev))
        d_out.zero_()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        rep_out, rep_res = d_out.cpu().numpy().copy(), d_lres.cpu().numpy().copy()
    finally:
        ctx.set_stream(None)
    eager_out, eager_res, _ = batch.logos_filter(ctx, fresh, pairs2)
    assert rep_res.tobytes() == eager_res.tobytes()
    assert rep_out.tobytes() == eager_out.tobytes()
    res = eager_res
    assert (res["status"] == 0).all() and res["n_out"].sum() > 0
    for k in range(n):
        a, b = int(pairs2["frame_a"][k]), int(pairs2["frame_b"][k])
        want, _ = _oneshot(_kp(a4n[a]), _kp(a4n[b]), wn[a], wn[b])
        o = int(pairs2["match_off"][k])
        assert eager_out[o:o + len(want)].tobytes() == want.tobytes()


# ---- 6. words: the exact nearest dictionary row -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,n_words", [(10000, 50), (10000, 100), (777, 1), (3000, 200)])
def test_words_l2(ctx, n_rows, n_words):
    batch = importlib.import_module("sfm-gms_amd.batch")
    rng = np.random.default_rng(n_rows + n_words)
    dic = rng.uniform(0, 60, (n_words, 128)).astype(np.float32)            # not integer-valued
    if n_words > 3:
        dic[n_words - 1] = dic[1]                                            # duplicated rows: the lower index must win
        dic[n_words - 2] = dic[0]
    desc = dic[rng.integers(0, n_words, n_rows)] + rng.normal(0, 8, (n_rows, 128)).astype(np.float32)
    desc[:50] = dic[1 % n_words]                                              # exact ties between rows 1 and n_words - 1
    # near-ties: half-way between two words, off by a few ulps
    mid = (dic[2 % n_words] + dic[3 % n_words]) * np.float32(0.5)
    desc[50:100] = mid + rng.integers(-3, 4, (50, 128)).astype(np.float32) * np.float32(1e-5)
    desc = desc.astype(np.float32)
    got = np.concatenate(batch.logos_words(ctx, [desc[:4000], desc[4000:]], dic, pkg.GMS_DESC_L2_F32X128))
    want = logos_words_ref.words(desc, dic, 1)
    assert got.tobytes() == want.tobytes()
    if n_words > 3:
        assert (got[:50] == 1).all()


@pytest.mark.parametrize("n_rows,n_words", [(10000, 50), (10000, 100), (500, 65)])
def test_words_hamming(ctx, n_rows, n_words):
    batch = importlib.import_module("sfm-gms_amd.batch")
    rng = np.random.default_rng(n_rows * 7 + n_words)
    dic = rng.integers(0, 256, (n_words, 32)).astype(np.uint8)
    dic[n_words - 1] = dic[4]
    desc = dic[rng.integers(0, n_words, n_rows)].copy()
    flips = rng.integers(0, 256, desc.shape).astype(np.uint8) & rng.integers(0, 256, desc.shape).astype(np.uint8) \
        & rng.integers(0, 256, desc.shape).astype(np.uint8)
    desc ^= flips
    desc[:20] = dic[4]
    got = batch.logos_words(ctx, desc, dic, pkg.GMS_DESC_HAMMING256)
    assert got.tobytes() == logos_words_ref.words(desc, dic, 0).tobytes()
    assert (got[:20] == 4).all()


# ---- 7. descriptors -> words -> LOGOS batch -> two-view, against the one-shot's survivors through the same consumer ----------
def test_chain_to_two_view(ctx):
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    io = importlib.import_module("sfm-gms_amd.io")
    rng = np.random.default_rng(41)
    n_words, n = 50, 2000
    dic = rng.uniform(0, 100, (n_words, 128)).astype(np.float32)
    a4s, true_words = _sequence(42, 4, n, n_words)
    descs = [(dic[w] + rng.normal(0, 5, (n, 128))).astype(np.float32) for w in true_words]
    frames = [_kp(a) for a in a4s]
    words = batch.logos_words(ctx, descs, dic, pkg.GMS_DESC_L2_F32X128)
    assert all(w.tobytes() == logos_words_ref.words(d, dic, 1).tobytes() for w, d in zip(words, descs))
    table = batch.LogosTable(ctx, frames, words, n_words)
    fp = [(0, 1), (1, 2), (2, 3)]
    pairs = batch.logos_pair_table(table, fp, capacity=4000)
    out, lres, pres = batch.logos_filter(ctx, table, pairs)
    assert (lres["status"] == 0).all() and (pres["n_inliers"] >= 5).all()
    # the one-shot's survivors at the same offsets, with the same per-pair records
    ref_out = np.zeros_like(out)
    for k, (a, b) in enumerate(fp):
        want, _ = _oneshot(frames[a], frames[b], words[a], words[b])
        ref_out[int(pairs["match_off"][k]):int(pairs["match_off"][k]) + len(want)] = want
    cam = pkg.types.make_camera((800.0, 800.0, 320.0, 240.0))

    def two_view(filtered):
        ft = batch.FrameTable(ctx, frames, [(640, 480)] * len(frames))
        dev = ft.device
        tot = len(filtered)
        d_pairs = batch._to_dev(pairs, dev)
        d_f = batch._to_dev(filtered, dev)
        d_res = batch._to_dev(pres, dev)
        d_c1 = torch.zeros(tot * 2, dtype=torch.float32, device=dev)
        d_c2 = torch.zeros(tot * 2, dtype=torch.float32, device=dev)
        d_mask = torch.zeros(tot, dtype=torch.uint8, device=dev)
        d_p3 = torch.zeros(tot * 3, dtype=torch.float64, device=dev)
        d_tv = torch.zeros(len(pairs) * pkg.types.TWO_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.two_view_batch_device(cam, ft.d_kp.data_ptr(), ft.d_frame_off.data_ptr(), ft.n_frames, d_pairs.data_ptr(), len(pairs),
                                  int(pairs["m"].max()), d_f.data_ptr(), d_res.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(),
                                  d_mask.data_ptr(), d_p3.data_ptr(), d_tv.data_ptr(), 0.7, 1.0, 1000)
        ctx.synchronize()
        return d_tv.cpu().numpy()

    tv = two_view(out)
    assert tv.tobytes() == two_view(ref_out).tobytes()
    # the same flow from a dataset
    ds = io.Dataset(frames, [(640, 480)] * len(frames), descs, pkg.GMS_DESC_L2_F32X128, pairs=pairs.copy(),
                    matches=np.zeros(0, pkg.DMATCH_DTYPE))
    r = pipeline.run_dataset(ctx, ds, method="logos", dictionary=dic, camera=(800.0, 800.0, 320.0, 240.0), logos_capacity=4000)
    assert r["logos_results"].tobytes() == lres.tobytes()
    assert r["out"].tobytes() == out.tobytes()
    assert r["two_view"].tobytes() == tv.tobytes()
    # a capacity too small for every pair: the pipeline reruns and gets the same survivors
    r2 = pipeline.run_dataset(ctx, ds, method="logos", dictionary=dic, logos_capacity=1)
    assert (r2["results"]["status"] == 0).all()
    for k in range(len(fp)):
        o, o2 = int(pairs["match_off"][k]), int(r2["pairs"]["match_off"][k])
        m = int(lres["n_out"][k])
        assert r2["out"][o2:o2 + m].tobytes() == out[o:o + m].tobytes()


# ---- 8. a batch of more than 1024 pairs (more pairs than the one-workgroup scans have threads) ---------------------------------
def test_more_than_1024_pairs(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    rng = np.random.default_rng(51)
    n_frames = 35
    a4s, ws = _sequence(52, n_frames, 90, 6)
    sizes = rng.integers(40, 91, n_frames)           # ragged frames: every pair has its own query count
    a4s = [a[:k] for a, k in zip(a4s, sizes)]
    ws = [w[:k] for w, k in zip(ws, sizes)]
    frames = [_kp(a) for a in a4s]
    table = batch.LogosTable(ctx, frames, ws, 6)
    fp = [(a, b) for a in range(n_frames) for b in range(n_frames)]
    order = rng.permutation(len(fp))
    fp = [fp[k] for k in order]
    assert len(fp) > 1024
    got, lres = batch.logos_pairs(ctx, table, fp)
    assert (lres["status"] == 0).all()
    cache = {}
    for k, (a, b) in enumerate(fp):
        if (a, b) not in cache:
            cache[(a, b)] = _oneshot(frames[a], frames[b], ws[a], ws[b])
        want, wres = cache[(a, b)]
        assert got[k].tobytes() == want.tobytes(), (a, b)
        assert lres[k].tobytes() == wres.tobytes(), (a, b)
    assert lres["n_out"].sum() > 0
    # the same batch on a workspace full of junk: the filter must not read any of it before writing it
    pairs = batch.logos_pair_table(table, fp, capacity=8100)
    out, lres2, pres = _device_run(ctx, table, pairs, ws_fill=0x3C)
    assert lres2.tobytes() == lres.tobytes()
    rec = out.view(pkg.DMATCH_DTYPE)
    for k in range(len(fp)):
        o = int(pairs["match_off"][k])
        assert rec[o:o + len(got[k])].tobytes() == got[k].tobytes()
        assert pres["n_inliers"][k] == len(got[k])
