"""-m gpu: the contract of the C ABI beyond "one call, right answer" -- reserved launches neither allocate nor synchronise
(they can be captured into a graph), a context survives stream changes and concurrent host threads, the host-pointer
batch entry, sliced large batches, the one-shot call's output tail, and BASELINE config 3's table at its stated size."""
import importlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_batch(oracle, frames, sizes, foff, pairs, matches, rot, scale, threads=8):
    kp_all = np.concatenate(frames)
    wh = np.asarray(sizes, dtype=np.int32).reshape(-1)
    failed, out, res, mask = oracle.batch(kp_all, foff, wh, pairs, matches, rot, scale, 6.0, threads)
    return failed, out, res, mask


def _same(pairs, out, res, wout, wres):
    assert res.tobytes() == wres.tobytes()
    for i in range(len(pairs)):
        o, k = int(pairs["match_off"][i]), int(res["n_inliers"][i])
        assert out[o:o + k].tobytes() == wout[o:o + k].tobytes(), i


def _sequence(pkg, synth, n_frames, n_kp, n_pairs, seed, size, ragged=True):
    from test_gpu_parity import _sequence_batch
    return _sequence_batch(pkg, synth, n_frames, n_kp, n_pairs, seed, ragged=ragged, size=size)


# ---- gms_ctx_reserve: a reserved launch is nothing but launches -> it can be captured and replayed ----------------
@pytest.mark.parametrize("rot,scale,n_kp", [(False, False, 3000), (True, True, 3000), (False, False, 20000), (True, True, 20000)])
def test_reserved_launch_is_capturable(pkg, oracle, synth, rot, scale, n_kp):
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    size = (1280, 720)
    frames, pairs, matches = _sequence(pkg, synth, 6, n_kp, 12, 91, size)
    with pkg.GmsContext(0) as ctx:
        table = batch.FrameTable(ctx, frames, [size] * len(frames))
        dev = table.device
        d_pairs = batch._to_dev(pairs, dev)
        d_matches = batch._to_dev(matches, dev)
        d_out = torch.zeros(len(matches) * 16, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(len(pairs) * 16, dtype=torch.uint8, device=dev)
        max_m = int(pairs["m"].max())
        s = torch.cuda.Stream(device=dev)
        ctx.set_stream(s.cuda_stream)

        def launch():
            ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), table.n_frames, d_pairs.data_ptr(),
                              len(pairs), max_m, d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, rot, scale, 6.0)

        needs_ws = scale or n_kp > 16384
        if needs_ws:
            # not reserved: growing a workspace inside a capture is refused, loudly, and the capture survives it
            g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g0, stream=s):
                with pytest.raises(pkg.GmsError) as e:
                    launch()
                assert e.value.code == -6
        ctx.reserve(len(pairs), max_m, rot, scale)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):   # any allocation or synchronisation inside would fail the capture
            launch()
        d_out.zero_()
        d_res.zero_()
        g.replay()
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(pkg.DMATCH_DTYPE)
        res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE)
        ctx.set_stream(None)
    failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * len(frames), table.frame_off_host, pairs, matches, rot, scale)
    assert failed == 0
    _same(pairs, out, res, wout, wres)


# ---- one context, two streams, workspaces in use on both ------------------------------------------------------------------
def test_stream_switch_with_work_in_flight(pkg, oracle, synth):
    """Launches that share the context's workspaces (scale hypotheses: one record per pair) alternate between two streams
    without any host synchronisation in between; each must see its own records."""
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    size = (1280, 720)
    sets = [_sequence(pkg, synth, 5, 4000, 48, 200 + i, size) for i in range(2)]
    with pkg.GmsContext(0) as ctx:
        tabs, bufs = [], []
        for frames, pairs, matches in sets:
            t = batch.FrameTable(ctx, frames, [size] * len(frames))
            dev = t.device
            tabs.append(t)
            bufs.append((batch._to_dev(pairs, dev), batch._to_dev(matches, dev),
                         torch.zeros(len(matches) * 16, dtype=torch.uint8, device=dev),
                         torch.zeros(len(pairs) * 16, dtype=torch.uint8, device=dev)))
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        torch.cuda.synchronize()
        for rep in range(6):
            i = rep & 1
            ctx.set_stream(streams[i].cuda_stream)
            pairs = sets[i][1]
            dp, dm, do, dr = bufs[i]
            ctx.filter_device(tabs[i].d_pts.data_ptr(), tabs[i].d_frame_off.data_ptr(), tabs[i].n_frames, dp.data_ptr(),
                              len(pairs), int(pairs["m"].max()), dm.data_ptr(), do.data_ptr(), dr.data_ptr(), None, True, True, 6.0)
        torch.cuda.synchronize()
        ctx.set_stream(None)
        for i, (frames, pairs, matches) in enumerate(sets):
            out = bufs[i][2].cpu().numpy().view(pkg.DMATCH_DTYPE)
            res = bufs[i][3].cpu().numpy().view(pkg.RESULT_DTYPE)
            failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * len(frames), tabs[i].frame_off_host, pairs, matches, True, True)
            assert failed == 0
            _same(pairs, out, res, wout, wres)


def test_one_context_many_host_threads(ctx, oracle):
    """INTEGRATION.md calls a context thread-safe: one-shot calls from several threads, all flag combinations."""
    work = [(cases.random_pair(300 + i, n=2500 + 700 * i, inlier_frac=0.5), i & 1 == 1, i & 2 == 2) for i in range(8)]
    want = [oracle.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], r, s, 6.0)[1] for c, r, s in work]
    got, errs = [None] * len(work), []

    def run(i):
        try:
            for _ in range(5):
                c, r, s = work[i]
                got[i] = ctx.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], r, s, 6.0)
                assert got[i].tobytes() == want[i].tobytes()
        except Exception as e:  # noqa: BLE001
            errs.append((i, repr(e)))

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(work))]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errs, errs


# ---- the one-shot call leaves the caller's array alone beyond *n_out ---------------------------------------------------
def test_one_shot_output_tail_is_untouched(pkg, oracle):
    import ctypes as C
    lib = pkg.load_library()
    sentinel = np.zeros(1, dtype=pkg.DMATCH_DTYPE)
    sentinel["queryIdx"], sentinel["trainIdx"], sentinel["imgIdx"], sentinel["distance"] = -7, -8, -9, -1.5
    for n, rot in ((1500, False), (1500, True), (12000, False)):
        # a larger call first, so that the library's own buffers hold survivors of another call
        big = cases.random_pair(400, n=n + 500, inlier_frac=0.9)
        pkg.matchGMS(big["size1"], big["size2"], big["kp1"], big["kp2"], big["matches"])
        c = cases.random_pair(401 + n, n=n, inlier_frac=0.3)
        out = np.repeat(sentinel, n)
        n_out = C.c_int(-1)
        rc = lib.gms_match(c["kp1"].ctypes.data, n, *c["size1"], c["kp2"].ctypes.data, n, *c["size2"], c["matches"].ctypes.data, n,
                           int(rot), 0, 6.0, out.ctypes.data, C.byref(n_out))
        assert rc == 0
        want = oracle.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], rot, False, 6.0)[1]
        assert n_out.value == len(want) and out[:n_out.value].tobytes() == want.tobytes()
        assert out[n_out.value:].tobytes() == np.repeat(sentinel, n - n_out.value).tobytes()
    # an error leaves everything alone and reports zero survivors
    bad = cases.domain_error_cases()["train_oob"]
    n = len(bad["matches"])
    out = np.repeat(sentinel, n)
    n_out = C.c_int(-1)
    rc = lib.gms_match(bad["kp1"].ctypes.data, len(bad["kp1"]), *bad["size1"], bad["kp2"].ctypes.data, len(bad["kp2"]), *bad["size2"],
                       bad["matches"].ctypes.data, n, 0, 0, 6.0, out.ctypes.data, C.byref(n_out))
    assert rc == -2 and n_out.value == 0 and out.tobytes() == np.repeat(sentinel, n).tobytes()


# ---- gms_filter_host_batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot,scale", [(False, False), (True, True)])
def test_host_batch_matches_the_oracle(ctx, pkg, oracle, synth, rot, scale):
    size = (1280, 720)
    frames, pairs, matches = _sequence(pkg, synth, 8, 5000, 900, 55, size)   # ~2.2 M matches: two chunks at least
    pairs["m"][17] = 0
    out, res = ctx.filter_host_batch(frames, [size] * len(frames), pairs, matches, rot, scale, 6.0)
    counts = np.array([len(f) for f in frames])
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * len(frames), foff, pairs, matches, rot, scale)
    assert failed == 0
    _same(pairs, out, res, wout, wres)


def test_host_batch_mixed_sizes_and_a_bad_pair(ctx, pkg, oracle, synth):
    """Small and large pairs in one list (every chunk picks its own kernel family), pairs out of order in the match array,
    one pair outside the parity domain."""
    size = (1920, 1080)
    frames = synth.make_sequence(77, 4, size=size, n_kp=30000)
    rng = np.random.default_rng(9)
    ms = [30000, 100, 9000, 0, 30000, 2000, 17000, 5]
    blocks = [synth.sequence_matches(7000 + i, 30000, 30000, 0.5)[:m] for i, m in enumerate(ms)]
    order = rng.permutation(len(ms))
    offs, off = {}, 0
    for i in order:   # blocks laid out in a shuffled order
        offs[i] = off
        off += ms[i]
    matches = np.zeros(off, dtype=pkg.DMATCH_DTYPE)
    pairs = np.zeros(len(ms), dtype=pkg.PAIR_DTYPE)
    for i, m in enumerate(ms):
        matches[offs[i]:offs[i] + m] = blocks[i]
        pairs[i] = (i % 3, 3, m, 0, offs[i])
    matches["trainIdx"][offs[5] + 3] = 10 ** 6
    out, res = ctx.filter_host_batch(frames, [size] * 4, pairs, matches, False, False, 6.0)
    foff = np.arange(5, dtype=np.int64) * 30000
    failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * 4, foff, pairs, matches, False, False)
    assert failed == 1 and res["status"].tolist() == [0, 0, 0, 0, 0, -2, 0, 0]
    _same(pairs, out, res, wout, wres)


# ---- gms_filter_host_batch over many chunks: lanes reused (chunk k rides lane k % 3), the tail iterations of a long list ------------
_CHUNK_MATCHES, _CHUNK_PAIRS = 2 << 20, 8192   # the cut of gms_filter_host_batch (gms_capi.cpp: kChunkMatches, kChunkPairs)


def _host_chunks(m):
    """The chunks gms_filter_host_batch cuts a pair list into, by its rule: runs of consecutive pairs, at most _CHUNK_PAIRS pairs and
    _CHUNK_MATCHES matches (a larger pair alone). [(first pair, pairs, matches)]."""
    chunks, i, m = [], 0, [int(v) for v in m]
    while i < len(m):
        first, total = i, 0
        while i < len(m) and i - first < _CHUNK_PAIRS and (i == first or total + m[i] <= _CHUNK_MATCHES):
            total += m[i]
            i += 1
        chunks.append((first, i - first, total))
    return chunks


def _lay_out(pkg, ms, blocks, rng):
    """Pair i's match block (a window of blocks[i % len(blocks)]) placed in a shuffled order in the match array."""
    offs, off = np.zeros(len(ms), dtype=np.int64), 0
    for i in rng.permutation(len(ms)):
        offs[i] = off
        off += ms[i]
    matches = np.zeros(off, dtype=pkg.DMATCH_DTYPE)
    for i, m in enumerate(ms):
        b = blocks[i % len(blocks)]
        s = int(rng.integers(0, len(b) - m + 1))
        matches[offs[i]:offs[i] + m] = b[s:s + m]
    return offs, matches


def _fill(rng, total, lo=3000, hi=20000):
    """Ragged pair sizes in [lo, hi] (a remainder above lo / 2) that add up to exactly `total`."""
    ms = []
    while total > hi + lo:
        ms.append(int(rng.integers(lo, hi + 1)))
        total -= ms[-1]
    return ms + ([total // 2, total - total // 2] if total > hi else [total])


@pytest.fixture(scope="module")
def long_list(pkg, synth, oracle):
    """Default flags, 1280 x 720 frames of 20 000 keypoints, about 12.6 M matches in seven chunks cut by match count. Pair 0 is empty
    (it opens chunk 0), chunk 1 holds exactly _CHUNK_MATCHES (the inclusive edge of the cut), a pair of chunk 4 -- lane 1, second
    use -- is outside the parity domain, the last chunk holds one small pair and the empty last pair; match blocks in shuffled
    order (the host's overlap check sorts). The oracle's answer once for the module."""
    size, n_kp, n_frames = (1280, 720), 20000, 8
    frames = synth.make_sequence(61, n_frames, size=size, n_kp=n_kp)
    rng = np.random.default_rng(61)
    chunk_ms = [[0] + _fill(rng, _CHUNK_MATCHES - 5000),
                [n_kp] + _fill(rng, _CHUNK_MATCHES - n_kp),
                [n_kp] + [1, 2, 5] + _fill(rng, _CHUNK_MATCHES - n_kp - 8 - 777),
                [n_kp] + _fill(rng, _CHUNK_MATCHES - n_kp - 3000),
                [n_kp] + _fill(rng, _CHUNK_MATCHES - n_kp - 12000),
                [n_kp] + _fill(rng, _CHUNK_MATCHES - n_kp - 20),
                [37, 0]]
    ms = [m for c in chunk_ms for m in c]
    blocks = [synth.sequence_matches(6100 + j, n_kp, n_kp, 0.5) for j in range(5)]
    offs, matches = _lay_out(pkg, ms, blocks, rng)
    pairs = np.zeros(len(ms), dtype=pkg.PAIR_DTYPE)
    for i, m in enumerate(ms):
        a = i % (n_frames - 1)
        pairs[i] = (a, min(a + 1 + (i // 7) % 2, n_frames - 1), m, 0, offs[i])
    chunks = _host_chunks(pairs["m"])
    bad = chunks[4][0] + 3
    matches["trainIdx"][offs[bad] + 2] = 10 ** 6
    foff = np.arange(n_frames + 1, dtype=np.int64) * n_kp
    failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * n_frames, foff, pairs, matches, False, False)
    return dict(frames=frames, size=size, foff=foff, pairs=pairs, matches=matches, chunks=chunks, bad=bad, failed=failed, wout=wout,
                wres=wres)


def test_host_batch_long_list_across_chunks(ctx, pkg, long_list):
    L = long_list
    pairs, chunks = L["pairs"], L["chunks"]
    # the layout the test is about, by the library's own rule
    assert len(chunks) == 7 and all(n < _CHUNK_PAIRS for _, n, _ in chunks)            # cut by match count, lanes 0 1 2 0 1 2 0
    assert chunks[1][2] == _CHUNK_MATCHES                                                # the inclusive edge
    assert pairs["m"][0] == 0 and pairs["m"][-1] == 0 and chunks[-1][1:] == (2, 37)
    assert len(pairs) > 600 and len(L["matches"]) > 12_000_000 and (np.diff(pairs["match_off"]) < 0).any()
    assert [i for i, (f, n, _) in enumerate(chunks) if f <= L["bad"] < f + n] == [4]
    assert L["failed"] == 1 and np.flatnonzero(L["wres"]["status"]).tolist() == [L["bad"]] and L["wres"]["status"][L["bad"]] == -2
    assert (L["wres"]["n_inliers"] > 0).sum() > 600
    out, res = ctx.filter_host_batch(L["frames"], [L["size"]] * len(L["frames"]), pairs, L["matches"], False, False, 6.0)
    _same(pairs, out, res, L["wout"], L["wres"])


def _oracle_subset(oracle, frames, sizes, foff, pairs, matches, idx, rot, scale):
    """The oracle on pairs[idx] alone (their match blocks gathered back to back): (failed, out, results, the blocks' offsets)."""
    sel = pairs[idx].copy()
    sel["match_off"] = np.concatenate([[0], np.cumsum(sel["m"])[:-1]])
    m = np.concatenate([matches[o:o + k] for o, k in zip(pairs["match_off"][idx], pairs["m"][idx])])
    failed, wout, wres, _ = _oracle_batch(oracle, frames, sizes, foff, sel, m, rot, scale)
    return failed, wout, wres, sel["match_off"]


def test_host_batch_pair_count_cut_with_rotation_and_scale(ctx, pkg, oracle, synth):
    """More than 5 x 8192 pairs of a few dozen matches (every 64th pair 1000): six chunks cut by pair count, empty pairs that open
    chunks 1 and 2, a pair outside the parity domain in chunk 4, rotation + scale hypotheses. Every pair against the device-resident
    entry (one launch over the whole list, no chunks, no staging), and a thousand of them -- both sides of every chunk border,
    the bad pair's neighbours, the tail, a spread sample -- against the oracle (all 42 k: minutes of CPU)."""
    batch = importlib.import_module("sfm-gms_amd.batch")
    size, n_kp, n_frames = (1280, 720), 3000, 6
    frames = synth.make_sequence(62, n_frames, size=size, n_kp=n_kp)
    rng = np.random.default_rng(62)
    n_pairs = 5 * _CHUNK_PAIRS + 1234
    ms = rng.integers(20, 81, n_pairs)
    ms[::64] = 1000
    ms[[_CHUNK_PAIRS, 2 * _CHUNK_PAIRS]] = 0
    blocks = [synth.sequence_matches(6200 + j, n_kp, n_kp, 0.6) for j in range(7)]
    offs, matches = _lay_out(pkg, ms, blocks, rng)
    pairs = np.zeros(n_pairs, dtype=pkg.PAIR_DTYPE)
    a = np.arange(n_pairs) % (n_frames - 1)
    pairs["frame_a"], pairs["frame_b"], pairs["m"], pairs["match_off"] = a, a + 1, ms, offs
    chunks = _host_chunks(ms)
    assert len(chunks) == 6 and [n for _, n, _ in chunks] == [_CHUNK_PAIRS] * 5 + [1234]
    assert all(t < _CHUNK_MATCHES for _, _, t in chunks) and 2_000_000 < len(matches) < 3_000_000
    bad = 4 * _CHUNK_PAIRS + 100
    matches["trainIdx"][offs[bad] + 1] = n_kp
    out, res = ctx.filter_host_batch(frames, [size] * n_frames, pairs, matches, True, True, 6.0)
    assert res["status"][bad] == -2 and (np.flatnonzero(res["status"]) == [bad]).all() and (res["n_inliers"] > 0).sum() > 20000

    table = batch.FrameTable(ctx, frames, [size] * n_frames)
    dout, dres, _ = batch.filter_pairs(ctx, table, pairs, matches, True, True, 6.0, want_mask=False)
    _same(pairs, out, res, dout, dres)

    near = [i for c in range(1, 6) for i in range(c * _CHUNK_PAIRS - 40, c * _CHUNK_PAIRS + 40)]
    idx = np.unique(np.r_[near, np.arange(bad - 30, bad + 30), np.arange(n_pairs - 60, n_pairs), np.arange(0, n_pairs, 64)[::4],
                          rng.choice(n_pairs, 300, replace=False)])
    failed, wout, wres, woff = _oracle_subset(oracle, frames, [size] * n_frames, table.frame_off_host, pairs, matches, idx, True, True)
    assert failed == 1 and len(idx) > 900
    assert res[idx].tobytes() == wres.tobytes()
    for j, i in enumerate(idx):
        o, k = int(pairs["match_off"][i]), int(res["n_inliers"][i])
        assert out[o:o + k].tobytes() == wout[woff[j]:woff[j] + k].tobytes(), i


def test_host_batch_tuple_form_reuses_the_callers_arrays(ctx, pkg, oracle, synth, long_list):
    """(kp_all, frame_off) three times into the same caller-owned out / results, prefilled with a sentinel record: the long list,
    a short list of other matches with rotation + scale (on a prefix of the frame table), the long list again. Each call gives
    the oracle's bytes; the first leaves every record it does not own -- behind each pair's survivors, beyond the pairs -- alone."""
    L = long_list
    frames, pairs, matches = L["frames"], L["pairs"], L["matches"]
    kp_all, foff, n_frames = np.concatenate(frames), L["foff"], len(frames)
    sentinel = np.zeros(1, dtype=pkg.DMATCH_DTYPE)
    sentinel["queryIdx"], sentinel["trainIdx"], sentinel["imgIdx"], sentinel["distance"] = -7, -8, -9, -1.5
    rsent = np.zeros(1, dtype=pkg.RESULT_DTYPE)
    rsent["n_inliers"], rsent["best_scale"], rsent["best_rot"], rsent["status"] = -11, -12, -13, -14
    out = np.repeat(sentinel, len(matches) + 1000)
    results = np.repeat(rsent, len(pairs) + 50)

    o, r = ctx.filter_host_batch((kp_all, foff), [L["size"]] * n_frames, pairs, matches, False, False, 6.0, out=out, results=results)
    assert np.shares_memory(o, out) and np.shares_memory(r, results)
    _same(pairs, out, results[:len(pairs)], L["wout"], L["wres"])
    written = np.zeros(len(out), dtype=bool)
    for off, k in zip(pairs["match_off"], results["n_inliers"][:len(pairs)]):
        written[off:off + k] = True
    rows = out.view(np.uint8).reshape(-1, 16)
    assert (rows[~written] == np.frombuffer(sentinel.tobytes(), np.uint8)).all()
    assert results[len(pairs):].tobytes() == np.repeat(rsent, 50).tobytes()

    # a short list: two chunks, other matches, rotation + scale, the first five frames of the same table (a prefix: legal)
    use, n_kp = 5, len(frames[0])
    rng = np.random.default_rng(63)
    ms2 = [int(v) for v in rng.integers(2000, n_kp + 1, 200)]
    blocks = [synth.sequence_matches(6300 + j, n_kp, n_kp, 0.6) for j in range(3)]
    offs2, matches2 = _lay_out(pkg, ms2, blocks, rng)
    pairs2 = np.zeros(len(ms2), dtype=pkg.PAIR_DTYPE)
    for i, m in enumerate(ms2):
        pairs2[i] = (i % (use - 1), i % (use - 1) + 1, m, 0, offs2[i])
    assert len(_host_chunks(ms2)) == 2
    failed, wout2, wres2, _ = _oracle_batch(oracle, frames[:use], [L["size"]] * use, foff[:use + 1], pairs2, matches2, True, True)
    assert failed == 0 and (wres2["n_inliers"] > 0).mean() > 0.9
    ctx.filter_host_batch((kp_all, foff[:use + 1]), [L["size"]] * use, pairs2, matches2, True, True, 6.0, out=out, results=results)
    _same(pairs2, out, results[:len(pairs2)], wout2, wres2)

    ctx.filter_host_batch((kp_all, foff), [L["size"]] * n_frames, pairs, matches, False, False, 6.0, out=out, results=results)
    _same(pairs, out, results[:len(pairs)], L["wout"], L["wres"])
    assert results[len(pairs):].tobytes() == np.repeat(rsent, 50).tobytes()


def test_host_batch_frame_off_is_validated(ctx, pkg, synth):
    """The tuple form's frame table: ValueError for offsets that decrease, do not start at 0, run past the keypoints or miss a frame.
    The C entry refuses the first two itself (GMS_ERR_BAD_ARG) before it copies or launches anything, results untouched."""
    size = (640, 480)
    frames, pairs, matches = _sequence(pkg, synth, 3, 500, 4, 64, size, ragged=False)
    kp_all = np.concatenate(frames)
    for foff in ([0, 600, 400, 1500], [5, 500, 1000, 1500], [0, 500, 1000, 1501], [0, 500, 1500], [0, 500, 1000, 1500, 1500]):
        with pytest.raises(ValueError):
            ctx.filter_host_batch((kp_all, np.array(foff)), [size] * 3, pairs, matches, False, False, 6.0)
    out, res = ctx.filter_host_batch((kp_all, np.array([0, 500, 1000, 1500])), [size] * 3, pairs, matches, False, False, 6.0)
    assert (res["status"] == 0).all() and res["n_inliers"].sum() > 0
    lib = pkg.load_library()
    wh = np.array([size] * 3, dtype=np.int32)
    for foff in ([0, 600, 400, 1500], [5, 500, 1000, 1500]):
        foff = np.array(foff, dtype=np.int64)
        out = np.zeros(len(matches), dtype=pkg.DMATCH_DTYPE)
        results = np.full(len(pairs) * 4, -5, dtype=np.int32).view(pkg.RESULT_DTYPE)
        before = results.tobytes()
        rc = lib.gms_filter_host_batch(ctx._h, kp_all.ctypes.data, foff.ctypes.data, wh.ctypes.data, 3, pairs.ctypes.data, len(pairs),
                                       matches.ctypes.data, 0, 0, 6.0, out.ctypes.data, results.ctypes.data)
        assert rc == -1 and results.tobytes() == before and not out.view(np.uint8).any()


# ---- large batches filtered in slices of the workspace budget (GMS_BAND_WS_BYTES is read once per process) ----------------
_SLICE_WORKER = r'''
import importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/oracle")
import gms_oracle
pkg = importlib.import_module("sfm-gms_amd"); synth = importlib.import_module("sfm-gms_amd.synth")
batch = importlib.import_module("sfm-gms_amd.batch")
from test_gpu_parity import _sequence_batch
size = (1920, 1080)
for rot, scale in ((False, False), (True, True)):
    frames, pairs, matches = _sequence_batch(pkg, synth, 4, 20000, 11, 5 + rot, ragged=False, size=size)
    # ragged sizes, full-size pairs on both sides of the slice borders (ranges stay disjoint: only m shrinks)
    pairs["m"] = [20000, 16385, 49, 17000, 20000, 18000, 16500, 20000, 20000, 500, 19999]
    matches = matches.copy()
    matches["trainIdx"][int(pairs["match_off"][3]) + 1] = 1 << 30   # a domain error next to a border
    with pkg.GmsContext(0) as ctx:
        table = batch.FrameTable(ctx, frames, [size] * 4)
        out, res, mask = batch.filter_pairs(ctx, table, pairs, matches, rot, scale, 6.0)
    kp_all = np.concatenate(frames); wh = np.array([size] * 4, dtype=np.int32).reshape(-1)
    failed, wout, wres, wmask = gms_oracle.batch(kp_all, table.frame_off_host, wh, pairs, matches, rot, scale, 6.0, 8)
    assert failed == 1 and res.tobytes() == wres.tobytes(), (res, wres)
    for i in range(len(pairs)):
        o, k = int(pairs["match_off"][i]), int(res["n_inliers"][i])
        assert out[o:o + k].tobytes() == wout[o:o + k].tobytes(), i
        if res["status"][i] == 0:
            assert np.array_equal(mask[o:o + int(pairs["m"][i])], wmask[o:o + int(pairs["m"][i])]), i
print("slices ok")
'''


def test_large_batch_in_forced_slices(tmp_path):
    script = tmp_path / "slices.py"
    script.write_text(_SLICE_WORKER)
    # 2 MB of workspace: 3 pairs per slice under the default flags (four slices of 11 pairs), 1 with rotation + scale
    res = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, GMS_BAND_WS_BYTES=str(2 << 20)))
    assert res.returncode == 0 and "slices ok" in res.stdout, res.stderr[-3000:]


# ---- BASELINE config 3 at its stated size: the 1000-frame table (80 MB, beyond the L2s), chunks of the real pair list -----
def test_config3_thousand_frame_table_two_chunks(ctx, pkg, oracle, synth):
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    d = importlib.import_module("sfm-gms_amd.dist")
    size, n_frames, n_kp, per_chunk = (1920, 1080), 1000, 10000, 1024
    frames = synth.make_sequence(1000, n_frames, size=size, n_kp=n_kp)
    table = batch.FrameTable(ctx, frames, [size] * n_frames)
    assert table.d_pts.numel() * 4 == 160_000_032 and table.total * 8 == 80_000_000   # points: 80 MB, beyond the L2s
    dev = table.device
    kp_all = np.concatenate(frames)
    wh = np.array([size] * n_frames, dtype=np.int32).reshape(-1)
    # rank 5 of 8: its block of the global list, first two chunks; plus the very last pairs of the list
    plan = d.RankPlan(n_frames, n_kp, per_chunk, 2, 5, 8)
    firsts = plan.starts + [plan.total_pairs - per_chunk]
    for first in firsts:
        pairs = d.pair_table(n_frames, first, first + per_chunk, n_kp)
        d_matches = d.synth_matches_device(first, per_chunk, n_kp, 0.5, dev)
        d_pairs = batch._to_dev(pairs, dev)
        d_out = torch.zeros((per_chunk * n_kp, 4), dtype=torch.int32, device=dev)
        d_res = torch.zeros((per_chunk, 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), n_frames, d_pairs.data_ptr(), per_chunk, n_kp,
                          d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, False, False, 6.0)
        ctx.synchronize()
        res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
        assert (res["status"] == 0).all() and (res["n_inliers"] > 2000).all()
        # every 97th pair of the chunk (and the global parity sample, where the chunk holds one) against the oracle
        idx = sorted(set(range(0, per_chunk, 97)) | {k - first for k in d.parity_sample(first, per_chunk)})
        sel = pairs[idx].copy()
        sel["match_off"] = np.arange(len(idx), dtype=np.int64) * n_kp
        m = np.concatenate([d.synth_matches_host(first + j, n_kp, 0.5) for j in idx])   # the host form of the same matches
        got_m = np.concatenate([d_matches[j * n_kp:(j + 1) * n_kp].cpu().numpy() for j in idx])
        assert got_m.view(np.uint8).tobytes() == m.tobytes()
        failed, wout, wres, _ = oracle.batch(kp_all, table.frame_off_host, wh, sel, m, False, False, 6.0, 8)
        assert failed == 0
        for t, j in enumerate(idx):
            assert res[j].tobytes() == wres[t].tobytes()
            k = int(res["n_inliers"][j])
            got = d_out[j * n_kp:j * n_kp + k].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
            assert got.tobytes() == wout[t * n_kp:t * n_kp + k].tobytes()
        del d_matches, d_out, d_res, d_pairs


# ---- the frame table describes itself: any subset of its frames may be named by a filter call ------------------------------
@pytest.mark.parametrize("rot,scale", [(False, False), (True, True)])
def test_filter_with_a_prefix_of_the_frame_table(pkg, oracle, synth, rot, scale):
    """gms_filter_device with n_frames smaller than the table was built for (and with an offsets array of its own): the kernels
    read where the code arrays lie from the table's header, not from frame_off[n_frames]. Before the header existed this read
    later frames' points as cell codes and returned wrong inliers without any error."""
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    size = (1280, 720)
    frames, pairs, matches = _sequence(pkg, synth, 8, 2500, 10, 93, size)
    use = 5                                                     # the call names frames 0..4 only
    keep = (pairs["frame_a"] < use) & (pairs["frame_b"] < use)
    pairs = pairs[keep]
    assert len(pairs) >= 3
    with pkg.GmsContext(0) as ctx:
        table = batch.FrameTable(ctx, frames, [size] * len(frames))
        dev = table.device
        d_foff = torch.from_numpy(table.frame_off_host[:use + 1].copy()).to(dev)
        d_pairs, d_matches = batch._to_dev(pairs, dev), batch._to_dev(matches, dev)
        d_out = torch.zeros(len(matches) * 16, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(len(pairs) * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.filter_device(table.d_pts.data_ptr(), d_foff.data_ptr(), use, d_pairs.data_ptr(), len(pairs), int(pairs["m"].max()),
                          d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, rot, scale, 6.0)
        ctx.synchronize()
        out, res = d_out.cpu().numpy().view(pkg.DMATCH_DTYPE), d_res.cpu().numpy().view(pkg.RESULT_DTYPE)
        # a block that carries the points but no header (a caller's own copy of the points, say): filtered from the points alone
        bare = table.d_pts.clone()
        bare[:4] = 0
        d_out2, d_res2 = torch.zeros_like(d_out), torch.zeros_like(d_res)
        torch.cuda.synchronize()
        ctx.filter_device(bare.data_ptr(), d_foff.data_ptr(), use, d_pairs.data_ptr(), len(pairs), int(pairs["m"].max()),
                          d_matches.data_ptr(), d_out2.data_ptr(), d_res2.data_ptr(), None, rot, scale, 6.0)
        ctx.synchronize()
        out2, res2 = d_out2.cpu().numpy().view(pkg.DMATCH_DTYPE), d_res2.cpu().numpy().view(pkg.RESULT_DTYPE)
    failed, wout, wres, _ = _oracle_batch(oracle, frames[:use], [size] * use, table.frame_off_host[:use + 1], pairs, matches, rot, scale)
    assert failed == 0 and wres["n_inliers"].sum() > 0
    _same(pairs, out, res, wout, wres)
    _same(pairs, out2, res2, wout, wres)


# ---- overlapping match ranges are refused (round 2's api.log: silently different counts on the large-pair path) -----------
def test_overlapping_match_ranges_are_flagged(pkg, oracle, synth):
    """Pairs own disjoint ranges [match_off, match_off + m) of the match / output arrays (include/gms.h). The device check runs behind
    the first launch of a context: every pair that overlaps another gets GMS_ERR_BAD_ARG, the others keep their results. In order
    (each range ending inside the next) and out of order (the table shuffled). The host-batch entry refuses the call."""
    import torch
    batch = importlib.import_module("sfm-gms_amd.batch")
    size = (1280, 720)
    for n_kp, shuffled in ((20000, False), (3000, True), (3000, False)):
        frames, pairs, matches = _sequence(pkg, synth, 6, n_kp, 12, 95, size, ragged=False)
        pairs = pairs.copy()
        pairs["match_off"][5] -= n_kp // 2        # pair 5 now starts inside pair 4's range
        pairs["m"][8] = 0                          # an empty pair overlaps nothing ...
        pairs["match_off"][8] = pairs["match_off"][2] + 7   # ... wherever it points
        order = np.random.default_rng(3).permutation(len(pairs)) if shuffled else np.arange(len(pairs))
        tab = pairs[order]
        want_bad = np.isin(order, [4, 5])
        with pkg.GmsContext(0) as ctx:             # a fresh context: its first launch is a checked one
            table = batch.FrameTable(ctx, frames, [size] * len(frames))
            out, res, _ = batch.filter_pairs(ctx, table, tab, matches, False, False, 6.0, want_mask=False)
            assert np.array_equal(res["status"] == -1, want_bad), (n_kp, shuffled, res["status"])
            assert (res["status"][~want_bad] == 0).all()
            good = np.flatnonzero(~want_bad & (order != 3))      # (pair 3 lies before 4: untouched; 4's tail was overwritten by 5's head)
            failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * len(frames), table.frame_off_host, tab[good], matches, False, False)
            assert failed == 0
            _same(tab[good], out, res[good], wout, wres)
            with pytest.raises(pkg.GmsError) as e:
                ctx.filter_host_batch(frames, [size] * len(frames), tab, matches, False, False, 6.0)
            assert e.value.code == -1
            # the same table with the overlap removed passes both entries
            fixed = tab.copy()
            fixed["match_off"][np.flatnonzero(order == 5)[0]] += n_kp // 2
            out, res, _ = batch.filter_pairs(ctx, table, fixed, matches, False, False, 6.0, want_mask=False)
            assert (res["status"] == 0).all()
            out2, res2 = ctx.filter_host_batch(frames, [size] * len(frames), fixed, matches, False, False, 6.0)
            assert res2.tobytes() == res.tobytes()


# ---- gms_ctx_set_option / gms_ctx_query: the library's bit-identical variants, forced ---------------------------------------------------
def test_forced_variants_give_the_same_bytes(pkg, oracle, synth):
    """gms_ctx_set_option forces the lane mapping of the byte-matrix kernel (option 1) and the scale probe (option 2); gms_ctx_query reports
    what the last launch ran with. On a zooming sequence (the right image at half the left one's magnification: the 28 x 28 hypothesis
    wins, the probe cannot bound it out; other pairs are won by scales 1 and 2) and with the default flags: every variant returns
    the oracle's bytes."""
    batch = importlib.import_module("sfm-gms_amd.batch")
    size, n_kp = (1920, 1080), 6000
    frames = synth.make_zoom_sequence(5, 6, size=size, n_kp=n_kp, zoom=2.0)
    pairs = np.zeros(6, dtype=pkg.PAIR_DTYPE)
    ms = []
    for i, (a, b) in enumerate(((1, 0), (3, 2), (5, 4), (0, 1), (1, 3), (0, 2))):
        mt = synth.sequence_matches(900 + i, n_kp, n_kp, 0.5)
        pairs[i] = (a, b, n_kp, 0, i * n_kp)
        ms.append(mt)
    matches = np.concatenate(ms)
    with pkg.GmsContext(0) as ctx:
        table = batch.FrameTable(ctx, frames, [size] * len(frames))
        failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * len(frames), table.frame_off_host, pairs, matches, True, True)
        assert failed == 0 and (wres["best_scale"][:3] == 3).all() and set(wres["best_scale"][3:].tolist()) <= {0, 1, 2}
        for val in (0, 1, -1):
            ctx.set_option(2, val)
            out, res, _ = batch.filter_pairs(ctx, table, pairs, matches, True, True, 6.0, want_mask=False)
            _same(pairs, out, res, wout, wres)
            if val >= 0:
                assert (ctx.query(2) != 0) == bool(val)
        failed, wout, wres, _ = _oracle_batch(oracle, frames, [size] * len(frames), table.frame_off_host, pairs, matches, False, False)
        for val in (0, 1, -1):
            ctx.set_option(1, val)
            out, res, _ = batch.filter_pairs(ctx, table, pairs, matches, False, False, 6.0, want_mask=False)
            _same(pairs, out, res, wout, wres)
            if val >= 0:
                assert ctx.query(1) == val and ctx.query(3) == 10
        with pytest.raises(pkg.GmsError):
            ctx.set_option(7, 1)
