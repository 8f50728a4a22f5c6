"""-m gpu: every kernel family of the large-pair path (pairs above 16 384 matches) is launched once, at the smallest size that reaches
it, and must agree with the CPU oracle byte for byte -- the counterpart of test_gpu_filter_instantiations.py. What sends a case where
(plan_workspace and filter_launch in gms_capi.cpp):
  * filter_pick_kpt(max_m) is 0 above 16 384 matches: the launch leaves the per-pair kernels;
  * max_m <= stream_max_matches() = 65 536 picks the streamed kernels. With scale hypotheses, or when the slice has fewer pairs than
    the device has CUs, that is launch_filter_stream (stream_index_kernel<0|1>, stream_filter / _mark / _compact_kernel<ROT>); without
    scale hypotheses and with a pair for every CU it is launch_filter_stream_dense: stream_dense_kernel<true> with rotation,
    stream_plain_kernel without -- or stream_dense_kernel<false> in a process started with GMS_STREAM_PLAIN=0;
  * above 65 536 matches the default flags go to launch_filter_band (band_codes / _filter / _compact_kernel), every other flag
    combination to launch_filter_tiles (tile_codes_kernel, tile_filter / _count / _apply_kernel<ROT>, band_compact_kernel);
  * behind each of them launch_filter_big (filter_kernel_big<ROT>) takes the pairs whose flag word says kFlagGeneral: here a pair of
    16 385 matches with one queryIdx past its frame, which stream_index_kernel<0> hands on and the slab kernel fails as the oracle does.
A context that has met a byte-matrix overflow (test_gpu_band_path.py provokes one) stays off the streamed kernels for its next 64
large launches (stream_penalty in gms_capi.cpp): the module spends them first, so that the cases reach the kernels they name whatever
ran before on the session's context."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

M_STREAM = 16385   # the first size beyond the per-pair kernels
M_BAND = 65537     # the first size the streamed kernels do not take


class _Large:
    """Pairs of m matches and their oracle answers per (rot, scale): built once, never modified."""

    def __init__(self, oracle):
        self.oracle, self.pairs, self.want = oracle, {}, {}

    def cases(self, m):
        if m not in self.pairs:
            self.pairs[m] = [cases.random_pair(700 + m % 97, n=m, size1=(3840, 2160), inlier_frac=0.6),
                             cases.random_pair(750 + m % 97, n=m, size1=(3840, 2160), inlier_frac=0.4, theta_deg=90.0, scale=0.5)]
            assert all(len(c["matches"]) == m for c in self.pairs[m])
        return self.pairs[m]

    def answer(self, m, i, rot, scale):
        if (m, i, rot, scale) not in self.want:
            c = self.cases(m)[i]
            rc, want, _, wres = self.oracle.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], rot, scale, 6.0)
            assert rc == 0
            self.want[(m, i, rot, scale)] = (want, wres)
        return self.want[(m, i, rot, scale)]


@pytest.fixture(scope="module")
def large(ctx, oracle):
    batch = importlib.import_module("sfm-gms_amd.batch")
    types = importlib.import_module("sfm-gms_amd.types")
    lg = _Large(oracle)
    c = lg.cases(M_STREAM)[0]
    frames = batch.FrameTable(ctx, [c["kp1"], c["kp2"]], [c["size1"], c["size2"]])
    pair = np.zeros(1, dtype=types.PAIR_DTYPE)
    pair[0]["frame_a"], pair[0]["frame_b"], pair[0]["m"] = 0, 1, M_STREAM
    for _ in range(65):  # (the launch that notices an overflow, then the 64 of the penalty)
        batch.filter_pairs(ctx, frames, pair, c["matches"], False, False, 6.0, want_mask=False)
    return lg


def _filter(ctx, cs, pair_of, matches, rot, scale):
    """frames = both images of every case; pair_of = [(case index, match_off)]"""
    batch = importlib.import_module("sfm-gms_amd.batch")
    types = importlib.import_module("sfm-gms_amd.types")
    frames = batch.FrameTable(ctx, [c["kp1"] for c in cs] + [c["kp2"] for c in cs], [c["size1"] for c in cs] + [c["size2"] for c in cs])
    pairs = np.zeros(len(pair_of), dtype=types.PAIR_DTYPE)
    for k, (i, off) in enumerate(pair_of):
        pairs[k]["frame_a"], pairs[k]["frame_b"], pairs[k]["m"], pairs[k]["match_off"] = i, len(cs) + i, len(cs[i]["matches"]), off
    out, results, _ = batch.filter_pairs(ctx, frames, pairs, matches, rot, scale, 6.0)
    return frames, pairs, out, results


def _same(out, results, k, off, want, wres):
    n = int(results[k]["n_inliers"])
    assert results[k]["status"] == 0
    assert (n, int(results[k]["best_scale"]), int(results[k]["best_rot"])) == (wres["n_inliers"], wres["best_scale"], wres["best_rot"])
    assert out[off:off + n].tobytes() == want.tobytes()


def _two_pairs(ctx, large, m, rot, scale):
    cs = large.cases(m)
    _, _, out, results = _filter(ctx, cs, [(0, 0), (1, m)], np.concatenate([c["matches"] for c in cs]), rot, scale)
    assert large.answer(m, 0, rot, scale)[1]["n_inliers"] > 0  # (the unrotated pair has survivors under every flag combination)
    for i in range(2):
        _same(out, results, i, i * m, *large.answer(m, i, rot, scale))


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("rot", [False, True])
def test_streamed_pipeline(ctx, large, rot, scale):
    """launch_filter_stream: two pairs of 16 385 matches -- with scale hypotheses by the first rule, without them because two pairs are
    fewer than the device's CUs."""
    assert ctx.query(5) > 2
    _two_pairs(ctx, large, M_STREAM, rot, scale)


@pytest.mark.parametrize("rot", [False, True])
def test_streamed_one_workgroup_per_pair(ctx, large, rot):
    """launch_filter_stream_dense: no scale hypotheses and as many pairs as the device has CUs -- one pair of 16 385 matches submitted
    that many times over disjoint ranges of the match array that repeat its records. rot = True: stream_dense_kernel<true>;
    rot = False: stream_plain_kernel, or stream_dense_kernel<false> under GMS_STREAM_PLAIN=0 (the test below)."""
    n = ctx.query(5)  # GMS_QUERY_CUS
    c = large.cases(M_STREAM)[0]
    _, _, out, results = _filter(ctx, [c], [(0, k * M_STREAM) for k in range(n)], np.tile(c["matches"], n), rot, False)
    want, wres = large.answer(M_STREAM, 0, rot, False)
    assert wres["n_inliers"] > 0
    for k in (0, n // 2, n - 1):
        _same(out, results, k, k * M_STREAM, want, wres)


def test_older_one_workgroup_per_pair_kernel_in_a_child_process():
    """GMS_STREAM_PLAIN=0 (read once per process): the default-flags case above on stream_dense_kernel<false>."""
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q",
                          "-k", "test_streamed_one_workgroup_per_pair and False"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, GMS_STREAM_PLAIN="0"))
    assert res.returncode == 0 and "1 passed" in res.stdout, res.stdout[-3000:]


@pytest.mark.parametrize("rot,scale", [(False, False), (True, False), (True, True)])
def test_band_and_tile_kernels(ctx, large, rot, scale):
    """Two pairs of 65 537 matches: launch_filter_band under the default flags, launch_filter_tiles (one ROT instantiation each)
    under the other two."""
    _two_pairs(ctx, large, M_BAND, rot, scale)


def test_slab_kernel_for_a_pair_handed_on(ctx, oracle, large):
    """Default flags, two pairs of 16 385 matches, one queryIdx of the first one past its frame: stream_index_kernel<0> flags that
    pair general, filter_kernel_big<false> reports the oracle's domain error for it with nothing kept; the other pair is untouched."""
    cs = large.cases(M_STREAM)
    bad = cs[0]["matches"].copy()
    bad["queryIdx"][4321] = len(cs[0]["kp1"])
    matches = np.concatenate([bad, cs[1]["matches"]])
    frames, pairs, out, results = _filter(ctx, cs, [(0, 0), (1, M_STREAM)], matches, False, False)
    kp_all = np.concatenate([c["kp1"] for c in cs] + [c["kp2"] for c in cs])
    wh = np.array([c["size1"] for c in cs] + [c["size2"] for c in cs], dtype=np.int32).reshape(-1)
    failed, _, wres, _ = oracle.batch(kp_all, frames.frame_off_host, wh, pairs, matches, False, False, 6.0, 2)
    assert failed == 1 and wres["status"][0] == -2 and results.tobytes() == wres.tobytes()
    _same(out, results, 1, M_STREAM, *large.answer(M_STREAM, 1, False, False))
