"""-m gpu: every template instantiation of the per-pair filter kernels is launched once and must agree with the CPU oracle byte
for byte. The kernels are built in three files (hashed, byte matrix, byte matrix with scale hypotheses) for the matches-per-thread
classes 4, 10 and 16 with and without rotation hypotheses; a launch picks one through the host glue (launch_filter,
launch_filter_scales) and needs the dynamic-LDS limit that init_filter_kernels raised for exactly that instantiation. A missed
limit or a wrong branch in a launcher shows here as a failed launch or a wrong result.
Without scale hypotheses a case runs filter_kernel_dense, with them filter_kernel_dense_scales and then filter_kernel; the child
process with GMS_DEAL=1 runs the dealt instantiations of filter_kernel_dense: all 24 kernels (6 hashed, 12 byte-matrix, 6 with scale hypotheses)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

# the smallest m of each class (filter_pick_kpt: up to 4096, 10240 and 16384 matches per pair)
M_OF_KPT = {4: 4096, 10: 4097, 16: 10241}


@pytest.fixture(scope="module")
def pairs_of():
    """kpt -> two pairs of M_OF_KPT[kpt] matches each (built once, never modified)"""
    made = {}

    def get(kpt):
        if kpt not in made:
            m = M_OF_KPT[kpt]
            made[kpt] = [cases.random_pair(900 + kpt, n=m, inlier_frac=0.6),
                         cases.random_pair(950 + kpt, n=m, inlier_frac=0.4, theta_deg=90.0, scale=0.5)]
            assert all(len(c["matches"]) == m for c in made[kpt])
        return made[kpt]
    return get


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("kpt", [4, 10, 16])
def test_every_instantiation_against_the_oracle(ctx, oracle, pairs_of, kpt, rot, scale):
    batch = importlib.import_module("sfm-gms_amd.batch")
    types = importlib.import_module("sfm-gms_amd.types")
    cs = pairs_of(kpt)
    frames = batch.FrameTable(ctx, [c["kp1"] for c in cs] + [c["kp2"] for c in cs], [c["size1"] for c in cs] + [c["size2"] for c in cs])
    pairs = np.zeros(len(cs), dtype=types.PAIR_DTYPE)
    off = 0
    for i, c in enumerate(cs):
        pairs[i]["frame_a"], pairs[i]["frame_b"], pairs[i]["m"], pairs[i]["match_off"] = i, len(cs) + i, len(c["matches"]), off
        off += len(c["matches"])
    out, results, _ = batch.filter_pairs(ctx, frames, pairs, np.concatenate([c["matches"] for c in cs]), rot, scale, 6.0)
    for i, c in enumerate(cs):
        rc, want, _, wres = oracle.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], rot, scale, 6.0)
        assert rc == 0 and results[i]["status"] == 0
        assert i != 0 or wres["n_inliers"] > 0  # (the unrotated pair has survivors under every flag combination: there is something to compare)
        o, k = int(pairs[i]["match_off"]), int(results[i]["n_inliers"])
        assert (k, int(results[i]["best_scale"]), int(results[i]["best_rot"])) == (wres["n_inliers"], wres["best_scale"], wres["best_rot"])
        assert out[o:o + k].tobytes() == want.tobytes()


def test_dealt_instantiations_whole_file_again():
    """GMS_DEAL=1 (read once per process) selects the byte-matrix kernel's dealt instantiations: the same twelve cases once more."""
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "not whole_file_again"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, GMS_DEAL="1"))
    assert res.returncode == 0, res.stdout[-3000:]
