"""The header-only C++ shim's semi-global matching entry points (sfm-gms_amd/include/mi355_gms.hpp): mi355::stereo_match_sgm and
mi355::stereoSGM on flat 8-bit vectors. CPU: they compile and link against libgms_hip.so. GPU: on the committed 450 x 375 pair both
equal the Python result."""
import os

import numpy as np
import pytest

import hostbuild as hb

GOLDEN = os.path.join(hb.ROOT, "tests", "golden", "image_stereo_pair_450x375.npz")


def test_stereo_sgm_shim_compiles_and_links():
    exe = hb.shim_exe("stereo_sgm_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_stereo_sgm_shim_matches_python(tmp_path, pkg):
    exe = hb.shim_exe("stereo_sgm_shim_main.cpp")
    z = np.load(GOLDEN)
    left, right = z["left"], z["right"]
    h, w = left.shape
    path = tmp_path / "pair.bin"
    path.write_bytes(np.array([w, h], np.int32).tobytes() + left.tobytes() + right.tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split()
    assert lines == [str(hb.fnv1a(pkg.stereo_match_sgm(left, right).tobytes())), str(hb.fnv1a(pkg.stereoSGM(left, right, n_paths=4).tobytes()))]
