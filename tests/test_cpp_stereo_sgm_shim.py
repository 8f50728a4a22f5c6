"""The header-only C++ shim's semi-global matching entry points (sfm-gms_amd/include/mi355_gms.hpp): mi355::stereo_match_sgm and
mi355::stereoSGM on flat 8-bit vectors. CPU: they compile and link against libgms_hip.so. GPU: on the committed 450 x 375 pair both
equal the Python result."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_stereo_pair_450x375.npz")


def _build(tmp_path):
    exe = str(tmp_path / "stereo_sgm_shim_main")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "stereo_sgm_shim_main.cpp"), "-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def _fnv(b):
    s = 1469598103934665603
    for v in np.frombuffer(b, np.uint8):
        s = ((s ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return s


def test_stereo_sgm_shim_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_stereo_sgm_shim_matches_python(tmp_path, pkg):
    exe = _build(tmp_path)
    z = np.load(GOLDEN)
    left, right = z["left"], z["right"]
    h, w = left.shape
    path = tmp_path / "pair.bin"
    path.write_bytes(np.array([w, h], np.int32).tobytes() + left.tobytes() + right.tobytes())
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split()
    assert lines == [str(_fnv(pkg.stereo_match_sgm(left, right).tobytes())), str(_fnv(pkg.stereoSGM(left, right, n_paths=4).tobytes()))]
