"""The header-only C++ shim's bundle adjustment entry point (sfm-gms_amd/include/mi355_gms.hpp): mi355::bundleAdjust behind
mi355::registerViews on flat vectors. CPU: it compiles and links against libgms_hip.so. GPU: on hand-made inputs of
tests/sfm_ba_cases.py every output equals the Python one-shots', byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import sfm_ba_cases as cases
from test_cpp_sfm_register_shim import _fnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")


def _build(tmp_path):
    exe = str(tmp_path / "sfm_ba_shim_main")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "sfm_ba_shim_main.cpp"), "-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_sfm_ba_shim_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_chain", "multi"])
def test_sfm_ba_shim_matches_python(tmp_path, pkg, name):
    exe = _build(tmp_path)
    c = cases.case(name)
    total = len(c["matches"])
    cam = pkg.types.make_camera(c["camera"][:4], c["camera"][4:])
    path = tmp_path / "records.bin"
    path.write_bytes(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["root"], c["min_links"]], np.int32).tobytes() +
                     np.array([total], np.int64).tobytes() + cam.tobytes() + c["frame_off"].tobytes() + c["kp"].tobytes() + c["pairs"].tobytes() +
                     c["matches"].tobytes() + c["mask"].tobytes() + np.ascontiguousarray(c["points3d"]).tobytes() + c["tv"].tobytes())
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    reg = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    want = pkg.bundleAdjust(c["kp"], c["frame_off"], c["pairs"], c["matches"], c["mask"], reg, c["camera"][:4], c["camera"][4:])
    assert int(want["ba_summary"]["n_tracks_used"][0]) > 30
    assert res.stdout.split() == [str(_fnv(want[k].tobytes())) for k in ("views_ba", "cloud_ba", "track_status", "ba_summary")]
