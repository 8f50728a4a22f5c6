"""The header-only C++ shim's registration entry point (sfm-gms_amd/include/mi355_gms.hpp): mi355::registerViews on flat vectors.
CPU: it compiles and links against libgms_hip.so. GPU: on the hand-made records of tests/sfm_register_cases.py every output equals the
Python one-shot's, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import sfm_register_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")


def _build(tmp_path):
    exe = str(tmp_path / "sfm_register_shim_main")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "sfm_register_shim_main.cpp"), "-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def _fnv(b):
    s = 1469598103934665603
    for v in np.frombuffer(b, np.uint8):
        s = ((s ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return s


def test_sfm_register_shim_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain_roles", "upstream_failures"])
def test_sfm_register_shim_matches_python(tmp_path, pkg, name):
    exe = _build(tmp_path)
    c = cases.case(name)
    total = len(c["matches"])
    path = tmp_path / "records.bin"
    path.write_bytes(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["root"], c["min_links"]], np.int32).tobytes() +
                     np.array([total], np.int64).tobytes() + c["frame_off"].tobytes() + c["pairs"].tobytes() + c["matches"].tobytes() +
                     c["mask"].tobytes() + np.ascontiguousarray(c["points3d"]).tobytes() + c["tv"].tobytes())
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    want = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    keys = ("views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")
    assert res.stdout.split() == [str(_fnv(want[k].tobytes())) for k in keys]
