"""The header-only C++ shim's one-to-one entry points (sfm-gms_amd/include/mi355_gms.hpp): mi355::uniqueMatches and mi355::registerViews
with a keep plane, on flat vectors. CPU: they compile and link against libgms_hip.so. GPU: on a registration case with redirected train
indices every output equals the numpy statement's (integers) and the Python one-shots' (every byte)."""
import os
import subprocess

import numpy as np
import pytest

import match_unique_ref as U
import sfm_register_cases as cases
from test_cpp_sfm_register_shim import _fnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")


def _build(tmp_path):
    exe = str(tmp_path / "match_unique_shim_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "match_unique_shim_main.cpp"), "-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_match_unique_shim_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_match_unique_shim_matches_python(tmp_path, pkg):
    exe = _build(tmp_path)
    c = U.redirect_trains(cases.case("chain_roles"), 0.3, 77)
    total = len(c["matches"])
    path = tmp_path / "records.bin"
    path.write_bytes(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["root"], c["min_links"]], np.int32).tobytes() +
                     np.array([total], np.int64).tobytes() + c["frame_off"].tobytes() + c["pairs"].tobytes() + c["matches"].tobytes() +
                     c["mask"].tobytes() + np.ascontiguousarray(c["points3d"]).tobytes() + c["tv"].tobytes())
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    keep, counts = U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"])
    assert (counts[:, 1] < counts[:, 0]).any()
    want = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], keep=keep)
    keys = ("views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")
    n = int((c["pairs"]["match_off"] + c["pairs"]["m"]).max())   # (the shim's arrays end with the last pair's range)
    assert res.stdout.split() == [str(_fnv(keep[:n].tobytes())), str(_fnv(counts.tobytes()))] + [str(_fnv(want[k].tobytes())) for k in keys]
