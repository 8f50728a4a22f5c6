"""The header-only C++ shim's registration entry point (sfm-gms_amd/include/mi355_gms.hpp): mi355::registerViews on flat vectors.
CPU: it compiles and links against libgms_hip.so. GPU: on the hand-made records of tests/sfm_register_cases.py every output equals the
Python one-shot's, byte for byte."""

import numpy as np
import pytest

import sfm_register_cases as cases
import hostbuild as hb


def test_sfm_register_shim_compiles_and_links():
    exe = hb.shim_exe("sfm_register_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain_roles", "upstream_failures"])
def test_sfm_register_shim_matches_python(tmp_path, pkg, name):
    exe = hb.shim_exe("sfm_register_shim_main.cpp")
    c = cases.case(name)
    total = len(c["matches"])
    path = tmp_path / "records.bin"
    path.write_bytes(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["root"], c["min_links"]], np.int32).tobytes() +
                     np.array([total], np.int64).tobytes() + c["frame_off"].tobytes() + c["pairs"].tobytes() + c["matches"].tobytes() +
                     c["mask"].tobytes() + np.ascontiguousarray(c["points3d"]).tobytes() + c["tv"].tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    want = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    keys = ("views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")
    assert res.stdout.split() == [str(hb.fnv1a(want[k].tobytes())) for k in keys]
