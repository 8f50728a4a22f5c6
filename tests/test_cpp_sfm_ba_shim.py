"""The header-only C++ shim's bundle adjustment entry point (sfm-gms_amd/include/mi355_gms.hpp): mi355::bundleAdjust behind
mi355::registerViews on flat vectors. CPU: it compiles and links against libgms_hip.so. GPU: on hand-made inputs of
tests/sfm_ba_cases.py every output equals the Python one-shots', byte for byte."""

import numpy as np
import pytest

import sfm_ba_cases as cases
import hostbuild as hb


def test_sfm_ba_shim_compiles_and_links():
    exe = hb.shim_exe("sfm_ba_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_chain", "multi"])
def test_sfm_ba_shim_matches_python(tmp_path, pkg, name):
    exe = hb.shim_exe("sfm_ba_shim_main.cpp")
    c = cases.case(name)
    total = len(c["matches"])
    cam = pkg.types.make_camera(c["camera"][:4], c["camera"][4:])
    path = tmp_path / "records.bin"
    path.write_bytes(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["root"], c["min_links"]], np.int32).tobytes() +
                     np.array([total], np.int64).tobytes() + cam.tobytes() + c["frame_off"].tobytes() + c["kp"].tobytes() + c["pairs"].tobytes() +
                     c["matches"].tobytes() + c["mask"].tobytes() + np.ascontiguousarray(c["points3d"]).tobytes() + c["tv"].tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    reg = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    want = pkg.bundleAdjust(c["kp"], c["frame_off"], c["pairs"], c["matches"], c["mask"], reg, c["camera"][:4], c["camera"][4:])
    assert int(want["ba_summary"]["n_tracks_used"][0]) > 30
    assert res.stdout.split() == [str(hb.fnv1a(want[k].tobytes())) for k in ("views_ba", "cloud_ba", "track_status", "ba_summary")]
