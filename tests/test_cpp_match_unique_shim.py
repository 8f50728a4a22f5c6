"""The header-only C++ shim's one-to-one entry points (sfm-gms_amd/include/mi355_gms.hpp): mi355::uniqueMatches and mi355::registerViews
with a keep plane, on flat vectors. CPU: they compile and link against libgms_hip.so. GPU: on a registration case with redirected train
indices every output equals the numpy statement's (integers) and the Python one-shots' (every byte)."""

import numpy as np
import pytest

import match_unique_ref as U
import sfm_register_cases as cases
import hostbuild as hb


def test_match_unique_shim_compiles_and_links():
    exe = hb.shim_exe("match_unique_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_match_unique_shim_matches_python(tmp_path, pkg):
    exe = hb.shim_exe("match_unique_shim_main.cpp")
    c = U.redirect_trains(cases.case("chain_roles"), 0.3, 77)
    total = len(c["matches"])
    path = tmp_path / "records.bin"
    path.write_bytes(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["root"], c["min_links"]], np.int32).tobytes() +
                     np.array([total], np.int64).tobytes() + c["frame_off"].tobytes() + c["pairs"].tobytes() + c["matches"].tobytes() +
                     c["mask"].tobytes() + np.ascontiguousarray(c["points3d"]).tobytes() + c["tv"].tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    keep, counts = U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"])
    assert (counts[:, 1] < counts[:, 0]).any()
    want = pkg.registerViews(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"], keep=keep)
    keys = ("views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")
    n = int((c["pairs"]["match_off"] + c["pairs"]["m"]).max())   # (the shim's arrays end with the last pair's range)
    assert res.stdout.split() == [str(hb.fnv1a(keep[:n].tobytes())), str(hb.fnv1a(counts.tobytes()))] + [str(hb.fnv1a(want[k].tobytes())) for k in keys]
