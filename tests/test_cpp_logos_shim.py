"""The header-only C++ shim's LOGOS entry points (sfm-gms_amd/include/mi355_gms.hpp): mi355::matchLOGOS with the reference's
signature and mi355::matchLOGOSBatch. CPU: they compile and link against libgms_hip.so. GPU: the fixture cases of
tests/golden/refdll_logos.npz through both give the fixture's matches."""
import os

import numpy as np
import pytest

import hostbuild as hb

Z = np.load(os.path.join(hb.ROOT, "tests", "golden", "refdll_logos.npz"))
NAMES = sorted(k[: -len("_matches")] for k in Z.files if k.endswith("_matches"))

def _records(pairs):
    """The gms_dmatch records of (query, train) pairs: imgIdx -1, distance 0."""
    rec = np.zeros((len(pairs), 4), np.int32)
    rec[:, :2] = np.asarray(pairs, np.int32).reshape(-1, 2)
    rec[:, 2] = -1
    return rec


def test_logos_shim_compiles_and_links():
    exe = hb.shim_exe("logos_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_logos_shim_matches_fixture(tmp_path):
    exe = hb.shim_exe("logos_shim_main.cpp")
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(NAMES)).tobytes())
        for name in NAMES:
            k1, k2 = Z[name + "_kp1"].astype(np.float32), Z[name + "_kp2"].astype(np.float32)
            f.write(np.array([len(k1), len(k2)], np.int32).tobytes())
            f.write(k1.tobytes() + k2.tobytes())
            f.write(Z[name + "_nn1"].astype(np.int32).tobytes() + Z[name + "_nn2"].astype(np.int32).tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 2 * len(NAMES)
    for c, name in enumerate(NAMES):
        want = Z[name + "_matches"]
        assert lines[c].split() == [str(len(want)), str(hb.fnv1a(_records(want), words=True))], name
        assert lines[len(NAMES) + c].split() == [str(len(want)), str(hb.fnv1a(_records(want), words=True)), "1"], name
