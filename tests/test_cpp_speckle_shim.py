"""The header-only C++ shim's speckle filter (sfm-gms_amd/include/mi355_gms.hpp): mi355::filterSpeckles. CPU: the shim compiles and
links without a device, and refuses bad arguments before any device is touched. GPU: on cases of tests/speckle_cases.py the shim's
results equal the `literal` statement's (tests/speckle_ref.py), compared by digest."""

import numpy as np
import pytest

import speckle_cases as sc
import hostbuild as hb

SHIM_CASES = ("plus_on_lattice_135x71", "extremes", "random_blobs_259x131")     # the first two runs of each: a process per run


def test_speckle_shim_compiles_links_and_refuses(tmp_path):
    exe = hb.shim_exe("speckle_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr
    path = tmp_path / "bad.bin"
    path.write_bytes(sc.case_bytes(np.zeros((3, 4), np.int16), 40000, 1, 1))        # new_val outside int16: refused before any launch
    res = hb.run(exe, path)
    assert res.returncode == 3 and "bad argument" in res.stderr


@pytest.mark.gpu
def test_speckle_shim_matches_the_statement(tmp_path):
    exe = hb.shim_exe("speckle_shim_main.cpp")
    by = {c["name"]: c for c in sc.all_cases()}
    for name in SHIM_CASES:
        case = by[name]
        for k, (size, diff, _) in enumerate(case["runs"][:2]):
            want, n_want = sc.expected(name, k)
            path = tmp_path / f"{name}_{k}.bin"
            path.write_bytes(sc.case_bytes(case["disp"], case["new_val"], size, diff))
            res = hb.run(exe, path, timeout=600)
            assert res.returncode == 0, (name, k, res.stderr)
            assert res.stdout.split() == [str(n_want), str(hb.fnv1a(want.tobytes()))], (name, k)
