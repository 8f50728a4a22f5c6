"""The header-only C++ shim's speckle filter (sfm-gms_amd/include/mi355_gms.hpp): mi355::filterSpeckles. CPU: the shim compiles and
links without a device, and refuses bad arguments before any device is touched. GPU: on cases of tests/speckle_cases.py the shim's
results equal the `literal` statement's (tests/speckle_ref.py), compared by digest."""
import os
import subprocess

import numpy as np
import pytest

import speckle_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include")]
SHIM_CASES = ("plus_on_lattice_135x71", "extremes", "random_blobs_259x131")     # the first two runs of each: a process per run


def _build(tmp_path):
    exe = str(tmp_path / "speckle_shim_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *INCLUDES, os.path.join(ROOT, "tests", "cpp", "speckle_shim_main.cpp"), "-L", CSRC,
                           "-lgms_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def _fnv(a):
    s = 1469598103934665603
    for v in np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8):
        s = ((s ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return s


def test_speckle_shim_compiles_links_and_refuses(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "usage" in res.stderr
    path = tmp_path / "bad.bin"
    path.write_bytes(sc.case_bytes(np.zeros((3, 4), np.int16), 40000, 1, 1))        # new_val outside int16: refused before any launch
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 3 and "bad argument" in res.stderr


@pytest.mark.gpu
def test_speckle_shim_matches_the_statement(tmp_path):
    exe = _build(tmp_path)
    by = {c["name"]: c for c in sc.all_cases()}
    for name in SHIM_CASES:
        case = by[name]
        for k, (size, diff, _) in enumerate(case["runs"][:2]):
            want, n_want = sc.expected(name, k)
            path = tmp_path / f"{name}_{k}.bin"
            path.write_bytes(sc.case_bytes(case["disp"], case["new_val"], size, diff))
            res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, (name, k, res.stderr)
            assert res.stdout.split() == [str(n_want), str(_fnv(want))], (name, k)
