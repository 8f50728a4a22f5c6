"""The header-only C++ shim's pair-pose entry point (sfm-gms_amd/include/mi355_gms.hpp): mi355::pairPosesFromViews on flat vectors.
CPU: it compiles and links against libgms_hip.so. GPU: on random views with good and bad pairs its records equal the numpy statement
(tests/sfm_pair_pose_ref.py), byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import sfm_pair_pose_cases as pc
import sfm_pair_pose_ref as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")


def _build(tmp_path):
    exe = str(tmp_path / "sfm_pair_pose_shim_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "sfm_pair_pose_shim_main.cpp"), "-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_sfm_pair_pose_shim_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_sfm_pair_pose_shim_matches_the_statement(tmp_path):
    exe = _build(tmp_path)
    _, views, fp = pc.random_case(21, 9, 70, bad_last=True)
    fp = np.concatenate([fp, [(3, 3), (-1, 2)]])
    src, dst = tmp_path / "case.bin", tmp_path / "result.bin"
    src.write_bytes(np.array([len(views), len(fp)], np.int32).tobytes() + views.tobytes() + fp.astype(np.int32).tobytes())
    res = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    tv, reg = pp.pair_poses(views, fp)
    assert (tv["status"] == pp.GMS_OK).sum() == 69
    assert dst.read_bytes() == pp.result_bytes(tv, reg)
