"""The header-only C++ shim's pair-pose entry point (sfm-gms_amd/include/mi355_gms.hpp): mi355::pairPosesFromViews on flat vectors.
CPU: it compiles and links against libgms_hip.so. GPU: on random views with good and bad pairs its records equal the numpy statement
(tests/sfm_pair_pose_ref.py), byte for byte."""

import numpy as np
import pytest

import sfm_pair_pose_cases as pc
import sfm_pair_pose_ref as pp
import hostbuild as hb


def test_sfm_pair_pose_shim_compiles_and_links():
    exe = hb.shim_exe("sfm_pair_pose_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_sfm_pair_pose_shim_matches_the_statement(tmp_path):
    exe = hb.shim_exe("sfm_pair_pose_shim_main.cpp")
    _, views, fp = pc.random_case(21, 9, 70, bad_last=True)
    fp = np.concatenate([fp, [(3, 3), (-1, 2)]])
    src, dst = tmp_path / "case.bin", tmp_path / "result.bin"
    src.write_bytes(np.array([len(views), len(fp)], np.int32).tobytes() + views.tobytes() + fp.astype(np.int32).tobytes())
    res = hb.run(exe, src, dst)
    assert res.returncode == 0, res.stderr
    tv, reg = pp.pair_poses(views, fp)
    assert (tv["status"] == pp.GMS_OK).sum() == 69
    assert dst.read_bytes() == pp.result_bytes(tv, reg)
