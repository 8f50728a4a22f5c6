"""The header-only C++ shim's dense stage (sfm-gms_amd/include/mi355_gms.hpp): mi355::stereoRectify, mi355::undistort and
mi355::denseStereo. CPU: the shim compiles and links without a device, and the stage's record and workspace layouts hold
(tests/cpp/dense_layout_check.cpp). GPU: on the rendered plane of tests/rectify_cases.py the shim's results equal the Python ones,
compared by digest."""

import numpy as np
import pytest

import rectify_cases as rc
import hostbuild as hb


def test_dense_shim_compiles_and_links():
    res = hb.run(hb.shim_exe("dense_shim_main.cpp"))
    assert res.returncode == 2 and "usage" in res.stderr


def test_dense_layouts():
    res = hb.run(hb.host_exe("dense_layout_check.cpp"))          # host code on the C ABI's records alone: no shim, no library
    assert res.returncode == 0 and res.stdout.strip() == "dense_layout: ok", res.stdout


@pytest.mark.gpu
def test_dense_shim_matches_python(tmp_path, pkg):
    exe = hb.shim_exe("dense_shim_main.cpp")
    img1, img2 = rc.scene()
    w, h = rc.SCENE_SIZE
    dist = (0.05, -0.02, 0.001, -0.002, 0.01)
    path = tmp_path / "pair.bin"
    path.write_bytes(np.array([w, h], np.int32).tobytes() + np.array(list(rc.SCENE_CAMERA) + list(dist), np.float64).tobytes() +
                     np.ascontiguousarray(rc.SCENE_R, dtype=np.float64).tobytes() + np.asarray(rc.SCENE_T, np.float64).tobytes() +
                     img1.tobytes() + img2.tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    r = pkg.denseStereo(img1, img2, rc.SCENE_CAMERA, dist, rc.SCENE_R, rc.SCENE_T, **rc.SCENE_SGM)
    plan = r["plan"]
    lines = res.stdout.split("\n")
    assert lines[0].split() == [str(int(plan["turn"])), str(plan.out_size[0]), str(plan.out_size[1]), str(r["count"])] and r["count"] > 1000
    want = [plan.record, pkg.undistort(img1, rc.SCENE_CAMERA, dist), r["disp16"], r["points"], r["pixel"], r["colors"]]
    assert lines[1:7] == [str(hb.fnv1a(np.ascontiguousarray(a).tobytes())) for a in want]
