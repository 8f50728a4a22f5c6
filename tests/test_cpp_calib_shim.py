"""The header-only C++ shim's calibration calls (sfm-gms_amd/include/mi355_gms.hpp): mi355::findChessboardCorners, cornerSubPix,
calibrateCamera and addChessboardPoints on flat grey images. CPU: they compile and link without a device. GPU: on three named boards
and one image without a board (tests/calib_cases.py) they give what the Python calls give, to the last digit printed."""

import numpy as np
import pytest

import calib_cases as CC
import hostbuild as hb


def test_calib_shim_compiles_and_links():
    res = hb.run(hb.shim_exe("calib_shim_main.cpp"))
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
def test_calib_shim_matches_python(tmp_path, pkg):
    exe = hb.shim_exe("calib_shim_main.cpp")
    names = ("rot0", "covered", "perspective", "edges")          # one size; the second has no board
    imgs = np.stack([CC.case(n).image for n in names])
    n, h, w = imgs.shape
    path = tmp_path / "images.bin"
    path.write_bytes(np.array([n, w, h, CC.NX, CC.NY], np.int32).tobytes() + imgs.tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    lines = [[float(v) for v in ln.split()] for ln in res.stdout.strip().splitlines()]
    ok, obj, img = pkg.addChessboardPoints(list(imgs), (CC.NX, CC.NY))
    assert ok == 3 and lines[0] == [3.0]
    for k in range(3):
        assert lines[1 + k] == [img[k][0, 0], img[k][0, 1], img[k][-1, 0], img[k][-1, 1]]
    rms, K, dist, _, _ = pkg.calibrateCamera(obj, img, (w, h))
    assert lines[4] == [K[0, 0], K[1, 1], K[0, 2], K[1, 2]] and lines[5] == list(dist) and lines[6] == [rms]
    # three views of one synthetic camera: the calibration is near the camera that rendered them
    assert abs(K[0, 0] - CC.INTR[0]) < 0.05 * CC.INTR[0] and rms < 0.5
