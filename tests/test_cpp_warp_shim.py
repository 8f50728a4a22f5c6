"""The header-only C++ shim's image transforms (sfm-gms_amd/include/mi355_gms.hpp): mi355::resize, mi355::warpAffine,
mi355::getRotationMatrix2D and mi355::img_rotate on flat 8-bit vectors. (That they compile and link without a device is checked in
tests/test_warp_ref.py.) GPU: on a cut of the reference's photograph they equal the Python results, compared by digest."""
import os

import numpy as np
import pytest

import hostbuild as hb

GOLDEN = os.path.join(hb.ROOT, "tests", "golden", "image_portrait_robot.npz")


@pytest.mark.gpu
def test_warp_shim_matches_python(tmp_path, pkg):
    exe = hb.shim_exe("warp_shim_main.cpp")
    bgr = np.ascontiguousarray(np.load(GOLDEN)["left_bgr"][:120, :200])
    h, w = bgr.shape[:2]
    path = tmp_path / "image.bin"
    path.write_bytes(np.array([w, h], np.int32).tobytes() + bgr.tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    want = [pkg.resize(bgr, (101, 67)), pkg.imgRotate(bgr, 180), pkg.warpAffine(bgr, pkg.getRotationMatrix2D((30, 20), 30, 0.8), (90, 50)),
            pkg.resize(np.ascontiguousarray(bgr[:, :, 0]), (w // 2, h // 2))]
    assert res.stdout.split() == [str(hb.fnv1a(a.tobytes())) for a in want]
