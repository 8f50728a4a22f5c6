"""The header-only C++ shim's image transforms (sfm-gms_amd/include/mi355_gms.hpp): mi355::resize, mi355::warpAffine,
mi355::getRotationMatrix2D and mi355::img_rotate on flat 8-bit vectors. (That they compile and link without a device is checked in
tests/test_warp_ref.py.) GPU: on a cut of the reference's photograph they equal the Python results, compared by digest."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_portrait_robot.npz")


def _build(tmp_path):
    exe = str(tmp_path / "warp_shim_main")
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sfm-gms_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "warp_shim_main.cpp"), "-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC,
           "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def _fnv(b):
    s = 1469598103934665603
    for v in np.frombuffer(b, np.uint8):
        s = ((s ^ int(v)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return s


@pytest.mark.gpu
def test_warp_shim_matches_python(tmp_path, pkg):
    exe = _build(tmp_path)
    bgr = np.ascontiguousarray(np.load(GOLDEN)["left_bgr"][:120, :200])
    h, w = bgr.shape[:2]
    path = tmp_path / "image.bin"
    path.write_bytes(np.array([w, h], np.int32).tobytes() + bgr.tobytes())
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    want = [pkg.resize(bgr, (101, 67)), pkg.imgRotate(bgr, 180), pkg.warpAffine(bgr, pkg.getRotationMatrix2D((30, 20), 30, 0.8), (90, 50)),
            pkg.resize(np.ascontiguousarray(bgr[:, :, 0]), (w // 2, h // 2))]
    assert res.stdout.split() == [str(_fnv(a.tobytes())) for a in want]
