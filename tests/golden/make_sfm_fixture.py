#!/usr/bin/env python3
"""Writes tests/golden/image_sfm_pair_1008x756.npz from the reference's own SfM input photographs (data, not source):
    /root/reference/SfM-GMS/SourceImages/PikaBun1.jpg, PikaBun4.jpg   two 2016 x 1512 views of one scene (main.cpp:52-75 reads such pairs
                                                                       and hands them to structureFromMotion, SfMUtil.cpp:4-83)
    left, right   8-bit grey, grey = (299 R + 587 G + 114 B + 500) // 1000 (make_image_fixture.py's formula), halved to 1008 x 756 with
                  tests/pyramid_ref.py's integer bilinear resize
    bgr_crop      a 96 x 64 x 3 piece of the first photograph as it is, channels in B, G, R order (what a CV_8UC3 Mat holds)
    camera        (fx, fy, cx, cy) = (800, 800, 504, 378) for the halved images: a STATED pinhole camera, not a calibration
The GPU box has no /root/reference; the tests and tools read this fixture. Run here: python tests/golden/make_sfm_fixture.py"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pyramid_ref  # noqa: E402

SRC = "/root/reference/SfM-GMS/SourceImages"
OUT = os.path.join(HERE, "image_sfm_pair_1008x756.npz")


def rgb(name):
    return np.array(Image.open(os.path.join(SRC, name)).convert("RGB"))


def grey_half(im):
    im = im.astype(np.int64)
    g = ((299 * im[..., 0] + 587 * im[..., 1] + 114 * im[..., 2] + 500) // 1000).astype(np.uint8)
    return pyramid_ref.resize(g, g.shape[1] // 2, g.shape[0] // 2)


first, second = rgb("PikaBun1.jpg"), rgb("PikaBun4.jpg")
assert first.shape == second.shape == (1512, 2016, 3)
crop = np.ascontiguousarray(first[700:764, 900:996, ::-1])   # 64 rows x 96 columns, B, G, R
np.savez_compressed(OUT, left=grey_half(first), right=grey_half(second), bgr_crop=crop, camera=np.array([800.0, 800.0, 504.0, 378.0]))
print(OUT, os.path.getsize(OUT), {k: v.shape for k, v in np.load(OUT).items()})
