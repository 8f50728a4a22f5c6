#!/usr/bin/env python3
"""Writes tests/golden/image_calib_a.npz .. image_calib_e.npz from the reference's own calibration photographs (data, not source):
    /root/reference/SfM-GMS/CalibrationImages/IMG_0.jpg .. IMG_9.jpg   ten 2016 x 1512 views of a chessboard with 6 x 9 inner corners
                                                                       (main.cpp:53-68 hands them to addChessboardPoints)
    images   uint8 [2, 756, 1008]: grey = (299 R + 587 G + 114 B + 500) // 1000 (make_image_fixture.py's formula), halved with the
             exact 2 x 2 mean (a + b + c + d + 2) >> 2 -- the scale of image_sfm_pair_1008x756.npz, so that a camera calibrated on
             these applies to that pair directly. IMG_0, IMG_1 in file a, IMG_2, IMG_3 in file b, and so on: five files of two
             images, about 0.8 MB each, so that no committed file passes 1 MiB (ten in one file compress to 4.1 MB)
    board    (6, 9): points per row, rows
The GPU box has no /root/reference; the tests and tools read these fixtures. Run here: python tests/golden/make_calib_fixture.py"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = "/root/reference/SfM-GMS/CalibrationImages"


def grey_half(name):
    im = np.array(Image.open(os.path.join(SRC, name)).convert("RGB")).astype(np.int64)
    assert im.shape == (1512, 2016, 3)
    g = (299 * im[..., 0] + 587 * im[..., 1] + 114 * im[..., 2] + 500) // 1000
    return ((g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2).astype(np.uint8)


for k, tag in enumerate("abcde"):
    ids = (2 * k, 2 * k + 1)
    out = os.path.join(HERE, f"image_calib_{tag}.npz")
    np.savez_compressed(out, images=np.stack([grey_half(f"IMG_{i}.jpg") for i in ids]), board=np.array([6, 9], np.int32))
    print(out, os.path.getsize(out))
