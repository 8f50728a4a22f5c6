#!/usr/bin/env python3
"""Writes tests/golden/image_portrait_robot.npz from the reference's own input images (data, not source):
    /root/reference/SfM-GMS/SourceImages/leftRobot.png, rightRobot.png   the 2594 x 1131 pair of the portrait-mode demo (DisparityUtil.cpp:465-476)
reduced by FACTOR in each direction (the rounded mean of each FACTOR x FACTOR block; the rows and columns left over are dropped): the left
image as BGR uint8 [H, W, 3], as imread gives it, and the right image as 8-bit grey, grey = (299 R + 587 G + 114 B + 500) // 1000 (the
weights of cv::cvtColor's BGR2GRAY, in integers). Pixel data only. The GPU box has no /root/reference; the tests and tools read this
fixture. Run here: python tests/golden/make_portrait_fixture.py"""
import os
import numpy as np
from PIL import Image

SRC = "/root/reference/SfM-GMS/SourceImages"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_portrait_robot.npz")
FACTOR = 4


def reduced_rgb(name):
    im = np.array(Image.open(os.path.join(SRC, name)).convert("RGB")).astype(np.int64)
    h, w = im.shape[0] // FACTOR, im.shape[1] // FACTOR
    blocks = im[:h * FACTOR, :w * FACTOR].reshape(h, FACTOR, w, FACTOR, 3)
    return (blocks.sum(axis=(1, 3)) + FACTOR * FACTOR // 2) // (FACTOR * FACTOR)


left, right = reduced_rgb("leftRobot.png"), reduced_rgb("rightRobot.png")
right_grey = ((299 * right[..., 0] + 587 * right[..., 1] + 114 * right[..., 2] + 500) // 1000).astype(np.uint8)
np.savez_compressed(OUT, left_bgr=left[..., ::-1].astype(np.uint8), right_grey=right_grey)
print(OUT, os.path.getsize(OUT), {k: v.shape for k, v in np.load(OUT).items()})
