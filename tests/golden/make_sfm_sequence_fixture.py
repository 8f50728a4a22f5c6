#!/usr/bin/env python3
"""Writes tests/golden/image_sfm_more_1008x756.npz from the reference's own SfM input photographs (data, not source):
    /root/reference/SfM-GMS/SourceImages/PikaBun2.jpg, PikaBun3.jpg   the two 2016 x 1512 views between those of
                                                                       image_sfm_pair_1008x756.npz (PikaBun1, PikaBun4)
    second, third   8-bit grey, halved to 1008 x 756, exactly as make_sfm_fixture.py makes its `left` and `right`
With the committed pair (left = view 1, right = view 4) this gives the sequence 1, 2, 3, 4 that the registration tests and
tools/gms_sfm_sequence.py run; the stated camera is that fixture's.
The GPU box has no /root/reference; the tests and tools read this fixture. Run here: python tests/golden/make_sfm_sequence_fixture.py"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pyramid_ref  # noqa: E402

SRC = "/root/reference/SfM-GMS/SourceImages"
OUT = os.path.join(HERE, "image_sfm_more_1008x756.npz")


def rgb(name):
    return np.array(Image.open(os.path.join(SRC, name)).convert("RGB"))


def grey_half(im):
    im = im.astype(np.int64)
    g = ((299 * im[..., 0] + 587 * im[..., 1] + 114 * im[..., 2] + 500) // 1000).astype(np.uint8)
    return pyramid_ref.resize(g, g.shape[1] // 2, g.shape[0] // 2)


second, third = rgb("PikaBun2.jpg"), rgb("PikaBun3.jpg")
assert second.shape == third.shape == (1512, 2016, 3)
np.savez_compressed(OUT, second=grey_half(second), third=grey_half(third))
print(OUT, os.path.getsize(OUT), {k: v.shape for k, v in np.load(OUT).items()})
