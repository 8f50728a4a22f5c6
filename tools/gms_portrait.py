#!/usr/bin/env python3
"""The reference's portrait-mode demo (DisparityUtil.cpp:274-428, called at :476) from two photographs to the final picture, on the GPU:
    left (BGR) + right -> an 8-bit disparity map by a named source -> portraitMode (gms_portrait) -> the portrait image.

    python tools/gms_portrait.py [pair.npz] [--disparity bm|matches|FILE.npy] [--out portrait.npy] [--threshold 60] [--dilate 2]
                                 [--contours 5] [--ksize 15] [--check]

pair.npz holds left_bgr [H, W, 3] and right_grey [H, W] (default: the committed reduced robot pair, tests/golden/image_portrait_robot.npz).
--disparity bm       the project's stereo_match map of the pair (StereoBM with the reference's parameters, normalised, 0 -> 255)
--disparity sgm      the same form from semi-global matching on StereoBM's costs (stereo_match_sgm)
--disparity matches  detector -> matcher -> matchGMS -> gms_disparity_device (tools/gms_image_pair.py, run as a child process); 255 = no match,
                     which is the map createPortraitMode itself starts from. There is no SIFT here, so the keypoints are the project's own.
--disparity FILE.npy any uint8 [H, W] map, 255 = no value
Writes the portrait as .npy (and a .png beside it when PIL is there); prints one JSON line. --check compares with tests/portrait_ref.py."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grey(bgr):
    b = bgr.astype(np.int64)
    return ((299 * b[..., 2] + 587 * b[..., 1] + 114 * b[..., 0] + 500) // 1000).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pair", nargs="?", default=os.path.join(ROOT, "tests", "golden", "image_portrait_robot.npz"))
    ap.add_argument("--disparity", default="bm")
    ap.add_argument("--out", default="portrait.npy")
    ap.add_argument("--threshold", type=int, default=60)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--contours", type=int, default=5)
    ap.add_argument("--ksize", type=int, default=15)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    z = np.load(a.pair)
    bgr = np.ascontiguousarray(z["left_bgr"], dtype=np.uint8)
    right = np.ascontiguousarray(z["right_grey"], dtype=np.uint8)
    left = grey(bgr)
    if a.disparity == "matches":   # before this process opens the device: the child has it to itself
        with tempfile.TemporaryDirectory() as tmp:
            pair, out = os.path.join(tmp, "pair.npz"), os.path.join(tmp, "out.npz")
            np.savez(pair, left=left, right=right)
            subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gms_image_pair.py"), pair, "--out", out],
                                  stdout=subprocess.DEVNULL)
            disparity = np.load(out)["disparity"].astype(np.uint8)
    pkg = importlib.import_module("sfm-gms_amd")
    if a.disparity == "bm":
        disparity = pkg.stereo_match(left, right)
    elif a.disparity == "sgm":
        disparity = pkg.stereo_match_sgm(left, right)
    elif a.disparity != "matches":
        disparity = np.ascontiguousarray(np.load(a.disparity), dtype=np.uint8)
    kw = dict(threshold=a.threshold, dilate_iterations=a.dilate, num_contours=a.contours, median_ksize=a.ksize)
    t0 = time.perf_counter()
    out, mask, selected, blurred = pkg.portraitMode(bgr, disparity, detail=True, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    np.save(a.out, out)
    rec = {"size": f"{bgr.shape[1]}x{bgr.shape[0]}", "disparity": a.disparity, "with_value": round(float((disparity != 255).mean()), 4),
           "mask": round(float((mask != 0).mean()), 4), "selected": round(float((selected != 0).mean()), 4), "call_ms": round(ms, 3),
           "out": a.out}
    try:
        from PIL import Image
        png = os.path.splitext(a.out)[0] + ".png"
        Image.fromarray(np.ascontiguousarray(out[..., ::-1])).save(png)
        rec["png"] = png
    except ImportError:
        pass
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import portrait_ref
        want = portrait_ref.portrait(bgr, disparity, **kw)
        rec["equals_statement"] = all(g.tobytes() == want[n].tobytes() for n, g in
                                      (("out", out), ("mask", mask), ("selected", selected), ("blurred", blurred)))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
