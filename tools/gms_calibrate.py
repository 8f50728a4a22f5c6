#!/usr/bin/env python3
"""The reference's camera calibration (main.cpp:53-68: addChessboardPoints, then calibrateCamera) on chessboard photographs
(pipeline.calibrate_images): prints one JSON line with K, the distortion and the RMS reprojection error.

    python tools/gms_calibrate.py [IMAGES.npz ...] [--board 6 9] [--check] [--out camera.npz]

IMAGES.npz: an array `images`, uint8 [n, H, W] grey or [n, H, W, 3] BGR (several files of one image size are joined); default: the
committed halves of the reference's ten CalibrationImages, tests/golden/image_calib_a.npz .. image_calib_e.npz. --out writes camera =
(fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3), K, rms, image_size: a file tools/gms_sfm_pair.py --camera accepts. --check (grey
images): runs the CPU statement (tests/calib_ref.py) beside it and compares candidates, corners and calibration; test infrastructure."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="*", default=[os.path.join(GOLDEN, f"image_calib_{t}.npz") for t in "abcde"])
    ap.add_argument("--board", type=int, nargs=2, default=(6, 9), metavar=("NX", "NY"))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = importlib.import_module("sfm-gms_amd")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    ims = np.concatenate([np.ascontiguousarray(np.load(p)["images"], dtype=np.uint8) for p in a.images])
    nx, ny = a.board
    ctx = pkg.GmsContext(0)
    r = pipeline.calibrate_images(ctx, ims, (nx, ny))
    ctx.close()
    line = {"images": len(ims), "image": [int(ims.shape[2]), int(ims.shape[1])], "board": [nx, ny], "found": [bool(v) for v in r["found"]]}
    if r["K"] is None:
        print(json.dumps(line))
        return 1
    line.update({"camera": [round(v, 4) for v in r["camera"]], "dist": [round(float(v), 6) for v in r["dist"]], "rms_px": round(r["rms"], 5)})
    ok = True
    if a.check:
        if ims.ndim != 3:
            ap.error("--check restates grey images")
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import calib_ref
        pts, same = [], True
        for i, im in enumerate(ims):
            cand = calib_ref.candidates(im)
            same = same and cand.tobytes() == r["candidates"][i].tobytes()
            found, o = calib_ref.order_board(np.stack([cand["x"][:nx * ny], cand["y"][:nx * ny]], 1), nx, ny) if len(cand) >= nx * ny else (False, None)
            same = same and found == bool(r["found"][i])
            if found:
                pts.append(calib_ref.corner_subpix(im, o))
        ref = calib_ref.calibrate_camera([calib_ref.object_points(nx, ny)] * len(pts), pts, (ims.shape[2], ims.shape[1]))
        chk = {"candidates_and_found": bool(same), "corners_1e-9": bool(len(pts) == len(r["image_points"]) and np.abs(np.array(pts) - r["image_points"]).max() < 1e-9),
               "K_1e-4": bool(np.abs(ref["K"] - r["K"]).max() < 1e-4), "rms_1e-6": bool(abs(ref["rms"] - r["rms"]) < 1e-6)}
        line["check_vs_cpu"] = chk
        line["cpu"] = {"camera": [round(float(ref["K"][0, 0]), 4), round(float(ref["K"][1, 1]), 4), round(float(ref["K"][0, 2]), 4), round(float(ref["K"][1, 2]), 4)],
                       "rms_px": round(ref["rms"], 5)}
        ok = all(chk.values())
    if a.out:
        np.savez(a.out, camera=np.array(r["camera"]), dist=np.asarray(r["dist"]), K=r["K"], rms=np.array(r["rms"]),
                 image_size=np.array([ims.shape[2], ims.shape[1]], np.int32))
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
