#!/usr/bin/env python3
"""The three feature-match scenarios of the reference's main() (main.cpp:28-47) from two photographs, on the GPU
(pipeline.run_main_scenarios): the pair as it is, the right image turned (img_rotate) and the right image resized (cv::resize), each
matched by bruteForceMatch and by matchGMS(withRotation, withScale).

    python tools/gms_main_scenarios.py [pair.npz] [--resize 1000x1000] [--angle 180] [--keypoints 10000] [--threshold 20] [--detector fast|dog] [--contrast 128] [--refine] [--check]

pair.npz holds `left` and `right`, equally sized [H, W] or [H, W, 3] (default: tests/golden/image_main_scenario_1080p.npz). Prints the
scenario table, one JSON line per scenario and method. --check compares the transformed images with tests/warp_ref.py."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pair", nargs="?", default=os.path.join(ROOT, "tests", "golden", "image_main_scenario_1080p.npz"))
    ap.add_argument("--resize", default="1000x1000")
    ap.add_argument("--angle", type=float, default=180.0)
    ap.add_argument("--keypoints", type=int, default=10000)
    ap.add_argument("--threshold", type=int, default=20)
    ap.add_argument("--detector", choices=("fast", "dog"), default="fast")
    ap.add_argument("--contrast", type=int, default=128)
    ap.add_argument("--refine", action="store_true", help="with --detector dog: keypoints refined to 1/16 pixel and 1/16 layer")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.refine and a.detector != "dog":
        ap.error("--refine needs --detector dog")
    z = np.load(a.pair)
    left, right = np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])
    resize_to = tuple(int(v) for v in a.resize.lower().split("x"))
    pkg = importlib.import_module("sfm-gms_amd")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    ctx = pkg.GmsContext(0)
    t0 = time.perf_counter()
    r = pipeline.run_main_scenarios(ctx, left, right, resize_to=resize_to, angle=a.angle, threshold=a.threshold, max_keypoints=a.keypoints,
                                    detector=a.detector, contrast=a.contrast, refine=a.refine)
    ms = (time.perf_counter() - t0) * 1e3
    counts = np.diff(r["tables"][0].frame_off_host).tolist()
    for k, name in enumerate(pipeline.MAIN_SCENARIOS, start=1):
        for method in ("bf", "gms"):
            res = r[name][method]["results"][0]
            rec = {"scenario": name, "method": method, "size2": "%dx%d" % r["sizes"][k], "keypoints": [counts[0], counts[k]],
                   "kept": int(res["n_inliers"]), "status": int(res["status"])}
            if method == "gms":
                rec.update(putative=int(r[name][method]["pairs"]["m"][0]), best_rot=int(res["best_rot"]), best_scale=int(res["best_scale"]))
            print(json.dumps(rec), flush=True)
    tail = {"call_ms": round(ms, 3)}
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import warp_ref
        tail["equals_statement"] = bool(np.array_equal(r["images"]["rotated"], warp_ref.img_rotate(right, a.angle)) and
                                        np.array_equal(r["images"]["resized"], warp_ref.resize(right, resize_to)))
    print(json.dumps(tail), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
