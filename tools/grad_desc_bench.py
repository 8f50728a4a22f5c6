#!/usr/bin/env python3
"""tools/grad_desc_bench.py -- the pyramid keypoint source with the gradient descriptor's rows (gms_detect_pyramid_grad_batch_device;
DESIGN.md §4.7c) against the same call without them (gms_detect_pyramid_batch_device) at the same arguments, on the same resident images:

    python tools/grad_desc_bench.py [--frames 32] [--levels 8] [--warmup 3] [--iters 5] [--repeats 7] [--out profiles/grad_desc_bench.json]

Images: the committed 1080p pair (tests/golden/image_main_scenario_1080p.npz) repeated to `frames` frames of 1920 x 1080, resident on
the device; threshold 20, 10 000 keypoints. After warm-up every repeat times `iters` calls with device events around them; the median
and the best repeat are reported for both calls, their ratio, and the difference per keypoint. Before timing, keypoints, 32-byte rows and
counts of the two calls are compared, and with --check one frame's 128-float rows against the CPU statement tests/grad_desc_ref.py."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD, MAX_KEYPOINTS = 20, 10000


def frames(n):
    import torch
    z = np.load(os.path.join(ROOT, "tests", "golden", "image_main_scenario_1080p.npz"))
    pair = np.stack([z["left"], z["right"]])
    return torch.from_numpy(np.concatenate([pair] * ((n + 1) // 2))[:n].copy()).cuda()


def timed(stream, fn, warmup, iters, repeats):
    import torch
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        stream.synchronize()
        times = []
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(iters):
                fn()
            t1.record(stream)
            t1.synchronize()
            times.append(t0.elapsed_time(t1) / iters)
    return float(np.median(times)), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    d_imgs = frames(a.frames)
    n, h, w = d_imgs.shape
    plain = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, a.levels)
    grad = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, a.levels, descriptor="both")
    plain.run(d_imgs)
    grad.run(d_imgs)
    ctx.synchronize()
    kp0, rows0, lc0 = plain.results()
    kp1, rows1, rows128, lc1 = grad.results()
    same = lc0.tobytes() == lc1.tobytes() and all(kp0[i].tobytes() == kp1[i].tobytes() and rows0[i].tobytes() == rows1[i].tobytes() for i in range(n))
    line = {"frames": n, "image": [w, h], "levels": a.levels, "threshold": THRESHOLD, "max_keypoints": MAX_KEYPOINTS,
            "keypoints_per_frame": float(np.mean([len(k) for k in kp0])), "other_outputs_equal": bool(same)}
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gms_oracle as oracle
        import grad_desc_ref
        want = grad_desc_ref.detect(oracle, d_imgs[0].cpu().numpy(), THRESHOLD, MAX_KEYPOINTS, a.levels)
        line["rows_equal_statement"] = bool(want[0].tobytes() == kp1[0].tobytes() and want[3].tobytes() == rows128[0].tobytes())
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        for name, run in (("pyramid", plain), ("pyramid_grad", grad)):
            med, best = timed(stream, lambda: run.run(d_imgs), a.warmup, a.iters, a.repeats)
            line[name + "_ms"] = {"median": round(med, 4), "best": round(best, 4)}
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
    line["ratio_median"] = round(line["pyramid_grad_ms"]["median"] / line["pyramid_ms"]["median"], 4)
    total_kp = sum(len(k) for k in kp0)
    line["added_us_per_keypoint"] = round((line["pyramid_grad_ms"]["median"] - line["pyramid_ms"]["median"]) * 1e3 / max(total_kp, 1), 5)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
    ctx.close()
    return 0 if same and line.get("rows_equal_statement", True) else 1


if __name__ == "__main__":
    sys.exit(main())
