#!/usr/bin/env python3
"""tools/dog_bench.py -- the pyramid keypoint source with the difference-of-Gaussians detector (gms_detect_dog_batch_device; DESIGN.md
§4.7d) against the same call with the FAST detector (gms_detect_pyramid_grad_batch_device), same build, same session, same resident images:

    python tools/dog_bench.py [--frames 8] [--levels 8] [--warmup 2] [--iters 5] [--repeats 7] [--refine] [--check] [--out profiles/dog_bench.json]

Images: the committed 1080p pair (tests/golden/image_main_scenario_1080p.npz) repeated to `frames` frames of 1920 x 1080, resident on
the device; descriptor "both", 10 000 keypoints, FAST threshold 20, DoG contrast 128. After warm-up every repeat times `iters` calls with
device events around them; the median and the best repeat are reported for both calls and their ratio. The candidate kernel alone is
timed through gms_dog_candidates_device on the same frames (level 0; that entry point skips the box sums and the histogram, so it
writes 1 of the 3 bytes per pixel), and its share of an 8 TB/s roofline is stated on the full call's algorithmic bytes (1 B in, 3 B out
per pixel) as an upper bound. --refine: gms_detect_dog_refined_batch_device is timed in the same session as well, and the ratio of its
median to the unrefined DoG call's is reported. --check compares one frame's keypoints and rows with the CPU statement
tests/dog_ref.py (the refined call's with tests/dog_refine_ref.py)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD, CONTRAST, MAX_KEYPOINTS = 20, 128, 10000
ROOFLINE_BYTES_PER_S = 8e12


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
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    d_imgs = frames(a.frames)
    n, h, w = d_imgs.shape
    fast = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, a.levels, descriptor="both")
    dog = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, a.levels, descriptor="both", detector="dog", contrast=CONTRAST)
    fine = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, a.levels, descriptor="both", detector="dog", contrast=CONTRAST,
                               refine=True) if a.refine else None
    d_cand = torch.zeros((n, h, w), dtype=torch.uint8, device=d_imgs.device)
    fast.run(d_imgs)
    dog.run(d_imgs)
    ctx.synchronize()
    kp_fast = fast.results()[0]
    kp_dog, rows32, rows128, lc = dog.results()
    line = {"frames": n, "image": [w, h], "levels": a.levels, "descriptor": "both", "threshold": THRESHOLD, "contrast": CONTRAST,
            "max_keypoints": MAX_KEYPOINTS, "keypoints_per_frame": {"fast": float(np.mean([len(k) for k in kp_fast])),
                                                                    "dog": float(np.mean([len(k) for k in kp_dog]))},
            "dog_level_counts_frame0": lc[0].tolist()}
    ok = True
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gms_oracle as oracle
        import dog_ref
        want = dog_ref.detect(oracle, d_imgs[0].cpu().numpy(), CONTRAST, MAX_KEYPOINTS, a.levels)
        ok = bool(want[0].tobytes() == kp_dog[0].tobytes() and want[1].tobytes() == rows32[0].tobytes() and want[3].tobytes() == rows128[0].tobytes()
                  and want[2].tolist() == lc[0].tolist())
        line["equals_statement"] = ok
        if fine is not None:
            import dog_refine_ref
            fine.run(d_imgs)
            ctx.synchronize()
            got = fine.results()
            want = dog_refine_ref.detect(oracle, d_imgs[0].cpu().numpy(), CONTRAST, MAX_KEYPOINTS, a.levels)
            same = bool(want[0].tobytes() == got[0][0].tobytes() and want[1].tobytes() == got[1][0].tobytes() and want[3].tobytes() == got[2][0].tobytes()
                        and want[2].tolist() == got[3][0].tolist())
            line["refined_equals_statement"] = same
            line["refined_records_that_differ_frame0"] = int((got[0][0] != kp_dog[0]).sum())
            ok = ok and same
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        runs = [("fast", lambda: fast.run(d_imgs)), ("dog", lambda: dog.run(d_imgs)),
                ("dog_candidates_level0", lambda: ctx.dog_candidates_device(d_imgs.data_ptr(), n, w, h, CONTRAST, d_cand.data_ptr()))]
        if fine is not None:
            runs += [("dog_refined", lambda: fine.run(d_imgs)), ("dog_again", lambda: dog.run(d_imgs))]   # (the unrefined call on both sides of it)
        for name, fn in runs:
            med, best = timed(stream, fn, a.warmup, a.iters, a.repeats)
            line[name + "_ms"] = {"median": round(med, 4), "best": round(best, 4)}
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
    line["ratio_median_dog_over_fast"] = round(line["dog_ms"]["median"] / line["fast_ms"]["median"], 4)
    if fine is not None:
        line["ratio_median_dog_refined_over_dog"] = round(line["dog_refined_ms"]["median"] / line["dog_ms"]["median"], 4)
    kernel_s = line["dog_candidates_level0_ms"]["median"] * 1e-3
    line["dog_maps_kernel_us_per_frame_level0"] = round(kernel_s * 1e6 / n, 3)
    line["dog_maps_kernel_roofline_share_4B_per_pixel"] = round(4.0 * n * w * h / kernel_s / ROOFLINE_BYTES_PER_S, 4)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
