#!/usr/bin/env python3
"""tools/stereo_bm_bench.py -- StereoBM block matching (gms_stereo_bm_device) with the reference's parameters:

    python tools/stereo_bm_bench.py [--warmup 3] [--iters 10] [--repeats 3] [--seed 1]

Two sizes: a batch of 16 pairs at 450 x 375 (the reference's disparity demo pair) and 4 pairs at 2594 x 1131 (its robot images).
Pairs are seeded synthetic images (smoothed noise, the right one shifted by a random disparity per pair), resident on the device.
After warm-up, each repeat times `iters` launches of the whole batch with device events; the table reports the best and the
median repeat: pairs/s and disparity evaluations/s (H * W * numDisparities per pair). One pair per size is checked byte for byte
against the one-shot gms_stereo_bm. Prints one JSON record per size."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pairs(rng, n, h, w):
    import torch
    lefts, rights = [], []
    for _ in range(n):
        base = rng.integers(0, 256, (h, w + 256)).astype(np.int32)
        base = (base + np.roll(base, 1, axis=1) + np.roll(base, 1, axis=0) + np.roll(base, -1, axis=1)) // 4
        s = int(rng.integers(10, 200))
        lefts.append(base[:, 256:])
        rights.append(np.clip(base[:, 256 - s:w + 256 - s] + rng.integers(-2, 3, (h, w)), 0, 255))
    return (torch.from_numpy(np.stack(lefts).astype(np.uint8)).cuda(), torch.from_numpy(np.stack(rights).astype(np.uint8)).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    nd = int(pkg.stereo_bm_params()["num_disparities"][0])
    for n, w, h in ((16, 450, 375), (4, 2594, 1131)):
        dl, dr = pairs(rng, n, h, w)
        run = batch.StereoBM(ctx, n, w, h)
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                run.run(dl, dr)
            stream.synchronize()
            times = []
            for _ in range(args.repeats):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(args.iters):
                    run.run(dl, dr)
                t1.record(stream)
                t1.synchronize()
                times.append(t0.elapsed_time(t1) / 1e3 / args.iters)
        one = pkg.stereoBM(dl[n - 1].cpu().numpy(), dr[n - 1].cpu().numpy())
        same = run.d_disp[n - 1].cpu().numpy().tobytes() == one.tobytes()
        best, med = min(times), float(np.median(times))
        print(json.dumps({"size": f"{w}x{h}", "pairs": n, "num_disparities": int(nd), "batch_ms_best": round(best * 1e3, 4),
                          "batch_ms_median": round(med * 1e3, 4), "pairs_per_s": round(n / best, 1),
                          "disparity_evals_per_s": float(f"{n * w * h * nd / best:.4g}"), "repeats_ms": [round(t * 1e3, 4) for t in times],
                          "one_shot_equal": same}), flush=True)
    ctx.set_stream(None)


if __name__ == "__main__":
    main()
