#!/usr/bin/env python3
"""tools/calib_bench.py -- gms_chess_candidates_device on the ten committed calibration photographs:

    python tools/calib_bench.py [--warmup 2] [--repeats 7] [--iters 20] [--out profiles/calib_bench.json]

Two batches resident on the device: the ten 1008 x 756 images of tests/golden/image_calib_{a..e}.npz, and the same ten tiled 2 x 2 to
2016 x 1512 (the size of the photographs as taken). After `warmup` repeats, `repeats` repeats each time `iters` calls between two
device events; the median repeat is reported (and the best). hbm_share is the least time the memory system could take for the
algorithmic bytes -- one byte per pixel in; the candidate records out are negligible -- at PEAK_HBM_BYTES_PER_S, over the measured
time. The call itself moves more: it writes R once (4 bytes per pixel) and reads it once for the peaks, 9 bytes per pixel in all."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM_BYTES_PER_S = 8.0e12    # MI355X: 8 TB/s


def timed(stream, fn, warmup, iters, repeats):
    import torch
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            for _ in range(iters):
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ims = np.concatenate([np.load(os.path.join(ROOT, "tests", "golden", f"image_calib_{t}.npz"))["images"] for t in "abcde"])
    records = []
    for name, stack in (("fixture", ims), ("tiled_2x2", np.tile(ims, (1, 2, 2)))):
        n, h, w = stack.shape
        d = torch.from_numpy(np.ascontiguousarray(stack)).cuda()
        run = batch.ChessCorners(ctx, n, w, h, 256)
        torch.cuda.synchronize()
        med, best = timed(stream, lambda: run.run(d), args.warmup, args.iters, args.repeats)
        peaks = [len(c) for c in run.candidates()]
        nbytes = n * w * h
        rec = {"what": name, "call": "gms_chess_candidates_device", "batch": n, "image": f"{w}x{h}", "max_candidates": 256,
               "candidates_min": min(peaks), "ms_median": round(med, 5), "ms_best": round(best, 5), "algorithmic_bytes": nbytes,
               "gbytes_per_s": round(nbytes / (med * 1e-3) / 1e9, 1), "hbm_share": round(nbytes / PEAK_HBM_BYTES_PER_S / (med * 1e-3), 4),
               "moved_bytes": 9 * nbytes, "hbm_share_of_moved_bytes": round(9 * nbytes / PEAK_HBM_BYTES_PER_S / (med * 1e-3), 4)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del run, d
    ctx.set_stream(None)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
