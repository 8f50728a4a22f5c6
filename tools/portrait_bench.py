#!/usr/bin/env python3
"""tools/portrait_bench.py -- portrait mode (gms_portrait_device) with the reference's parameters:

    python tools/portrait_bench.py [--warmup 3] [--iters 5] [--repeats 7] [--seed 1] [--no-cpu] [--out profiles/portrait_bench.json]

Sizes: the reference's robot photograph, 2594 x 1131 x 3, as a batch of 1 and of 16, and 1920 x 1080 as a batch of 1. Inputs are
seeded and resident on the device: noise photographs and three kinds of disparity map, each with a tenth of the pixels without value:
    figure   one ellipse in front (about a quarter of the image) and a few small blobs: a portrait's foreground share
    blobs    smoothed-noise blobs at level 0.5, which the dilation joins into one border around most of the image
    noisy    independent pixels, 5 % in front: after the dilation one ragged component with long chains (the one-lane walks' bad case)
Every record carries selected_fraction, the share of pixels that keep the photograph and skip the median search, because the call's
time depends on it. After warm-up every repeat times `iters` calls with device events (median and best repeat): the call without
the optional outputs, the call with all of them (every pixel's median is computed: the upper figure), and gms_median_blur_device
alone. Per kernel: gms_portrait_profile_device puts a device event between the launches; the median over `repeats` such calls of
each kernel's time is reported (stage_ms). The median-plus-composite kernel's share of the HBM roofline is taken on its algorithmic
bytes, 3 W H read + 3 W H written + W H of mask per image, against PEAK_HBM_BYTES_PER_S, with its time in the all-outputs profile.
As a sanity line, not a gate: tests/portrait_ref.py's vectorised median of one full-size image on the host, timed once."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_HBM_BYTES_PER_S = 8.0e12    # MI355X: 8 TB/s


def inputs(rng, kind, n, h, w):
    import torch
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if kind == "noisy":
        front = rng.random((n, h, w)) < 0.05
    else:
        a = rng.random((n, h // 8 + 2, w // 8 + 2))
        a = (a + np.roll(a, 1, 1) + np.roll(a, 1, 2) + np.roll(a, -1, 1) + np.roll(a, -1, 2)) / 5
        a = np.repeat(np.repeat(a, 8, axis=1), 8, axis=2)[:, :h, :w]
        if kind == "blobs":
            front = a > 0.5
        else:
            yy, xx = np.mgrid[:h, :w]
            front = (((yy - 0.55 * h) / (0.42 * h)) ** 2 + ((xx - 0.5 * w) / (0.19 * w)) ** 2 < 1)[None] | (a > 0.62)
    disp = np.where(front, 120, 20).astype(np.uint8)
    disp[rng.random((n, h, w)) < 0.1] = 255
    return torch.from_numpy(img).cuda(), torch.from_numpy(disp).cuda()


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    records = []
    stages = ctx.PORTRAIT_STAGES
    for kind, n, w, h in (("figure", 1, 2594, 1131), ("figure", 16, 2594, 1131), ("figure", 1, 1920, 1080), ("blobs", 1, 2594, 1131),
                          ("blobs", 16, 2594, 1131), ("noisy", 1, 2594, 1131)):
        di, dd = inputs(rng, kind, n, h, w)
        lean = batch.Portrait(ctx, n, w, h, detail=False)
        full = batch.Portrait(ctx, n, w, h, detail=True)
        d_blur = torch.zeros_like(di)
        k = int(lean.params["median_ksize"][0])

        def profile(run, optional):
            ptrs = [t.data_ptr() for t in (run.d_mask, run.d_selected, run.d_blurred)] if optional else [None] * 3
            ms = [ctx.portrait_profile_device(run.params, di.data_ptr(), dd.data_ptr(), n, w, h, 3 * w, w, run.d_ws.data_ptr(),
                                              run.ws_bytes, run.d_out.data_ptr(), *ptrs) for _ in range(1 + args.repeats)]
            return np.median(np.stack(ms[1:]), axis=0)

        call = timed(stream, lambda: lean.run(di, dd), args.warmup, args.iters, args.repeats)
        call_full = timed(stream, lambda: full.run(di, dd), args.warmup, args.iters, args.repeats)
        med = timed(stream, lambda: ctx.median_blur_device(di.data_ptr(), n, w, h, 3, 3 * w, k, d_blur.data_ptr()), args.warmup,
                    args.iters, args.repeats)
        st_lean, st_full = profile(lean, False), profile(full, True)
        ctx.synchronize()
        same = full.d_blurred.cpu().numpy().tobytes() == d_blur.cpu().numpy().tobytes()
        bytes_alg = n * 7 * w * h
        rec = {"map": kind, "size": f"{w}x{h}x3", "batch": n, "median_ksize": k,
               "selected_fraction": round(float((full.d_selected != 0).float().mean()), 4),
               "call_ms_median": round(call[0], 4), "call_ms_best": round(call[1], 4),
               "call_all_outputs_ms_median": round(call_full[0], 4), "call_all_outputs_ms_best": round(call_full[1], 4),
               "images_per_s": round(n / call[0] * 1e3, 2), "images_per_s_all_outputs": round(n / call_full[0] * 1e3, 2),
               "stage_ms": {s: round(float(v), 4) for s, v in zip(stages, st_lean)},
               "stage_ms_all_outputs": {s: round(float(v), 4) for s, v in zip(stages, st_full)},
               "median_blur_device_ms_median": round(med[0], 4), "median_blur_device_ms_best": round(med[1], 4),
               "median_kernel_algorithmic_bytes": bytes_alg, "peak_hbm_bytes_per_s": PEAK_HBM_BYTES_PER_S,
               "median_kernel_hbm_roofline_fraction": float(f"{bytes_alg / (float(st_full[-1]) * 1e-3) / PEAK_HBM_BYTES_PER_S:.4g}"),
               "blurred_equals_median_alone": same, "repeats": args.repeats, "iters": args.iters, "warmup": args.warmup}
        if not args.no_cpu and n == 1 and w == 2594 and kind == "figure":
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import portrait_ref
            host = di[0].cpu().numpy()
            t0 = time.perf_counter()
            ref = portrait_ref.median_blur(host, k)
            rec["cpu_statement_median_s_once"] = round(time.perf_counter() - t0, 2)
            rec["cpu_statement_equal"] = ref.tobytes() == d_blur[0].cpu().numpy().tobytes()
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del lean, full, di, dd, d_blur
    ctx.set_stream(None)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
