#!/usr/bin/env python3
"""tools/warp_bench.py -- gms_resize_device / gms_warp_affine_device and pipeline.run_main_scenarios:

    python tools/warp_bench.py [--warmup 2] [--repeats 7] [--iters 20] [--seed 1] [--no-scenarios] [--out profiles/warp_bench.json]

Per kernel, on seeded noise images resident on the device, at batch 1 and batch 32:
    resize        1920 x 1080 x 3 -> 1000 x 1000            (the linear kernel)
    area          2016 x 1512 -> 1008 x 756, one channel     (the 2 x 2 mean)
    rotate180     img_rotate(180) of 1920 x 1080 x 3
    rotate30      img_rotate(30) of 1920 x 1080 x 3
After `warmup` repeats, `repeats` repeats each time `iters` calls between two device events; the median repeat is reported (and the
best). hbm_share is the least time the memory system could take for the algorithmic bytes -- every source byte once plus every
destination byte once -- at PEAK_HBM_BYTES_PER_S, over the measured time. At batch 1 the images fit the caches, so that figure is a
share of a bound the call never meets; batch 32 is the one that streams.
Whole call, single-session wall clock (host timer around calls that end in a synchronise; median of `repeats` after `warmup`), on
tests/golden/image_main_scenario_1080p.npz: run_main_scenarios against the route tests/test_gpu_main_scenario.py takes to the same
three scenarios -- flip on the host, PIL's bilinear resize (numpy striding when PIL is absent), upload, then two separate runs:
run_images over the three equally sized images (both methods), and the host-list route for the resized pair (detect_images_pyramid per
image -> FrameTable / DescriptorTable -> match_pairs -> filter_pairs, and bf_select_pairs). The two routes do not see the same pixels
(PIL samples differently, the flip lacks warpAffine's one-pixel shift): the ratio compares time, not results."""
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


def wall(fn, warmup, repeats):
    times = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-scenarios", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    records = []
    cases = (("resize", (1920, 1080), 3, (1000, 1000), None), ("area", (2016, 1512), 1, (1008, 756), None),
             ("rotate180", (1920, 1080), 3, (1920, 1080), 180.0), ("rotate30", (1920, 1080), 3, (1920, 1080), 30.0))
    for name, (sw, sh), ch, (dw, dh), angle in cases:
        for n in (1, 32):
            src = torch.from_numpy(rng.integers(0, 256, (n, sh, sw) + ((3,) if ch == 3 else ()), dtype=np.uint8)).cuda()
            run = batch.Warp(ctx, n, (sw, sh), (dw, dh), ch, 1)
            if angle is not None:
                run.set_matrices(pkg.getRotationMatrix2D((sw / 2., sh / 2.), angle, 1.0))
            torch.cuda.synchronize()
            fn = (lambda: run.resize(src)) if angle is None else (lambda: run.warp_affine(src))
            med, best = timed(stream, fn, args.warmup, args.iters, args.repeats)
            nbytes = n * ch * (sw * sh + dw * dh)
            rec = {"what": name, "kernel": "warp_affine" if angle is not None else ("resize_area2" if name == "area" else "resize_linear"),
                   "batch": n, "src": f"{sw}x{sh}x{ch}", "dst": f"{dw}x{dh}", "ms_median": round(med, 5), "ms_best": round(best, 5),
                   "algorithmic_bytes": nbytes, "gbytes_per_s": round(nbytes / (med * 1e-3) / 1e9, 1),
                   "hbm_share": round(nbytes / PEAK_HBM_BYTES_PER_S / (med * 1e-3), 4)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del run, src
    ctx.set_stream(None)
    if not args.no_scenarios:
        z = np.load(os.path.join(ROOT, "tests", "golden", "image_main_scenario_1080p.npz"))
        left, right = np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])
        try:
            from PIL import Image
            shrink, how = (lambda im: np.asarray(Image.fromarray(im).resize((1000, 1000), Image.BILINEAR))), "PIL"
        except ImportError:
            shrink, how = (lambda im: np.ascontiguousarray(im[np.arange(1000) * im.shape[0] // 1000][:, np.arange(1000) * im.shape[1] // 1000])), "numpy striding"

        def device_route():
            pipeline.run_main_scenarios(ctx, left, right, resize_to=(1000, 1000), angle=180)

        def host_route():
            flipped, small = np.ascontiguousarray(right[::-1, ::-1]), np.ascontiguousarray(shrink(right))
            images = np.stack([left, right, flipped])
            for method in ("bf", "gms"):
                pipeline.run_images(ctx, images, method=method, pairs=[(0, 1), (0, 2)], withRotation=True, withScale=True)
            det = [batch.detect_images_pyramid(ctx, im[None], 20, 10000, 8, descriptor="grad") for im in (left, small)]
            kps, rows = [d[0][0] for d in det], [d[1][0] for d in det]
            table = batch.FrameTable(ctx, kps, [(left.shape[1], left.shape[0]), (1000, 1000)])
            dt = batch.DescriptorTable(ctx, table, rows, pkg.GMS_DESC_L2_F32X128)
            pairs = np.zeros(1, dtype=pkg.PAIR_DTYPE)
            pairs[0] = (0, 1, len(kps[0]), 0, 0)
            matches = batch.match_pairs(ctx, dt, pairs)
            batch.filter_pairs(ctx, table, pairs, matches, True, True, 6.0)
            batch.bf_select_pairs(ctx, dt, np.array([[0, 1]], dtype=np.int64))

        dev_med, dev_best = wall(device_route, args.warmup, args.repeats)
        host_med, host_best = wall(host_route, args.warmup, args.repeats)
        rec = {"what": "run_main_scenarios", "images": "1920x1080 grey pair", "host_resize": how, "device_route_ms_median": round(dev_med, 2),
               "device_route_ms_best": round(dev_best, 2), "host_route_ms_median": round(host_med, 2), "host_route_ms_best": round(host_best, 2),
               "host_over_device": round(host_med / dev_med, 3), "clock": "single-session wall clock"}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
