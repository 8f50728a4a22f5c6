#!/usr/bin/env python3
"""tools/speckle_bench.py -- the speckle filter: gms_filter_speckles_device with (max_speckle_size, max_diff) =
(100, 32) on four kinds of int16 maps, beside the two yardsticks the library already had: gms_stereo_sgm_device, the stage the filter
sits behind, and the labelling kernels of portrait mode (init + merge + flatten of gms_portrait_profile_device), the only other
connected-component labelling in the library. Also gms_dense_pairs_filtered_device beside gms_dense_pairs_device on a grey pair.

    python tools/speckle_bench.py [--warmup 2] [--repeats 7] [--iters 20] [--seed 1] [--sizes 1008x756,1920x1080] [--batches 1,8]
                                  [--maps plane,noise,constant,serpentine] [--no-yardsticks] [--no-dense]
                                  [--out profiles/speckle_bench.json]

Maps: plane -- a slanted plane's disparity plus noise of at most 3 sixteenths, 3 % filtered (the fusion bench's map); noise --
independent values, so nearly every pixel is a component of its own; constant -- one component; serpentine -- a one-pixel-wide
snake through the whole map, the longest chain. The filter works in place, so every timed call is preceded by a device copy that
restores the map; that copy is timed alone and subtracted (ms = ms_with_restore - ms_restore). After `warmup` repeats, `repeats`
repeats each time `iters` calls between two device events; the median repeat is reported (and the best).
hbm_share: 4 algorithmic bytes per pixel (2 read, 2 written) at PEAK_HBM_BYTES_PER_S over the call's time.
Yardstick (b): the mask is the same map thresholded (plane: at the median of its values; noise: at the 95th percentile, 5 % in front,
which keeps portrait mode's one-lane border walks short); the ratio compares init + merge + flatten only."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from warp_bench import PEAK_HBM_BYTES_PER_S, timed  # noqa: E402

NEW_VAL, SIZE, DIFF = -16, 100, 32


def make_map(kind, rng, w, h):
    if kind == "plane":
        f, cx, cy = 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0
        u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        z = 12.0 / (0.1 * (u - cx) / f + 0.05 * (v - cy) / f + 1.0)
        d = np.rint(f * 16.0 / z).astype(np.int64) + rng.integers(-3, 4, (h, w))
        d[rng.random((h, w)) < 0.03] = NEW_VAL
        return d.astype(np.int16)
    if kind == "noise":
        return rng.integers(0, 2048, (h, w)).astype(np.int16) * 16
    if kind == "constant":
        return np.full((h, w), 640, np.int16)
    if kind == "serpentine":
        d = np.full((h, w), NEW_VAL, np.int16)
        d[0::2, :] = 640
        d[1::4, w - 1] = 640
        d[3::4, 0] = 640
        return d
    raise ValueError(kind)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sizes", default="1008x756,1920x1080")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--maps", default="plane,noise,constant,serpentine")
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    types = importlib.import_module("sfm-gms_amd.types")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(args.seed)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:                       # after every record: a run that is cut short leaves what it measured
            with open(args.out, "w") as f:
                json.dump(records, f, indent=1)

    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for n in (int(v) for v in args.batches.split(",")):
            yard = {}
            if not args.no_yardsticks:
                img = torch.from_numpy(rng.integers(0, 256, (n, h, w), dtype=np.uint8)).cuda()
                img2 = torch.roll(img, 20, dims=2).contiguous()
                sgm = batch.StereoSGM(ctx, n, w, h, with_cost=False)
                torch.cuda.synchronize()
                med, best = timed(stream, lambda: sgm.run(img, img2), args.warmup, max(args.iters // 4, 1), args.repeats)
                yard["sgm_ms"] = med
                emit({"what": "stereo_sgm", "image": f"{w}x{h}", "batch": n, "ms_median": round(med, 5), "ms_best": round(best, 5)})
                del sgm, img, img2
                torch.cuda.empty_cache()
            for kind in args.maps.split(","):
                one = make_map(kind, rng, w, h)
                src = torch.from_numpy(np.stack([one] * n)).cuda()
                d = src.clone()
                job = batch.SpeckleFilter(ctx, n, (w, h))
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    job.run(d, NEW_VAL, SIZE, DIFF)
                stream.synchronize()
                removed = int(job.d_removed[0])

                def call():
                    d.copy_(src)
                    job.run(d, NEW_VAL, SIZE, DIFF)

                both = timed(stream, call, args.warmup, args.iters, args.repeats)
                copy = timed(stream, lambda: d.copy_(src), args.warmup, args.iters, args.repeats)
                ms = both[0] - copy[0]
                px = n * w * h
                rec = {"what": "filter_speckles", "map": kind, "image": f"{w}x{h}", "batch": n, "removed_per_map": removed,
                       "ms_with_restore": round(both[0], 5), "ms_restore": round(copy[0], 5), "ms": round(ms, 5),
                       "ms_best": round(both[1] - copy[0], 5), "ns_per_pixel": round(ms * 1e6 / px, 4),
                       "hbm_share": round(4 * px / PEAK_HBM_BYTES_PER_S / (ms * 1e-3), 4)}
                if "sgm_ms" in yard:
                    rec["ratio_to_sgm"] = round(ms / yard["sgm_ms"], 4)
                if not args.no_yardsticks and kind in ("plane", "noise"):
                    cut = np.median(one[one != NEW_VAL]) if kind == "plane" else np.percentile(one, 95)
                    mask8 = torch.from_numpy(np.stack([np.where(one > cut, 200, 0).astype(np.uint8)] * n)).cuda()
                    bgr = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
                    pm = batch.Portrait(ctx, n, w, h, dict(threshold=60, dilate_iterations=0, num_contours=1, median_ksize=3), detail=False)
                    torch.cuda.synchronize()
                    prof = [ctx.portrait_profile_device(pm.params, bgr.data_ptr(), mask8.data_ptr(), n, w, h, 3 * w, w, pm.d_ws.data_ptr(),
                                                        pm.ws_bytes, pm.d_out.data_ptr()) for _ in range(1 + args.repeats)]
                    st = np.median(np.stack(prof[1:]), axis=0)
                    lab = float(sum(st[ctx.PORTRAIT_STAGES.index(k)] for k in ("init", "merge", "flatten")))
                    rec.update(portrait_label_ms=round(lab, 5), ratio_to_portrait_label=round(ms / lab, 4))
                    del pm, bgr, mask8
                emit(rec)
                del job, d, src
                torch.cuda.empty_cache()
    # the dense stage with and without the filter: a grey 1080p pair, batch 1
    w, h = 1920, 1080
    if args.no_dense:
        ctx.set_stream(None)
        ctx.close()
        return
    img = torch.from_numpy(rng.integers(0, 256, (1, h, w), dtype=np.uint8)).cuda()
    img2 = torch.roll(img, 20, dims=2).contiguous()
    tv = np.zeros(1, types.TWO_VIEW_DTYPE)
    tv["R"], tv["t"] = np.eye(3), (-1.0, 0.0, 0.0)
    for speckle in (None, (SIZE, DIFF)):
        run = batch.DensePairs(ctx, 1, (w, h), (w, h), (0.8 * w, 0.8 * w, w / 2.0, h / 2.0), None, 1, speckle=speckle)
        run.set_two_view(tv)
        torch.cuda.synchronize()
        med, best = timed(stream, lambda: run.run(img, img2), args.warmup, max(args.iters // 4, 1), args.repeats)
        emit({"what": "dense_pairs_filtered" if speckle else "dense_pairs", "image": f"{w}x{h}", "batch": 1, "num_disparities": 128,
              "speckle": speckle, "ms_median": round(med, 5), "ms_best": round(best, 5)})
        del run
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
