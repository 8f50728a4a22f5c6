#!/usr/bin/env python3
"""tools/dense_fuse_bench.py -- the fusion of per-pair dense clouds: gms_dense_fuse_device on the clouds of 2, 4 and
8 pairs, beside gms_dense_pairs_device, the stage that feeds it, at the same image size and number of pairs.

    python tools/dense_fuse_bench.py [--warmup 2] [--repeats 7] [--iters 20] [--seed 1] [--out profiles/dense_fuse_bench.json]

Per image size (1008 x 756, 1920 x 1080) and number of pairs: the sources are a chain of cameras one baseline apart along x, all
looking along z at a slanted plane about 12 baselines away; each pair's int16 map is the plane's disparity plus seeded noise of at most
3 sixteenths, with 3 % of the pixels filtered, so that most lookups hit and agree. Every other source is a neighbour. After `warmup`
repeats, `repeats` repeats each time `iters` calls between two device events; the median repeat is reported (and the best).
hbm_share: the least time the memory system could take for the mark kernel's algorithmic bytes -- 12 bytes per point read, 3 bytes per
point and live neighbour gathered -- at PEAK_HBM_BYTES_PER_S, over the time of the whole call (mark, scan and write kernels), so it
understates the mark kernel's own share. dense_pairs: the whole dense stage on seeded noise images of the same size and batch, grey,
num_disparities 128 (the time does not depend on what the images show)."""
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


def chain_sources(torch, types, rng, n, w, h):
    """n sources as batch.DenseFuse takes them: camera i at x = i, R = I; plane 0.1 x + 0.05 y + z = 12."""
    f, cx, cy = 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0
    plan = np.zeros(1, types.RECTIFY_PLAN_DTYPE)
    plan["R1"][0], plan["R2"][0] = np.eye(3), np.eye(3)
    plan["fx"], plan["fy"], plan["cx"], plan["cy"], plan["B"], plan["out_w"], plan["out_h"] = f, f, cx, cy, 1.0, w, h
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rx, ry = (u - cx) / f, (v - cy) / f
    out = []
    for i in range(n):
        z = (12.0 - 0.1 * i) / (0.1 * rx + 0.05 * ry + 1.0)             # the plane along the rays of a camera at (i, 0, 0)
        d16 = np.rint(f * 16.0 / z).astype(np.int64) + rng.integers(-3, 4, (h, w))
        d16[rng.random((h, w)) < 0.03] = -16
        d16 = d16.astype(np.int16)
        ok = d16 >= 16
        zc = f * 16.0 / d16[ok].astype(np.float64)
        xyz = np.stack([(u[ok] - cx) * zc / f + i, (v[ok] - cy) * zc / f, zc], axis=1).astype(np.float32)   # world = camera 0's frame
        view = np.zeros(1, types.SFM_VIEW_DTYPE)
        view["R"][0], view["t"][0], view["registered"] = np.eye(3), (-float(i), 0.0, 0.0), 1
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out.append(dict(d_disp16=dev(d16), d_valid=dev(np.ones((h, w), np.uint8)), d_plan=dev(plan.view(np.uint8).reshape(-1)), d_xyz=dev(xyz),
                        d_color=dev(rng.integers(0, 256, (len(xyz), 1), dtype=np.uint8)),
                        d_count=torch.tensor([len(xyz)], dtype=torch.int32, device="cuda"), d_view=dev(view.view(np.uint8).reshape(-1))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sizes", default="1008x756,1920x1080")
    ap.add_argument("--pairs", default="2,4,8")
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
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for n in (int(v) for v in args.pairs.split(",")):
            srcs = chain_sources(torch, types, rng, n, w, h)
            job = batch.DenseFuse(ctx, srcs)
            torch.cuda.synchronize()
            job.run()
            res = job.result()
            points = int(sum(int(s["d_count"][0]) for s in srcs))
            med, best = timed(stream, job.run, args.warmup, args.iters, args.repeats)
            nbytes = 12 * points + 3 * points * (n - 1)
            rec = {"what": "dense_fuse", "pairs": n, "image": f"{w}x{h}", "points_in": points, "points_out": int(res["counts"][-1]),
                   "support_histogram": {str(k): int(c) for k, c in enumerate(np.bincount(res["support"])) if c},
                   "ms_median": round(med, 5), "ms_best": round(best, 5), "algorithmic_bytes": nbytes,
                   "gbytes_per_s": round(nbytes / (med * 1e-3) / 1e9, 1), "hbm_share": round(nbytes / PEAK_HBM_BYTES_PER_S / (med * 1e-3), 4)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del job, srcs
            img = torch.from_numpy(rng.integers(0, 256, (n, h, w), dtype=np.uint8)).cuda()
            img2 = torch.roll(img, 20, dims=2).contiguous()
            run = batch.DensePairs(ctx, n, (w, h), (w, h), (0.8 * w, 0.8 * w, w / 2.0, h / 2.0), None, 1)
            tv = np.zeros(n, types.TWO_VIEW_DTYPE)
            tv["R"], tv["t"] = np.eye(3), (-1.0, 0.0, 0.0)
            run.set_two_view(tv)
            torch.cuda.synchronize()
            med, best = timed(stream, lambda: run.run(img, img2), args.warmup, max(args.iters // 4, 1), args.repeats)
            rec = {"what": "dense_pairs", "pairs": n, "image": f"{w}x{h}", "num_disparities": 128, "ms_median": round(med, 5), "ms_best": round(best, 5)}
            records.append(rec)
            print(json.dumps(rec), flush=True)
            del run, img, img2
            torch.cuda.empty_cache()
    ctx.set_stream(None)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
