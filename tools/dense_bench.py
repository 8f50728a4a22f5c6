#!/usr/bin/env python3
"""tools/dense_bench.py -- the dense stage of a posed pair: gms_rectify_device beside gms_warp_affine_device, the
parent's nearest kernel (another bilinear byte gather), and gms_dense_pairs_device split into plan, rectify, matcher and cloud.

    python tools/dense_bench.py [--warmup 2] [--repeats 7] [--iters 20] [--seed 1] [--out profiles/dense_bench.json]

Per image size (1008 x 756, 1920 x 1080), channel count (1, 3) and batch (1, 8), on seeded noise images resident on the device, a pose
of 5 degrees with a slanted baseline and all five distortion coefficients set: after `warmup` repeats, `repeats` repeats each time
`iters` calls between two device events; the median repeat is reported (and the best). hbm_share is the least time the memory system
could take for the algorithmic bytes -- every source byte once plus every destination byte once (the valid plane included) -- at
PEAK_HBM_BYTES_PER_S, over the measured time. The stage's parts are timed each on its own with the same events, on grey 1080p
pairs at batch 1, num_disparities 128."""
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


def rot(axis, degrees):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
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
    R, t, dist = rot((0.3, 1.0, 0.2), 5.0), np.array([-1.0, 0.25, 0.05]), (0.05, -0.02, 0.001, -0.002, 0.01)
    records = []
    for (w, h) in ((1008, 756), (1920, 1080)):
        cam = (0.8 * w, 0.8 * w, w / 2.0, h / 2.0)
        plan = pkg.stereoRectify(cam, dist, R, t, (w, h))
        assert plan.ok
        for ch in (1, 3):
            for n in (1, 8):
                src = torch.from_numpy(rng.integers(0, 256, (n, h, w) + ((3,) if ch == 3 else ()), dtype=np.uint8)).cuda()
                rect = batch.Rectify(ctx, n, (w, h), (w, h), types.make_camera(cam, dist), ch, 1)
                rect.set_plans(plan)
                warp = batch.Warp(ctx, n, (w, h), (w, h), ch, 1)
                warp.set_matrices(pkg.getRotationMatrix2D((w / 2., h / 2.), 5.0, 1.0))
                torch.cuda.synchronize()
                for name, fn, extra in (("rectify", lambda: rect.run(src, 1), n * w * h), ("warp_affine", lambda: warp.warp_affine(src), 0)):
                    med, best = timed(stream, fn, args.warmup, args.iters, args.repeats)
                    nbytes = 2 * n * ch * w * h + extra
                    rec = {"what": name, "batch": n, "image": f"{w}x{h}x{ch}", "ms_median": round(med, 5), "ms_best": round(best, 5),
                           "ms_per_image": round(med / n, 5), "algorithmic_bytes": nbytes, "gbytes_per_s": round(nbytes / (med * 1e-3) / 1e9, 1),
                           "hbm_share": round(nbytes / PEAK_HBM_BYTES_PER_S / (med * 1e-3), 4)}
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
                del rect, warp, src
    # the stage's parts on a grey 1080p pair
    w, h = 1920, 1080
    cam = (0.8 * w, 0.8 * w, w / 2.0, h / 2.0)
    img = torch.from_numpy(rng.integers(0, 256, (1, h, w), dtype=np.uint8)).cuda()
    img2 = torch.roll(img, 20, dims=2).contiguous()
    run = batch.DensePairs(ctx, 1, (w, h), (w, h), cam, dist, 1)
    tv = np.zeros(1, types.TWO_VIEW_DTYPE)
    tv["R"][0], tv["t"][0] = R, t
    run.set_two_view(tv)
    torch.cuda.synchronize()
    camrec = run.camera
    sgm_ws = ctx.stereo_sgm_workspace_bytes(w, h, 1, run.params)
    cloud_ws = ctx.dense_cloud_workspace_bytes(w, h, 1)
    d_ws = torch.zeros(max(sgm_ws, cloud_ws), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    parts = (
        ("plan", lambda: ctx.rectify_plan_device(camrec, run.d_tv.data_ptr(), 1, w, h, w, h, run.d_plans.data_ptr())),
        ("rectify_two_grey", lambda: (ctx.rectify_device(camrec, img.data_ptr(), 1, w, h, 1, w, run.d_plans.data_ptr(), 1, 1, run.d_rect1.data_ptr(), w, h, w,
                                                         run.d_valid.data_ptr()),
                                      ctx.rectify_device(camrec, img2.data_ptr(), 1, w, h, 1, w, run.d_plans.data_ptr(), 1, 2, run.d_rect2.data_ptr(), w, h, w))),
        ("sgm", lambda: ctx.stereo_sgm_device(run.params, run.d_rect1.data_ptr(), run.d_rect2.data_ptr(), 1, w, h, w, d_ws.data_ptr(), sgm_ws,
                                              run.d_disp16.data_ptr())),
        ("cloud", lambda: ctx.dense_cloud_device(run.d_disp16.data_ptr(), run.d_valid.data_ptr(), run.d_rect1.data_ptr(), 1, w, 1, w, h,
                                                 run.d_plans.data_ptr(), -16, 16, d_ws.data_ptr(), cloud_ws, run.cap, run.d_xyz.data_ptr(),
                                                 run.d_cloud_color.data_ptr(), run.d_pixel.data_ptr(), run.d_count.data_ptr())),
        ("whole_stage", lambda: run.run(img, img2)),
    )
    for name, fn in parts:
        med, best = timed(stream, fn, args.warmup, max(args.iters // 4, 1), args.repeats)
        rec = {"what": "stage_" + name, "image": f"{w}x{h}x1", "batch": 1, "num_disparities": 128, "ms_median": round(med, 5), "ms_best": round(best, 5)}
        if name == "whole_stage":
            rec["points"] = int(run.d_count[0])
        records.append(rec)
        print(json.dumps(rec), flush=True)
    ctx.set_stream(None)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
