#!/usr/bin/env python3
"""tools/sfm_images_bench.py -- pipeline.run_images (the detector's blocks are packed and the tables built on the
device) against the route there was before it, over N resident frames of one size:

    before   batch.detect_images_pyramid -> keypoints and rows as host lists -> FrameTable / DescriptorTable (concatenate, upload) -> the stages
             (= pipeline.run_dataset on an io.Dataset of the lists)
    now      pipeline.run_images on the same resident frames

    python tools/sfm_images_bench.py [--frames 8] [--method gms] [--max-keypoints 10000] [--warmup 2] [--repeats 7] [--out profiles/sfm_images_bench.json]

Frames: the committed SfM pair (tests/golden/image_sfm_pair_1008x756.npz) repeated to `frames` frames, resident on the device; pairs
(i, i + 1); the pair's stated camera. Both routes are whole calls, host work included, timed with a wall clock between device
synchronisations; the median and the best of `repeats` calls after `warmup`. The record states both times, their ratio, the parts of
the earlier route (detector, readback of keypoints and rows, tables from the host lists, stages) with the share that was copies --
the readback plus the time to upload the same bytes again -- and whether the two routes returned the same records."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD, LEVELS = 20, 8


def clock(fn, sync, warmup, repeats):
    out, times = None, []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return out, {"median": round(float(np.median(times)), 3), "best": round(min(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--method", choices=("gms", "bf", "logos"), default="gms")
    ap.add_argument("--max-keypoints", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    io = importlib.import_module("sfm-gms_amd.io")
    z = np.load(os.path.join(ROOT, "tests", "golden", "image_sfm_pair_1008x756.npz"))
    pair = np.stack([z["left"], z["right"]])
    n = max(a.frames, 2)
    d_imgs = torch.from_numpy(np.concatenate([pair] * ((n + 1) // 2))[:n].copy()).cuda()
    h, w = pair.shape[1:]
    camera = tuple(float(v) for v in z["camera"])
    fp = [(i, i + 1) for i in range(n - 1)]
    recs = batch.pair_table(fp, 0)
    kw = dict(camera=camera, method=a.method, withRotation=True, withScale=True)
    if a.method == "logos":
        kw.update(train_dictionary=True)
    ctx = pkg.GmsContext(0)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def before():
        kps, rows, _ = batch.detect_images_pyramid(ctx, d_imgs, THRESHOLD, a.max_keypoints, LEVELS, descriptor="grad")
        return pipeline.run_dataset(ctx, io.Dataset(kps, [(w, h)] * n, rows, pkg.GMS_DESC_L2_F32X128, recs, None), **kw)

    def now():
        return pipeline.run_images(ctx, d_imgs, pairs=fp, threshold=THRESHOLD, max_keypoints=a.max_keypoints, n_levels=LEVELS, descriptor="grad", **kw)

    r0, t_before = clock(before, sync, a.warmup, a.repeats)
    r1, t_now = clock(now, sync, a.warmup, a.repeats)
    same = sorted(r0) == sorted(r1) and all(r0[k].tobytes() == r1[k].tobytes() for k in ("pairs", "out", "results", "mask"))
    same = same and all(np.abs(r0["two_view"][f] - r1["two_view"][f]).max() <= 1e-12 for f in ("E", "R", "t"))   # (sums that atomics may reorder)
    # the parts of the earlier route
    run = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, a.max_keypoints, LEVELS, descriptor="grad")
    _, t_detect = clock(lambda: run.run(d_imgs), sync, a.warmup, a.repeats)
    (kps, rows, _), t_readback = clock(run.results, sync, a.warmup, a.repeats)
    sizes = [(w, h)] * n

    def tables():
        f = batch.FrameTable(ctx, kps, sizes)
        return f, batch.DescriptorTable(ctx, f, rows, pkg.GMS_DESC_L2_F32X128)

    _, t_tables = clock(tables, sync, a.warmup, a.repeats)
    kp_all, rows_all = np.concatenate(kps), np.concatenate(rows)
    _, t_upload = clock(lambda: (batch._to_dev(kp_all, "cuda"), batch._to_dev(rows_all, "cuda")), sync, a.warmup, a.repeats)
    _, t_device_tables = clock(lambda: batch.tables_from_detector(run, sizes, pkg.GMS_DESC_L2_F32X128), sync, a.warmup, a.repeats)
    copies = t_readback["median"] + t_upload["median"]
    line = {"frames": n, "image": [int(w), int(h)], "pairs": len(fp), "method": a.method, "max_keypoints": a.max_keypoints,
            "keypoints": int(sum(len(k) for k in kps)), "survivors": int(r1["results"]["n_inliers"].sum()),
            "poses": int((r1["two_view"]["status"] == 0).sum()), "records_equal": bool(same),
            "before_ms": t_before, "run_images_ms": t_now, "ratio_median": round(t_before["median"] / t_now["median"], 3),
            "before_parts_ms": {"detector": t_detect, "readback_of_keypoints_and_rows": t_readback, "tables_from_host_lists": t_tables,
                                "upload_of_the_same_bytes": t_upload},
            "tables_from_detector_ms": t_device_tables, "copied_bytes_each_way": int(kp_all.nbytes + rows_all.nbytes),
            "copies_share_of_before": round(copies / t_before["median"], 3)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
