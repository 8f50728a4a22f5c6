#!/usr/bin/env python3
"""tools/sfm_pair_poses_bench.py -- pair records from views: gms_sfm_pair_poses_device alone at 7 and 999 pairs, and
gms_dense_pairs_device + gms_dense_fuse_device at 1008 x 756 with 4 pairs fed by those records, beside the same two calls fed by
hand-set two-view records and a registration (set_two_view / set_registration, the route without the stage), in one session.

    python tools/sfm_pair_poses_bench.py [--warmup 2] [--repeats 7] [--iters 20] [--seed 1] [--out profiles/sfm_pair_poses_bench.json]

tools/dense_fuse_bench.py's conditions: after `warmup` repeats, `repeats` repeats each time `iters` calls between two device events;
the median repeat is reported with the least and the largest. The dense pair: five cameras one baseline apart along x, R = I, seeded
noise images (the time does not depend on what they show), grey, num_disparities 128; the two routes hold the same poses, and their
repeats alternate, so that a drift of the clocks meets both. The kernels of the two routes are the same: the ratio says what run-to-run
spread is."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def repeat_ms(stream, fn, iters):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(iters):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def timed_all(stream, fns, warmup, iters, repeats):
    """Every fn's repeats, taken in turn (fn 0's repeat r, fn 1's repeat r, ...), after `warmup` untimed rounds."""
    import torch
    out = [[] for _ in fns]
    with torch.cuda.stream(stream):
        for r in range(warmup + repeats):
            for k, fn in enumerate(fns):
                ms = repeat_ms(stream, fn, iters)
                if r >= warmup:
                    out[k].append(ms)
    return out


def stats(times):
    return {"ms_median": round(float(np.median(times)), 5), "ms_min": round(min(times), 5), "ms_max": round(max(times), 5)}


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
    records = []
    for n_pairs in (7, 999):
        n_frames = 40
        views = np.zeros(n_frames, types.SFM_VIEW_DTYPE)
        for f in range(n_frames):
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            views["R"][f] = (Q if np.linalg.det(Q) > 0 else -Q).reshape(views["R"][f].shape)
            views["t"][f] = rng.uniform(-4, 4, 3)
        views["registered"] = 1
        a = rng.integers(0, n_frames, n_pairs)
        fp = np.stack([a, (a + rng.integers(1, n_frames, n_pairs)) % n_frames], 1)
        job = batch.pair_poses(ctx, views, fp)
        tv, _ = job.results()
        (t,) = timed_all(stream, [job.run], args.warmup, args.iters, args.repeats)
        rec = dict({"what": "sfm_pair_poses", "pairs": n_pairs, "frames": n_frames, "ok": int((tv["status"] == 0).sum())}, **stats(t))
        records.append(rec)
        print(json.dumps(rec), flush=True)
    w, h, n = 1008, 756, 4
    views = np.zeros(n + 1, types.SFM_VIEW_DTYPE)
    for f in range(n + 1):
        views["R"][f] = np.eye(3).reshape(views["R"][f].shape)
        views["t"][f] = (-float(f), 0.0, 0.0)
    views["registered"] = 1
    fp = [(i, i + 1) for i in range(n)]
    poses = batch.pair_poses(ctx, views, fp)
    tv, reg = poses.results()
    img = torch.from_numpy(rng.integers(0, 256, (n, h, w), dtype=np.uint8)).cuda()
    img2 = torch.roll(img, 20, dims=2).contiguous()
    cam = (0.8 * w, 0.8 * w, w / 2.0, h / 2.0)
    new = batch.DensePairs(ctx, n, (w, h), (w, h), cam, None, 1, views=poses.d_views, pose_records=poses)
    old = batch.DensePairs(ctx, n, (w, h), (w, h), cam, None, 1)
    old.set_two_view(tv)
    keep = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda() for x in (poses.recs, reg, views)]
    old.set_registration(keep[0], keep[1], keep[2], n + 1)
    torch.cuda.synchronize()
    for run in (new, old):
        run.run(img, img2)
    ctx.synchronize()
    fuse_new, fuse_old = batch.DenseFuse(ctx, [new]), batch.DenseFuse(ctx, [old])
    torch.cuda.synchronize()

    def route(run, fuse):
        def go():
            run.run(img, img2)
            fuse.run()
        return go
    route(new, fuse_new)()
    route(old, fuse_old)()
    ctx.synchronize()
    same = all(getattr(new, k).cpu().numpy().tobytes() == getattr(old, k).cpu().numpy().tobytes() for k in ("d_plans", "d_disp16", "d_xyz", "d_count")) \
        and all(getattr(fuse_new, k).cpu().numpy().tobytes() == getattr(fuse_old, k).cpu().numpy().tobytes() for k in ("d_xyz", "d_support", "d_counts"))
    t_new, t_old = timed_all(stream, [route(new, fuse_new), route(old, fuse_old)], args.warmup, max(args.iters // 4, 1), args.repeats)
    rec = {"what": "dense_pairs+dense_fuse", "pairs": n, "image": f"{w}x{h}", "num_disparities": 128, "same_bytes": bool(same),
           "fused_points": int(fuse_new.d_counts[-1]), "from_pose_records": stats(t_new), "from_set_records": stats(t_old),
           "ratio_of_medians": round(float(np.median(t_new) / np.median(t_old)), 4)}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    ctx.set_stream(None)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
