#!/usr/bin/env python3
"""tools/detect_pyramid_bench.py -- the pyramid keypoint source (gms_detect_pyramid_batch_device) against the
single-scale call (gms_detect_batch_device) on the same resident images:

    python tools/detect_pyramid_bench.py [--frames 32] [--levels 8] [--warmup 3] [--iters 5] [--repeats 7] [--no-trace]
                                         [--out profiles/detect_pyramid_bench.json]

Images: the committed 1080p pair (tests/golden/image_main_scenario_1080p.npz) repeated to `frames` frames of 1920 x 1080, resident on
the device; threshold 20, 10 000 keypoints. After warm-up every repeat times `iters` calls with device events around them; the median
and the best repeat are reported for both calls, and their ratio. Unless --no-trace is given, the pyramid call is then run in a child
process under `rocprofv3 --kernel-trace --stats` (kernel tracing alone) and the per-kernel totals of that run, divided by its calls,
are reported as kernel_ms_per_call with the launches per call. One frame's result is checked against the single-scale call at
n_levels = 1 and, with --check, against the CPU statement tests/pyramid_ref.py."""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THRESHOLD, MAX_KEYPOINTS = 20, 10000


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


def child(args):
    """The pyramid call alone, `iters` times after one warm-up: what the kernel trace sees."""
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    d_imgs = frames(args.frames)
    run = batch.DetectPyramid(ctx, args.frames, 1920, 1080, THRESHOLD, MAX_KEYPOINTS, args.levels)
    for _ in range(1 + args.iters):
        run.run(d_imgs)
    ctx.synchronize()
    torch.cuda.synchronize()


def kernel_trace(args):
    """{kernel: [ms per call, launches per call]} from one rocprofv3 --kernel-trace --stats run of child()."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--frames", str(args.frames), "--levels", str(args.levels), "--iters", str(args.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not stats:
            return {"error": (r.stdout[-300:] + r.stderr[-300:]) or "no kernel_stats.csv"}
        calls = 1 + args.iters
        out = {}
        for row in csv.DictReader(open(stats[0])):
            if "gms::" not in row["Name"]:
                continue
            name = row["Name"].split("(")[0].split("gms::")[-1].replace("(anonymous namespace)::", "")
            total_ns = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["AverageNs"]) * int(row["Calls"])
            out[name] = [round(total_ns / calls * 1e-6, 4), round(int(row["Calls"]) / calls, 2)]
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    n, w, h = args.frames, 1920, 1080
    d_imgs = frames(n)
    sizes = ctx.pyramid_level_sizes(w, h, args.levels)
    run = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, args.levels)
    one = batch.DetectPyramid(ctx, n, w, h, THRESHOLD, MAX_KEYPOINTS, 1)
    nb = ctx.detect_workspace_bytes(w, h, n, MAX_KEYPOINTS)
    d_ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_levels = torch.zeros(n * sum(a * b for a, b in sizes[1:]) + 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def single():   # into the n_levels = 1 object's output buffers: the same bytes are expected there
        ctx.detect_batch_device(d_imgs.data_ptr(), n, w, h, THRESHOLD, MAX_KEYPOINTS, d_ws.data_ptr(), nb, one.d_kp.data_ptr(),
                                one.d_desc.data_ptr(), d_counts.data_ptr())

    t_single = timed(stream, single, args.warmup, args.iters, args.repeats)
    ctx.synchronize()
    kp_single, counts_single = one.d_kp.cpu().numpy().tobytes(), d_counts.cpu().numpy()
    t_one = timed(stream, lambda: one.run(d_imgs), args.warmup, args.iters, args.repeats)
    ctx.synchronize()
    same = one.d_kp.cpu().numpy().tobytes() == kp_single and np.array_equal(one.d_counts.cpu().numpy(), counts_single)
    t_pyr = timed(stream, lambda: run.run(d_imgs), args.warmup, args.iters, args.repeats)
    t_build = timed(stream, lambda: ctx.pyramid_build_device(d_imgs.data_ptr(), n, w, h, args.levels, d_levels.data_ptr(), d_levels.numel()),
                    args.warmup, args.iters, args.repeats)
    ctx.synchronize()
    kps, rows, lc = run.results()
    area = sum(a * b for a, b in sizes) / (w * h)
    rec = {"frames": n, "size": f"{w}x{h}", "threshold": THRESHOLD, "max_keypoints": MAX_KEYPOINTS, "n_levels": len(sizes),
           "level_sizes": sizes, "level_area_over_level0": round(area, 3),
           "single_scale_ms_median": round(t_single[0], 4), "single_scale_ms_best": round(t_single[1], 4),
           "pyramid_one_level_ms_median": round(t_one[0], 4),
           "pyramid_ms_median": round(t_pyr[0], 4), "pyramid_ms_best": round(t_pyr[1], 4),
           "pyramid_build_alone_ms_median": round(t_build[0], 4),
           "pyramid_over_single_scale": round(t_pyr[0] / t_single[0], 3),
           "frames_per_s_pyramid": round(n / t_pyr[0] * 1e3, 1), "frames_per_s_single_scale": round(n / t_single[0] * 1e3, 1),
           "keypoints_frame0_per_level": lc[0].tolist(), "keypoints_frame0_single_scale": int(counts_single[0]),
           "one_level_equals_single_scale": bool(same), "repeats": args.repeats, "iters": args.iters, "warmup": args.warmup}
    if args.check:
        sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
        import gms_oracle
        import pyramid_ref
        want = pyramid_ref.detect(gms_oracle, d_imgs[0].cpu().numpy(), THRESHOLD, MAX_KEYPOINTS, args.levels)
        rec["frame0_equals_cpu_statement"] = bool(want[0].tobytes() == kps[0].tobytes() and want[1].tobytes() == rows[0].tobytes())
    ctx.set_stream(None)
    if not args.no_trace:
        rec["kernel_ms_per_call"] = kernel_trace(args)
        rec["kernel_ms_per_call_note"] = "[ms per pyramid call summed over the levels, launches per call]; rocprofv3 --kernel-trace --stats, own run"
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
