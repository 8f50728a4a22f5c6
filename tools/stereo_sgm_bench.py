#!/usr/bin/env python3
"""tools/stereo_sgm_bench.py -- semi-global matching (gms_stereo_sgm_device) beside StereoBM (gms_stereo_bm_device) on
the committed pairs, written to profiles/stereo_sgm_bench.json:

    python tools/stereo_sgm_bench.py [--warmup 2] [--repeats 7] [--iters 5] [--out profiles/stereo_sgm_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/stereo_sgm_bench.py --trace CONFIG
    python tools/stereo_sgm_bench.py --merge CONFIG=DIR/..._kernel_stats.csv [CONFIG=...]      (no device needed)

Configurations: the 450 x 375 pair and the 1920 x 1080 pair of tests/golden, each with the reference's parameters (224 disparities from
-39) and with 64 disparities from 0 without the texture rule, in batches of 1 and 8 (the pair and copies of it turned upside down,
resident on the device). Each repeat times `iters` launches of gms_stereo_sgm_device and then `iters` of gms_stereo_bm_device with
device events, so the two alternate in one session; after `warmup` repeats the medians of `repeats` repeats are reported, and their
ratio SGM / BM. One batch per size is checked byte for byte against the one-shot gms_stereo_sgm.

--trace runs one configuration three times without timing, for a kernel trace in a run of its own. --merge reads such a trace's
kernel statistics and adds, per kernel, its average time, and for the two forms of the aggregation kernel their algorithmic bytes (C
read once; S written by the first direction, read and written by the others), the rate they give and its share of the HBM peak
(8.0 TB/s)."""
import argparse
import csv
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
HBM_PEAK = 8.0e12
SIZES = {"450x375": "image_stereo_pair_450x375.npz", "1920x1080": "image_main_scenario_1080p.npz"}
PARAMS = {"reference": {}, "nd64": dict(num_disparities=64, min_disparity=0, texture_threshold=0)}


def configs():
    return {f"{size}_{pname}_n{n}": (size, pname, n) for size in SIZES for pname in PARAMS for n in (1, 8)}


def region(w, h, kw):
    """(ny, wx, nd, n_paths) of a configuration: the pixels the volumes cover (stereo_bm_core.h's geometry)."""
    types = importlib.import_module("sfm-gms_amd.types")
    p = types.stereo_sgm_params(kw)
    nd, md, w2 = int(p["num_disparities"][0]), int(p["min_disparity"][0]), int(p["block_size"][0]) // 2
    lofs, rofs = max(nd - 1 + md, 0), -min(nd - 1 + md, 0)
    width1 = w - rofs - nd + 1
    return h - 2 * w2, min(width1, w - lofs), nd, int(p["n_paths"][0])


def load(size, n):
    z = np.load(os.path.join(GOLDEN, SIZES[size]))
    left, right = z["left"], z["right"]
    lefts = np.stack([left if i % 2 == 0 else left[::-1] for i in range(n)])
    rights = np.stack([right if i % 2 == 0 else right[::-1] for i in range(n)])
    return np.ascontiguousarray(lefts), np.ascontiguousarray(rights)


def merge(out, items):
    rec = json.load(open(out))
    for item in items:
        name, path = item.split("=", 1)
        size, pname, n = configs()[name]
        w, h = (int(v) for v in size.split("x"))
        ny, wx, nd, _ = region(w, h, PARAMS[pname])
        vol = 2 * n * ny * wx * nd
        kernels = {}
        for row in csv.DictReader(open(path)):
            short = next((k for k in ("sbm_prefilter_kernel", "sgm_cost_kernel", "sgm_path_kernel", "sgm_decide_kernel", "sbm_validate_kernel")
                          if k in row["Name"]), None)
            if not short:
                continue
            k = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
            if short == "sgm_path_kernel":     # <R, true>: the first direction reads C and writes S; <R, false>: the others also read S
                first = ", true>" in row["Name"]
                short += "_first" if first else "_later"
                nbytes = vol * (2 if first else 3)
                rate = nbytes / (k["average_us"] * 1e-6)
                k.update(algorithmic_bytes_per_launch=nbytes, bytes_per_s=float(f"{rate:.4g}"), share_of_hbm_peak=round(rate / HBM_PEAK, 4))
            kernels[short] = k
        rec.setdefault("kernel_trace", {})[name] = kernels
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec.get("kernel_trace", {})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_sgm_bench.json"))
    ap.add_argument("--trace", default=None, choices=sorted(configs()))
    ap.add_argument("--merge", nargs="+", default=None)
    args = ap.parse_args()
    if args.merge:
        return merge(args.out, args.merge)
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    records = []
    for name, (size, pname, n) in configs().items():
        if args.trace and name != args.trace:
            continue
        kw = PARAMS[pname]
        lefts, rights = load(size, n)
        h, w = lefts.shape[1:]
        dl, dr = torch.from_numpy(lefts).cuda(), torch.from_numpy(rights).cuda()
        sgm, bm = batch.StereoSGM(ctx, n, w, h, kw), batch.StereoBM(ctx, n, w, h, kw)
        with torch.cuda.stream(stream):
            if args.trace:
                for _ in range(3):
                    sgm.run(dl, dr)
                stream.synchronize()
                continue
            times = {"sgm": [], "bm": []}
            for _ in range(args.warmup + args.repeats):
                for key, run in (("sgm", sgm), ("bm", bm)):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    for _ in range(args.iters):
                        run.run(dl, dr)
                    t1.record(stream)
                    t1.synchronize()
                    times[key].append(t0.elapsed_time(t1) / args.iters)
        ny, wx, nd, n_paths = region(w, h, kw)
        ms = {k: float(np.median(v[args.warmup:])) for k, v in times.items()}
        rec = {"config": name, "size": size, "params": pname, "pairs": n, "num_disparities": nd, "n_paths": n_paths, "region": [ny, wx],
               "workspace_bytes": sgm.ws_bytes, "sgm_ms_median": round(ms["sgm"], 4), "bm_ms_median": round(ms["bm"], 4),
               "ratio_sgm_over_bm": round(ms["sgm"] / ms["bm"], 2), "sgm_repeats_ms": [round(t, 4) for t in times["sgm"][args.warmup:]],
               "bm_repeats_ms": [round(t, 4) for t in times["bm"][args.warmup:]]}
        if n == 1 and pname == "reference":
            one = pkg.stereoSGM(lefts[0], rights[0], **kw)
            rec["one_shot_equal"] = sgm.d_disp[0].cpu().numpy().tobytes() == one.tobytes()
        records.append(rec)
        print(json.dumps(rec), flush=True)
        del sgm, bm, dl, dr
        torch.cuda.empty_cache()
    ctx.set_stream(None)
    if not args.trace:
        json.dump({"tool": "tools/stereo_sgm_bench.py", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
                   "iters": args.iters, "configs": records}, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
