#!/usr/bin/env python3
"""tools/logos_dict_bench.py -- times the LOGOS dictionary trainer (gms_logos_dict_train_device):

    python tools/logos_dict_bench.py [--sets 1 32 256] [--rows 10000] [--words 50 100] [--kinds 0 1] [--repeats 7] [--warmup 1]
                                     [--max-iters 100] [--no-statement] [--no-kernels] [--trace-sets 32]
                                     [--out profiles/logos_dict_bench.json]

Per configuration: seeded sets of `rows` descriptor rows scattered around 2 * words centres, one call over all sets between device
events on the context's stream, the median and the spread of `repeats` calls after `warmup`, the iterations every set actually ran,
and the time of the numpy statement (tests/logos_dict_ref.py) on the first set, for scale (taken once per kind and word count, with
the smallest number of sets; --no-statement leaves it out). The call is one stream of launches, so its kernels are told apart by a
trace: per kind and word count, a child process runs one call over --trace-sets sets under
`rocprofv3 --kernel-trace --stats --output-format csv`, in a run of its own, and the calls and total / average time of every trainer
kernel go into the record ("kernels"; --no-kernels leaves the pass out, and a profiler that is missing or fails is reported there).

Writes one JSON record (also printed)."""
import argparse
import importlib
import json
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_sets(kind, n_sets, rows, words, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_sets):
        which = rng.integers(0, 2 * words, rows)
        if kind == 1:
            centres = rng.uniform(0, 160, (2 * words, 128)).astype(np.float32)
            out.append(np.clip(np.rint(centres[which] + rng.normal(0, 20, (rows, 128))), 0, 255).astype(np.float32))
        else:
            centres = rng.integers(0, 256, (2 * words, 32), dtype=np.uint8)
            out.append(centres[which] ^ np.packbits(rng.random((rows, 256)) < 0.15, axis=1))
    return out


def run_config(batch, ctx, torch, kind, n_sets, words, a):
    sets = make_sets(kind, n_sets, a.rows, words, 1000 * n_sets + words + kind)
    job = batch.LogosDictionary(ctx, kind, n_sets, n_sets * a.rows, words, 3, a.max_iters, seed=1)
    job.load(sets)
    s = torch.cuda.Stream(device=job.device)
    torch.cuda.synchronize(job.device)
    ctx.set_stream(s.cuda_stream)
    try:
        times = []
        for r in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            job.run()
            e1.record(s)
            e1.synchronize()
            if r >= a.warmup:
                times.append(e0.elapsed_time(e1))
    finally:
        ctx.set_stream(None)
    dic, rec, _ = job.results()
    rec_out = {"kind": "l2_f32x128" if kind == 1 else "hamming256", "sets": n_sets, "rows_per_set": a.rows, "words": words, "attempts": 3,
               "max_iters": a.max_iters, "workspace_bytes": job.ws_bytes, "call_ms_median": round(float(np.median(times)), 3),
               "call_ms_min": round(min(times), 3), "call_ms_max": round(max(times), 3), "repeats": len(times),
               "all_ok": bool((rec["status"] == 0).all()), "iterations": rec["iterations"].tolist(),
               "empty_clusters": int(rec["empty_clusters"].sum())}
    if not a.no_statement and n_sets == min(a.sets):
        import logos_dict_ref
        t0 = time.perf_counter()
        want = logos_dict_ref.train_set(sets[0], kind, words, 3, a.max_iters, seed=1, set_index=0)
        rec_out["statement_one_set_s"] = round(time.perf_counter() - t0, 3)
        rec_out["first_set_equals_statement"] = bool(want[0].tobytes() == dic[0].tobytes() and want[1].tobytes() == rec[0].tobytes())
    return rec_out


KERNELS = ("plan_kernel", "check_l2_kernel", "seed_update_kernel", "seed_pick_kernel", "seed_potential_kernel", "seed_commit_kernel",
           "assign_l2_kernel", "assign_hamming_kernel", "update_kernel", "finish_kernel")


def kernel_trace(kind, words, a):
    """One call over a.trace_sets sets in a child process under the profiler -> {kernel: {calls, total_ms, average_us}}."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not found"}
    out_dir = tempfile.mkdtemp(prefix="logos_dict_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable,
               os.path.abspath(__file__), "--sets", str(a.trace_sets), "--rows", str(a.rows), "--words", str(words), "--kinds", str(kind),
               "--repeats", "1", "--warmup", "0", "--max-iters", str(a.max_iters), "--no-statement", "--no-kernels", "--out", ""]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.trace_timeout)
        if res.returncode != 0:
            return {"error": f"profiler run failed ({res.returncode}): {res.stderr[-300:]}"}
        found = {}
        for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k + "E" in row["Name"] or k + "(" in row["Name"]:   # mangled or demangled
                            found[k] = {"calls": int(row["Calls"]), "total_ms": round(int(row["TotalDurationNs"]) / 1e6, 3),
                                        "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
        return {"sets": a.trace_sets, "kernels": found} if found else {"error": "no trainer kernel in the profiler's statistics"}
    except (subprocess.TimeoutExpired, OSError, KeyError, ValueError) as e:
        return {"error": f"{type(e).__name__}: {e}"}
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--words", type=int, nargs="+", default=[50, 100])
    ap.add_argument("--kinds", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-iters", type=int, default=100)
    ap.add_argument("--no-statement", action="store_true", help="do not time the numpy statement")
    ap.add_argument("--no-kernels", action="store_true", help="no per-kernel pass under the profiler")
    ap.add_argument("--trace-sets", type=int, default=32, help="sets of the per-kernel pass")
    ap.add_argument("--trace-timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logos_dict_bench.json"))
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    configs = []
    with pkg.GmsContext(0) as ctx:
        for kind in a.kinds:
            for words in a.words:
                for n_sets in a.sets:
                    configs.append(run_config(batch, ctx, torch, kind, n_sets, words, a))
                    print(json.dumps(configs[-1]), file=sys.stderr, flush=True)
    out = {"tool": "logos_dict_bench", "device": torch.cuda.get_device_name(0), "configs": configs}
    if not a.no_kernels:   # after the context is closed: the child opens the device itself
        out["kernels"] = [dict(kind="l2_f32x128" if kind == 1 else "hamming256", words=words, rows_per_set=a.rows,
                               **kernel_trace(kind, words, a)) for kind in a.kinds for words in a.words]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if all(c["all_ok"] for c in configs) else 1


if __name__ == "__main__":
    sys.exit(main())
