#!/usr/bin/env python3
"""tools/sfm_ba_bench.py -- what bundle adjustment costs beside the stages in front of it: on the two chains of
tools/sfm_register_bench.py, the bundle adjustment call (gms_sfm_ba_device through batch.SfmBundle), the registration
(gms_sfm_register_device) and the two-view stage (gms_two_view_batch_device) of the same session on the same pairs.

    python tools/sfm_ba_bench.py [--workload small|long|both] [--warmup 2] [--repeats 7] [--out profiles/sfm_ba_bench.json]
                                 [--all-work] [--kernel-stats STATS.csv] [--counters COUNTERS.csv]

    small   8 frames, 7 chain pairs, 3000 keypoints per frame: about 3000 survivors per pair
    long    1000 frames, 999 chain pairs, 10000 keypoints per frame

Each time is a host clock around one call that ends in a synchronisation of the context's stream: the median and the best of `repeats`
calls after `warmup`. The keypoints carry half a pixel of noise, so that there is something to refine. The record also states the
launches per call (12 + n_iters (8 + 3 n_cg), whatever the flags on the device turn into no-ops) and, for the two kernels that run
once per conjugate-gradient iteration, the bytes their algorithm has to move: per observation of a used track sqrt(w) Jc and
sqrt(w) Jp (18 doubles), the track and frame of its keypoint (two int32), and per track or frame the small vectors.
--all-work runs with cg_tol = 0, ftol = 0, n_iters = 3 and n_cg = 20, so that no launch is a no-op: the shape to run under a kernel
trace. --kernel-stats: the kernel statistics (CSV with Name, Calls, TotalDurationNs columns) of such a traced run, `{workload}` in the
path standing for the workload's name (profiles/sfm_ba_kernel_stats_{workload}.csv are the committed ones); the record then states the two kernels' mean time and their share of the HBM roofline (--hbm-gbps, 8000 by default) on those bytes, and names the
traced run's parameters. --counters: per workload and kernel the sums of a counter run of its own in the same shape (`rocprofv3 --pmc
GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU TCC_HIT_sum
TCC_MISS_sum`, no tracing beside it; columns workload, kernel, counter, sum_over_dispatches, dispatches: profiles/sfm_ba_pmc.csv is
the committed one); the record then states where the waves' cycles go, the L2 hit rate and which bound that suggests."""
import argparse
import csv
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sfm_register_bench import WORKLOADS, clock  # noqa: E402


def run(name, ctx, mods, a):
    import torch
    pkg, batch, synth, types = mods
    w = WORKLOADS[name]
    n, n_kp = w["n_frames"], w["n_kp"]
    sc = synth.make_multi_view_scene(31, min(n, 8), size=w["size"], n_kp=n_kp, camera=w["camera"], noise_px=0.5)
    frames = batch.FrameTable(ctx, [sc["frames"][f % 8] for f in range(n)], [w["size"]] * n)
    pairs = batch.pair_table([(i, i + 1) for i in range(n - 1)], n_kp)
    n_pairs, total = len(pairs), (n - 1) * n_kp
    rng = np.random.default_rng(3)
    m = np.zeros(total, pkg.DMATCH_DTYPE)
    m["queryIdx"] = np.tile(np.arange(n_kp), n_pairs)
    t = m["queryIdx"].copy()
    bad = rng.choice(total, total // 10, replace=False)
    t[bad] = rng.integers(0, n_kp, len(bad))
    m["trainIdx"] = t
    res = np.zeros(n_pairs, pkg.RESULT_DTYPE)
    res["n_inliers"], res["best_scale"], res["best_rot"] = n_kp, -1, -1
    dev = frames.device
    d_pairs, d_out, d_res = batch._to_dev(pairs, dev), batch._to_dev(m, dev), batch._to_dev(res, dev)
    d_c1, d_c2 = (torch.zeros(total * 2, dtype=torch.float32, device=dev) for _ in range(2))
    d_mask = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_p3 = torch.zeros(total * 3, dtype=torch.float64, device=dev)
    d_tv = torch.zeros(n_pairs * types.TWO_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    cam = types.make_camera(w["camera"])

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def two_view():
        ctx.two_view_batch_device(cam, frames.d_kp.data_ptr(), frames.d_frame_off.data_ptr(), n, d_pairs.data_ptr(), n_pairs, n_kp, d_out.data_ptr(),
                                  d_res.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), d_mask.data_ptr(), d_p3.data_ptr(), d_tv.data_ptr(), 0.7, 1.0, 1000)

    ba = dict(n_iters=3, n_cg=20, cg_tol=0.0, ftol=0.0) if a.all_work else {}
    reg = batch.SfmRegister(ctx, frames.frame_off_host, pairs, d_frame_off=frames.d_frame_off, d_pairs=d_pairs)
    job = batch.SfmBundle(ctx, frames.frame_off_host, pairs, reg.cloud_cap, w["camera"], d_frame_off=frames.d_frame_off, d_pairs=d_pairs, **ba)
    t_tv = clock(two_view, sync, a.warmup, a.repeats)
    t_reg = clock(lambda: reg.run(d_out, d_mask, d_p3, d_tv), sync, a.warmup, a.repeats)
    t_ba = clock(lambda: job.run(reg, frames.d_kp, d_out, d_mask), sync, a.warmup, a.repeats)
    s = job.results()["ba_summary"][0]
    prm = job.params[0]
    n_obs, n_tracks, n_free = int(s["n_obs"]), int(s["n_tracks_used"]), int(s["n_frames_free"])
    # per CG iteration: the per-track pass reads Jc, Jp (18 doubles) and the keypoint's frame per observation, the list entry, p of
    # its frame (cached: counted once per frame), V^-1 per track, and writes q_t; the per-frame pass reads Jc, Jp and the keypoint's
    # track per observation, q_t per observation, U and p per frame, and writes q_f and its share of p.q
    track_bytes = n_obs * (18 * 8 + 4 + 4) + n_tracks * (9 * 8 + 3 * 8 + 8) + n_free * 6 * 8
    frame_bytes = n_obs * (18 * 8 + 4 + 3 * 8) + n_free * (36 * 8 + 6 * 8 + 6 * 8 + 8)
    line = {"frames": n, "pairs": n_pairs, "keypoints_per_frame": n_kp, "match_slots": total, "workspace_bytes": job.ws_bytes,
            "params": {k: (float(prm[k]) if prm[k].dtype.kind == "f" else int(prm[k])) for k in ("n_iters", "n_cg", "lambda0", "cg_tol", "ftol",
                                                                                             "huber_px", "retriangulate")},
            "launches_per_call": 12 + int(prm["n_iters"]) * (8 + 3 * int(prm["n_cg"])),
            "observations": n_obs, "tracks_used": n_tracks, "tracks_with_two_keypoints_of_a_frame": int(s["n_tracks_multi"]), "free_frames": n_free,
            "iterations_run": int(s["iters_run"]), "iterations_accepted": int(s["iters_accepted"]), "cg_iterations": int(s["cg_iters"]),
            "rms_px": [round(float(s["rms0_px"]), 4), round(float(s["rms_px"]), 4)],
            "bundle_ms": t_ba, "register_ms": t_reg, "two_view_ms": t_tv, "bundle_over_two_view": round(t_ba["median"] / t_tv["median"], 4),
            "cg_track_kernel_bytes": track_bytes, "cg_frame_kernel_bytes": frame_bytes}
    if a.kernel_stats:
        with open(a.kernel_stats.format(workload=name), newline="") as f:
            rows = list(csv.DictReader(f))
        line["kernel_figures_from"] = ("a kernel trace of its own, not this run: --all-work (n_iters 3, n_cg 20, cg_tol 0, ftol 0, one call, so "
                                       "that each of its 60 launches of either kernel does work); the times above and `params` are this run's")
        for key, nbytes in (("sba_cg_track_kernel", track_bytes), ("sba_cg_frame_kernel", frame_bytes)):
            hit = [r for r in rows if key in r["Name"]]
            if hit:
                ns = float(hit[0]["TotalDurationNs"]) / float(hit[0]["Calls"])
                line[key] = {"mean_us": round(ns / 1e3, 2), "gbps": round(nbytes / ns, 1), "share_of_hbm_roofline": round(nbytes / ns / a.hbm_gbps, 4)}
    if a.counters:
        with open(a.counters, newline="") as f:
            vals = {(r["kernel"], r["counter"]): float(r["sum_over_dispatches"]) for r in csv.DictReader(f) if r["workload"] == name}
        for key in ("sba_cg_track_kernel", "sba_cg_frame_kernel"):
            wave = vals.get((key, "SQ_WAVE_CYCLES"))
            if not wave:
                continue
            parked, stalled, issuing = (vals[(key, c)] / wave for c in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"))
            valu = vals[(key, "SQ_ACTIVE_INST_VALU")] / wave
            hit = vals[(key, "TCC_HIT_sum")] / (vals[(key, "TCC_HIT_sum")] + vals[(key, "TCC_MISS_sum")])
            line.setdefault(key, {})["counters"] = {
                "from": "a counter run of its own (--pmc alone, --all-work), summed over 60 dispatches", "wave_cycles_parked_on_a_wait": round(parked, 3),
                "wave_cycles_stalled_at_issue": round(stalled, 3), "wave_cycles_issuing": round(issuing, 3), "wave_cycles_issuing_valu": round(valu, 3),
                "l2_hit_rate": round(hit, 3),
                "bound_suggested": "memory" if parked + stalled > 0.8 and valu < 0.1 else ("compute" if valu > 0.5 else "mixed")}
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("small", "long", "both"), default="both")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--all-work", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--counters")
    ap.add_argument("--hbm-gbps", type=float, default=8000.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    mods = tuple(importlib.import_module("sfm-gms_amd" + s) for s in ("", ".batch", ".synth", ".types"))
    ctx = mods[0].GmsContext(0)
    record = {"what": "gms_sfm_ba_device beside gms_sfm_register_device and gms_two_view_batch_device on the same pairs; ms per call, median "
              f"and best of {a.repeats} after {a.warmup}", "workloads": {}}
    for name in (("small", "long") if a.workload == "both" else (a.workload,)):
        record["workloads"][name] = run(name, ctx, mods, a)
        print(json.dumps({name: record["workloads"][name]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
