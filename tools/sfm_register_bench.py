#!/usr/bin/env python3
"""tools/sfm_register_bench.py -- what joining the pairs costs beside the stage that made them: for a chain of
frames, the registration call (gms_sfm_register_device through batch.SfmRegister), the two-view stage of the same session on the
same pairs (gms_two_view_batch_device), and the numpy statement (tests/sfm_register_ref.py) on the records the stage left.

    python tools/sfm_register_bench.py [--workload small|long|both] [--warmup 2] [--repeats 7] [--out profiles/sfm_register_bench.json]
                                       [--unique [--parent-lib libgms_hip_parent.so]] [--lib NAME]

--unique (writes profiles/sfm_unique_bench.json by default): also gms_match_unique_device alone (batch.MatchUnique on
the same survivors, mask and records) with its share of the 8 TB/s roofline on its algorithmic bytes -- 16 B DMatch + 1 B mask read
and 1 B keep written per match slot --, and the registration on the plane beside the one without. --parent-lib NAME: a build of the
parent commit under sfm-gms_amd/csrc; the registration without a plane is then timed in fresh child processes, the two libraries in
turn, and the record states the ratio of the medians and the spread of either build's repeats. --lib NAME: the library to load.

    small   8 frames, 7 chain pairs, 3000 keypoints per frame: about 3000 survivors per pair
    long    1000 frames, 999 chain pairs, 10000 keypoints per frame on 2016 x 1512 images (the size of BASELINE config 5's views)

Frames: synth.make_multi_view_scene (a rigid scene, keypoint i of every frame shows scene point i; eight poses along an arc, which a
longer chain visits in turn); survivors: the identity matches
with one in ten train indices replaced by a seeded draw, handed to the stage as the filter would leave them. Each time is a host
clock around one call that ends in a synchronisation of the context's stream: the median and the best of `repeats` calls after
`warmup`. The yardstick is the two-view stage of the same session; the record states the ratio. The numpy statement is timed once
(it is a definition, not an implementation: its union-find is a Python loop per match), and only below --statement-max-matches."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = {"small": dict(n_frames=8, n_kp=3000, size=(1920, 1080), camera=(1400.0, 1380.0, 960.0, 540.0)),
             "long": dict(n_frames=1000, n_kp=10000, size=(2016, 1512), camera=(1600.0, 1600.0, 1008.0, 756.0))}


def clock(fn, sync, warmup, repeats):
    times = []
    for i in range(warmup + repeats):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(float(np.median(times)), 3), "best": round(min(times), 3)}


def run(name, ctx, mods, a):
    import torch
    pkg, batch, synth, types = mods
    w = WORKLOADS[name]
    n, n_kp = w["n_frames"], w["n_kp"]
    # eight poses along an arc, visited in turn: consecutive frames always have a baseline, however long the chain is
    sc = synth.make_multi_view_scene(31, min(n, 8), size=w["size"], n_kp=n_kp, camera=w["camera"], noise_px=0.0)
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

    job = batch.SfmRegister(ctx, frames.frame_off_host, pairs, d_frame_off=frames.d_frame_off, d_pairs=d_pairs)
    t_tv = clock(two_view, sync, a.warmup, a.repeats)
    t_reg = clock(lambda: job.run(d_out, d_mask, d_p3, d_tv), sync, a.warmup, a.repeats)
    r = job.results()
    if a.only_register:
        return {"register_ms": t_reg}
    reg = r["registration"]
    line = {"frames": n, "pairs": n_pairs, "keypoints_per_frame": n_kp, "match_slots": total, "workspace_bytes": job.ws_bytes,
            "survivors_per_pair": n_kp, "points_per_pair_median": int(np.median(d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE)["n_triangulated"])),
            "ok_pairs": int(r["summary"]["n_ok_pairs"][0]), "registered": int(r["summary"]["n_registered"][0]), "tracks": int(r["summary"]["n_tracks"][0]),
            "n_links_median": int(np.median(reg["n_links"][reg["link"] >= 0])) if (reg["link"] >= 0).any() else 0,
            "register_ms": t_reg, "two_view_ms": t_tv, "register_over_two_view": round(t_reg["median"] / t_tv["median"], 4)}
    if a.unique:
        uq = batch.MatchUnique(ctx, frames.frame_off_host, pairs, d_frame_off=frames.d_frame_off, d_pairs=d_pairs)
        on = batch.SfmRegister(ctx, frames.frame_off_host, pairs, d_frame_off=frames.d_frame_off, d_pairs=d_pairs, keep=uq.d_keep)
        t_uq = clock(lambda: uq.run(d_out, d_mask, d_tv), sync, a.warmup, a.repeats)
        t_on = clock(lambda: on.run(d_out, d_mask, d_p3, d_tv), sync, a.warmup, a.repeats)
        counts, ron = uq.results()[1], on.results()
        algorithmic = 18 * total
        line["unique"] = {"match_unique_ms": t_uq, "workspace_bytes": uq.ws_bytes, "live": int(counts[:, 0].sum()), "kept": int(counts[:, 1].sum()),
                          "algorithmic_bytes": algorithmic,
                          "share_of_8TBs_roofline": round(algorithmic / (t_uq["median"] * 1e-3) / 8e12, 5),
                          "match_unique_over_register": round(t_uq["median"] / t_reg["median"], 4),
                          "register_on_plane_ms": t_on, "register_on_plane_over_register": round(t_on["median"] / t_reg["median"], 4),
                          "tracks": [int(r["summary"]["n_tracks"][0]), int(ron["summary"]["n_tracks"][0])],
                          "n_multi": [int(r["summary"]["n_multi"][0]), int(ron["summary"]["n_multi"][0])],
                          "views_are_the_same_bytes": ron["views"].tobytes() == r["views"].tobytes()}
    if total <= a.statement_max_matches:
        import sfm_register_ref as ref
        tv = d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE)
        t0 = time.perf_counter()
        want = ref.register(frames.frame_off_host, pairs, m, d_mask.cpu().numpy(), d_p3.cpu().numpy().reshape(-1, 3), tv)
        line["numpy_statement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        line["integers_equal_the_statement"] = bool(np.array_equal(want["registration"]["n_links"], reg["n_links"]) and
                                                    np.array_equal(want["track"], r["track"]) and np.array_equal(want["cloud_id"], r["cloud_id"]))
    else:
        line["numpy_statement_ms"] = None
        line["numpy_statement_note"] = "not measured: the statement's union-find is a Python loop per match"
    return line


def against_parent(a, names, rounds=3):
    """gms_sfm_register_device of this build and of the parent's (--parent-lib), each in fresh child processes, in turn: per workload
    the medians of every round, the ratio of the medians of those, and the spread (max - min over median) of either build's rounds."""
    import subprocess
    out = {}
    for name in names:
        got = {"this": [], "parent": []}
        for _ in range(rounds):
            for which, lib in (("this", "libgms_hip.so"), ("parent", a.parent_lib)):
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", name, "--warmup", str(a.warmup), "--repeats", str(a.repeats),
                                      "--lib", lib, "--only-register"], capture_output=True, text=True, timeout=900)
                if res.returncode != 0:
                    return {"failed": res.stderr[-400:]}
                got[which].append(json.loads(res.stdout.strip().splitlines()[0])[name]["register_ms"]["median"])
        med = {k: float(np.median(v)) for k, v in got.items()}
        out[name] = {"register_ms_medians": got, "this_over_parent": round(med["this"] / med["parent"], 4),
                     "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in got.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("small", "long", "both"), default="both")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--statement-max-matches", type=int, default=100000)
    ap.add_argument("--out")
    ap.add_argument("--unique", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--lib")
    ap.add_argument("--only-register", action="store_true", help="(the child of --parent-lib: the registration's times alone)")
    a = ap.parse_args()
    if a.unique and not a.out:
        a.out = os.path.join(ROOT, "profiles", "sfm_unique_bench.json")
    if a.lib:
        capi = importlib.import_module("sfm-gms_amd.capi")
        capi.library_path = lambda: os.path.join(ROOT, "sfm-gms_amd", "csrc", a.lib)
        import ctypes
        import torch  # noqa: F401  (its HIP runtime first, as capi.load_library has it)
        have = ctypes.CDLL(capi.library_path())
        for name in [n for n in capi.SIGNATURES if not hasattr(have, n)]:   # an older build lacks the newer entry points
            del capi.SIGNATURES[name]
    mods = tuple(importlib.import_module("sfm-gms_amd" + s) for s in ("", ".batch", ".synth", ".types"))
    ctx = mods[0].GmsContext(0)
    record = {"what": "gms_sfm_register_device beside gms_two_view_batch_device on the same pairs; ms per call, median and best of "
              f"{a.repeats} after {a.warmup}", "workloads": {}}
    for name in (("small", "long") if a.workload == "both" else (a.workload,)):
        record["workloads"][name] = run(name, ctx, mods, a)
        print(json.dumps({name: record["workloads"][name]}), flush=True)
    ctx.close()
    if a.parent_lib and not a.only_register:
        record["existing_entry_point_against_parent"] = against_parent(a, [n for n in record["workloads"]])
        print(json.dumps(record["existing_entry_point_against_parent"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
