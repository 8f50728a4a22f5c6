#!/usr/bin/env python3
"""tools/logos_bench.py -- the batched LOGOS path against the one-shot gms_logos_match:

    python tools/logos_bench.py [--frames 9] [--warmup 3] [--iters 10] [--sample 3] [--seed 1]

A seeded synthetic sequence per configuration -- keypoints moved by a rotation and a scale from frame to frame, 20 % of the
labels redrawn, descriptors scattered around a random fp32 dictionary -- and its consecutive pairs. Two configurations from the
reference: 10 000 keypoints with 50 words (SIFT_matchLOGOS, FeatureMatchUtil.cpp:86-131) and 5 000 with 100 words
(DisparityUtil.cpp:13,119). Timed each on its own with device events after warm-up: prepare (gms_logos_prepare_device), filter
(gms_logos_filter_device, all pairs in one run), words (gms_logos_words_device, every descriptor of the sequence), and a loop of
the one-shot gms_logos_match over the same pairs (host calls, each with its own allocations, copies and synchronisation, as a
caller of the one-shot pays them; its first call timed apart). A seeded sample of pairs is checked byte
for byte against the one-shot. Prints one JSON record."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sequence(pkg, seed, n_frames, n, n_words):
    rng = np.random.default_rng(seed)
    a4 = np.concatenate([rng.uniform(0, 1920, (n, 2)), rng.uniform(2, 30, (n, 1)), rng.uniform(0, 360, (n, 1))], 1)
    w = rng.integers(0, n_words, n)
    dic = rng.uniform(0, 100, (n_words, 128)).astype(np.float32)
    frames, words = [], []
    for f in range(n_frames):
        if f:
            th, sc = rng.uniform(-0.3, 0.3), rng.uniform(0.9, 1.1)
            c, s = np.cos(th), np.sin(th)
            xy = a4[:, :2] - 960.0
            a4 = a4.copy()
            a4[:, 0] = sc * (c * xy[:, 0] - s * xy[:, 1]) + 960.0 + rng.uniform(-10, 10)
            a4[:, 1] = sc * (s * xy[:, 0] + c * xy[:, 1]) + 960.0 + rng.uniform(-10, 10)
            a4[:, 2] *= sc
            a4[:, 3] = np.mod(a4[:, 3] - np.degrees(th), 360.0)
            w = w.copy()
            flip = rng.random(n) < 0.2
            w[flip] = rng.integers(0, n_words, int(flip.sum()))
        k = np.zeros(n, pkg.KEYPOINT_DTYPE)
        k["x"], k["y"], k["size"], k["angle"] = a4[:, 0], a4[:, 1], a4[:, 2], a4[:, 3]
        frames.append(k)
        words.append(w.astype(np.int32))
    descs = [(dic[w] + rng.normal(0, 5, (n, 128))).astype(np.float32) for w in words]
    return frames, words, descs, dic


def oneshot(lib, pkg, kp1, kp2, l1, l2):
    cap = max(len(kp1), len(kp2))
    while True:
        out = np.zeros(cap, pkg.DMATCH_DTYPE)
        n = C.c_int64(0)
        rc = lib.gms_logos_match(kp1.ctypes.data, len(kp1), kp2.ctypes.data, len(kp2), l1.ctypes.data, l2.ctypes.data, out.ctypes.data,
                                 cap, C.byref(n), None)
        if rc == -5 and n.value > cap:
            cap = n.value
            continue
        assert rc == 0, rc
        return out[: n.value]


def run_config(pkg, batch, ctx, torch, n, n_words, a):
    lib = pkg.load_library()
    frames, words, descs, dic = sequence(pkg, a.seed * 1000 + n + n_words, a.frames, n, n_words)
    fp = [(f, f + 1) for f in range(a.frames - 1)]
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    ctx.set_stream(s.cuda_stream)
    try:
        table = batch.LogosTable(ctx, frames, words, n_words)
        pairs = batch.logos_pair_table(table, fp, capacity=4 * n)
        npairs = len(pairs)
        ws = ctx.logos_workspace_bytes(table.max_kp, npairs, n)
        d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        d_pairs = batch._to_dev(pairs, dev)
        d_out = torch.zeros(int(pairs["m"].sum()) * 16, dtype=torch.uint8, device=dev)
        d_lres = torch.zeros(npairs * 32, dtype=torch.uint8, device=dev)
        d_desc = torch.from_numpy(np.concatenate(descs).view(np.uint8).reshape(-1)).to(dev)
        d_dict = torch.from_numpy(dic.view(np.uint8).reshape(-1).copy()).to(dev)
        d_words = torch.zeros(table.total, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def prepare():
            ctx.logos_prepare_device(table.d_kp.data_ptr(), table.d_frame_off.data_ptr(), table.n_frames, table.total,
                                     table.d_words.data_ptr(), n_words, d_ws.data_ptr(), ws, table.d_table.data_ptr())

        def filt():
            table.filter_device(d_pairs.data_ptr(), npairs, d_ws.data_ptr(), ws, d_out.data_ptr(), d_lres.data_ptr())

        def wrds():
            ctx.logos_words_device(pkg.GMS_DESC_L2_F32X128, d_desc.data_ptr(), table.total, d_dict.data_ptr(), n_words, d_words.data_ptr())

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.iters):
                fn()
            e1.record(s)
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iters

        t_prep = timed(prepare)
        t_filter = timed(filt)
        t_words = timed(wrds)
        ctx.synchronize()
        lres = d_lres.cpu().numpy().view(pkg.LOGOS_RESULT_DTYPE).copy()
        out = d_out.cpu().numpy().view(pkg.DMATCH_DTYPE)
        words_ok = bool((d_words.cpu().numpy() == np.concatenate(words)).mean() > 0.99)
    finally:
        ctx.set_stream(None)
    assert (lres["status"] == 0).all(), lres["status"]
    # the one-shot over the same pairs: its first call apart, then the loop between events on the null stream it runs on
    t0 = time.perf_counter()
    oneshot(lib, pkg, frames[0], frames[1], words[0], words[1])
    t_first = (time.perf_counter() - t0) * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.default_stream(dev))
    w0 = time.perf_counter()
    ref = [oneshot(lib, pkg, frames[x], frames[y], words[x], words[y]) for x, y in fp]
    wall = (time.perf_counter() - w0) * 1e3
    e1.record(torch.cuda.default_stream(dev))
    e1.synchronize()
    t_loop = e0.elapsed_time(e1)
    rng = np.random.default_rng(a.seed)
    sample = sorted(rng.choice(npairs, size=min(a.sample, npairs), replace=False).tolist())
    equal = all(out[int(pairs["match_off"][p]):int(pairs["match_off"][p]) + int(lres["n_out"][p])].tobytes() == ref[p].tobytes()
                for p in sample)
    cand, supp = int(lres["n_candidates"].sum()), int(lres["n_supported"].sum())
    return {
        "keypoints": n, "words": n_words, "frames": a.frames, "pairs": npairs,
        "prepare_ms": round(t_prep, 4), "filter_ms": round(t_filter, 4), "words_ms": round(t_words, 4),
        # the one-shot per pair as a caller runs it: its device allocations, host copies and synchronisation included
        "oneshot_loop_ms": round(t_loop, 3), "oneshot_loop_wall_ms": round(wall, 3), "oneshot_first_call_ms": round(t_first, 3),
        "filter_pairs_per_s": round(npairs / (t_filter * 1e-3), 1),
        "prepare_plus_filter_pairs_per_s": round(npairs / ((t_prep + t_filter) * 1e-3), 1),
        "oneshot_pairs_per_s": round(npairs / (t_loop * 1e-3), 1),
        "speedup_filter_vs_oneshot": round(t_loop / t_filter, 2),
        "speedup_prepare_plus_filter_vs_oneshot": round(t_loop / (t_prep + t_filter), 2),
        "candidates": cand, "supported": supp, "survivors": int(lres["n_out"].sum()),
        # pass 1 runs the support test once per candidate (passes 2 and 3 again only for candidates within 0.1 rad of the peak, a
        # number the records do not give); the one-shot scans 3 n1 n2 labels per pair to find the same candidates
        "candidates_per_s": round(cand / (t_filter * 1e-3), 1),
        "oneshot_label_scans": 3 * n * n * npairs,
        "words_rows_per_s": round(table.total / (t_words * 1e-3), 1), "words_match_generating_labels": words_ok,
        "sample_pairs": sample, "sample_byte_equal": bool(equal),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sample", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    with pkg.GmsContext(0) as ctx:
        configs = [run_config(pkg, batch, ctx, torch, n, w, a) for n, w in ((10000, 50), (5000, 100))]
    print(json.dumps({"tool": "logos_bench", "device": torch.cuda.get_device_name(0), "configs": configs,
                      "sample_byte_equal": all(c["sample_byte_equal"] for c in configs)}))
    return 0 if all(c["sample_byte_equal"] for c in configs) else 1


if __name__ == "__main__":
    sys.exit(main())
