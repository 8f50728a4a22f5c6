#!/usr/bin/env python3
"""tools/bf_select_bench.py -- the batched bruteForceMatch (gms_bf_select_device: matcher + cross-check + sort + ratio prune;
DESIGN.md §4.5b) against the plain matcher gms_bfmatch_device on the same pairs:

    python tools/bf_select_bench.py [--rows 10000] [--frames 32] [--pairs 1024] [--warmup 3] [--iters 10] [--seed 1]

Two descriptor kinds: SIFT-like rows (128 integers 0..255 as floats, so the matcher runs on the matrix cores) and ORB rows (32 bytes,
prepared block). Each frame after the first is the previous one with 30 % of its rows redrawn, so cross-check and the ratio keep a
real share. Pairs are a seeded draw of (frame_a, frame_b), a != b. Timed with device events after warm-up, each on its own:
matcher (gms_bfmatch_device), select (gms_bf_select_device with cross-check), select_no_cc (without). The select share is the part
of the select time beyond the matcher's (plan + merge + sort + writes). Two pairs are checked byte for byte against
tests/bf_select_ref.py. Prints one JSON record."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def frames_of(kind, n_frames, n, rng):
    if kind == 0:
        cur = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    else:
        cur = np.where(rng.uniform(size=(n, 128)) < 0.5, rng.integers(0, 120, (n, 128)), 0).astype(np.float32)
    out = [cur]
    for _ in range(1, n_frames):
        cur = cur.copy()
        redraw = rng.uniform(size=n) < 0.3
        k = int(redraw.sum())
        cur[redraw] = rng.integers(0, 256, (k, 32), dtype=np.uint8) if kind == 0 else \
            np.where(rng.uniform(size=(k, 128)) < 0.5, rng.integers(0, 120, (k, 128)), 0).astype(np.float32)
        out.append(cur)
    return out


def timed(fn, stream, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("sfm-gms_amd")
    batch = importlib.import_module("sfm-gms_amd.batch")
    import bf_select_ref
    ctx = pkg.GmsContext(0)
    stream = torch.cuda.Stream()
    rec = dict(rows=args.rows, frames=args.frames, pairs=args.pairs, iters=args.iters)
    for name, kind in (("sift_int", pkg.GMS_DESC_L2_F32X128), ("orb", pkg.GMS_DESC_HAMMING256)):
        rng = np.random.default_rng(args.seed + kind)
        rows = frames_of(kind, args.frames, args.rows, rng)
        kps = [np.zeros(args.rows, pkg.KEYPOINT_DTYPE) for _ in rows]
        frames = batch.FrameTable(ctx, kps, [(1920, 1080)] * len(rows))
        descs = batch.DescriptorTable(ctx, frames, rows, kind)
        a = rng.integers(0, args.frames, args.pairs)
        b = (a + rng.integers(1, args.frames, args.pairs)) % args.frames
        fp = np.stack([a, b], 1)
        # the plain matcher: one match per query row, laid out by pair
        mrecs = np.zeros(args.pairs, pkg.PAIR_DTYPE)
        mrecs["frame_a"], mrecs["frame_b"], mrecs["m"] = a, b, args.rows
        mrecs["match_off"] = np.arange(args.pairs) * args.rows
        d_mpairs = batch._to_dev(mrecs, frames.device)
        d_matches = torch.zeros(args.pairs * args.rows * 16, dtype=torch.uint8, device=frames.device)
        runs = {cc: batch.BfSelect(ctx, descs, batch.bf_select_table(descs, fp), cc) for cc in (True, False)}
        ctx.set_stream(stream.cuda_stream)
        try:
            t_match = timed(lambda: descs.match_device(d_mpairs.data_ptr(), args.pairs, args.rows, d_matches.data_ptr()), stream,
                            args.warmup, args.iters)
            t_sel = timed(runs[True].run, stream, args.warmup, args.iters)
            t_nocc = timed(runs[False].run, stream, args.warmup, args.iters)
        finally:
            ctx.set_stream(None)
        out, res, _ = runs[True].results()
        assert (res["status"] == 0).all()
        recs = runs[True].recs
        for p in (0, args.pairs - 1):
            want, _, _, _ = bf_select_ref.bf_match_select(rows[int(a[p])], rows[int(b[p])], kind == 0, True)
            o = int(recs["match_off"][p])
            assert out[o:o + len(want)].tobytes() == want.tobytes(), (name, p)
        rec[name] = dict(matcher_ms=round(t_match, 3), select_ms=round(t_sel, 3), select_no_cc_ms=round(t_nocc, 3),
                         ratio=round(t_sel / t_match, 3), ratio_no_cc=round(t_nocc / t_match, 3),
                         select_share=round(max(t_sel - t_match, 0.0) / t_sel, 3),
                         mean_candidates=round(float(res["n_candidates"].mean()), 1), mean_survivors=round(float(res["n_out"].mean()), 1),
                         checked_pairs=2)
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
