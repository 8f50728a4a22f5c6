#!/usr/bin/env python3
"""bench.py -- GMS-filtered image pairs per second on MI355X (BASELINE.json metric).

Workload = BASELINE config 3: ONE synthetic 1000-frame 1080p sequence, 10k keypoints per frame (an 80 MB table of
normalised points, replicated on every GPU), all 499 500 pairs (a < b) in lexicographic order; rank r owns the contiguous
block shard_range(499500, r, world) of that one list. A "step" is one pass of the hot path (gms_filter_device, one
launch) over the next chunk of `--pairs` pairs of the rank's block, with the chunk's putative matches (M = 10k per pair,
generated on the device, a pure function of the global pair index) already resident in HBM; every step works on a
different chunk. Flags of the headline: the reference's DisparityUtil.cpp:149,299 call sites (withRotation=false,
withScale=false, 6.0); the (true, true) flags of FeatureMatchUtil.cpp:69 are reported beside it under "rot_scale".

  python bench.py --gpus N --steps K --warmup W         (N > 1 without a launcher: starts the N ranks itself)
  python bench.py ... --dump-outputs DIR                 (also writes what the last timed step computed: dump_outputs)
  python bench.py ... --full                             (also everything beyond the headline; see below)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A plain run does what the headline needs and nothing more: it sets up, warms up, times the K steps, writes
--dump-outputs, and prints the line (the headline with its roofline from the timed launches' own events).
--full adds, after the timed steps and the dump: the parity check, the committed PMC traffic profile, opencv_on_box and,
on one rank, the CPU baseline (unless --no-cpu) and the side records (unless --no-extra): rot_scale, real_pixels,
config4, descriptors_to_filtered_matches, descriptors_to_poses, pixels_to_keypoints.

Pairs are independent: no collective on the data path ("scaling": "weak": pairs per GPU per step are
fixed). The rendezvous (barrier around the timed region, MAX of the ranks' times, SUM of the parity counts) runs over
gloo on CPU tensors -- the path needs no RCCL. With --full every rank checks every 997th global pair it filtered against
the CPU oracle, outside the timed region; a mismatch makes the run exit non-zero.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "sfm-gms_amd"
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable by a copy
SIZE = (1920, 1080)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8192, help="image pairs per step per GPU (one chunk = one launch: 1.3 GB of matches in, up to 1.3 GB out)")
    ap.add_argument("--frames", type=int, default=1000, help="frames of the synthetic sequence (config 3: 1000)")
    ap.add_argument("--features", type=int, default=10000)
    ap.add_argument("--inlier-frac", type=float, default=0.5)
    ap.add_argument("--max-resident", type=int, default=24,
                    help="chunks kept resident in HBM (2.6 GB each at the defaults); more steps cycle through them")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the all-core CPU baseline (0 = every CPU this process may use)")
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--cpu-oversubscribe", action="store_true", help="also time one thread per CPU of the affinity mask, beyond the cgroup's quota")
    ap.add_argument("--spatial-order", action="store_true",
                    help="diagnostic: keypoints listed cell by cell instead of in random order (LDS bank-conflict experiment, DESIGN.md 6)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the parity check, the CPU baseline and the side measurements (off: the headline only)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline leg (profiling runs)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the side measurements (rot_scale and the records after it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy "
                         "(every pair's result record, the survivors of a fixed sample of its pairs; rank 0's shard)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as child processes (before anything here has
    touched the GPU), relay their output, exit with their code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


class Workload:
    """This rank's share of config 3, resident on the GPU: the frame table and `n_res` chunks of pairs + matches."""

    def __init__(self, args, rank, world, dev, pkg, ctx):
        import torch
        synth = importlib.import_module(PKG + ".synth")
        batch = importlib.import_module(PKG + ".batch")
        self.dist = importlib.import_module(PKG + ".dist")
        self.n_kp = args.features
        self.frames = synth.make_sequence(1000, args.frames, size=SIZE, n_kp=self.n_kp,  # the same sequence on every rank
                                          spatial_order=getattr(args, "spatial_order", False))
        self.table = batch.FrameTable(ctx, self.frames, [SIZE] * args.frames, device=dev)
        # the per-frame work the filter no longer does per pair (normalizePoints + the keypoints' cell codes): once per sequence,
        # amortised over the 999 pairs every frame takes part in; timed here so that the line can say what it costs
        # (on a stream of its own: the handle of torch's current stream is 0, which gms_ctx_set_stream reads as "the context's own
        #  stream" -- events recorded on stream 0 would not bracket the kernel)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = torch.cuda.Stream(device=dev)
        assert st.cuda_stream != 0
        ctx.set_stream(st.cuda_stream)
        t = self.table
        torch.cuda.synchronize()
        ctx.normalize_device(t.d_kp.data_ptr(), t.d_frame_off.data_ptr(), t.d_wh.data_ptr(), t.n_frames, t.total, t.d_pts.data_ptr())  # warm-up
        ev0.record(st)
        ctx.normalize_device(t.d_kp.data_ptr(), t.d_frame_off.data_ptr(), t.d_wh.data_ptr(), t.n_frames, t.total, t.d_pts.data_ptr())
        ev1.record(st)
        torch.cuda.synchronize()
        self.frame_table_build_ms = float(ev0.elapsed_time(ev1))
        self.frame_table_bytes = int(ctx.frame_table_bytes(t.total))
        n_chunks = min(args.warmup + args.steps, max(1, args.max_resident))
        self.plan = self.dist.RankPlan(args.frames, self.n_kp, args.pairs, n_chunks, rank, world)
        self.n_pairs = self.plan.chunk
        self.chunks = []
        for c in range(n_chunks):
            pairs = self.plan.chunk_pairs(c)
            total_m = self.n_pairs * self.n_kp
            self.chunks.append(dict(
                pairs=pairs,
                d_pairs=torch.from_numpy(pairs.view(np.uint8).reshape(-1)).to(dev),
                d_matches=self.dist.synth_matches_device(self.plan.starts[c], self.n_pairs, self.n_kp, args.inlier_frac, dev),
                d_out=torch.zeros((total_m, 4), dtype=torch.int32, device=dev),
                d_res=torch.zeros((self.n_pairs, 4), dtype=torch.int32, device=dev)))
        torch.cuda.synchronize()

    def launch(self, ctx, c, rot, scale, n_pairs=None):
        t, ch = self.table, self.chunks[c % len(self.chunks)]
        ctx.filter_device(t.d_pts.data_ptr(), t.d_frame_off.data_ptr(), t.n_frames, ch["d_pairs"].data_ptr(),
                          n_pairs or self.n_pairs, self.n_kp, ch["d_matches"].data_ptr(), ch["d_out"].data_ptr(),
                          ch["d_res"].data_ptr(), None, rot, scale, 6.0)

    def host_pairs(self, pkg, c, idx):
        """Host copies of pairs `idx` (indices inside chunk c): (pair table rebased to 0, matches, gpu out, gpu results)."""
        ch = self.chunks[c]
        n_kp = self.n_kp
        idx = list(idx)
        sel = ch["pairs"][idx].copy()
        if idx == list(range(idx[0], idx[0] + len(idx))):  # a run of consecutive pairs: one copy each
            m = ch["d_matches"][idx[0] * n_kp:(idx[-1] + 1) * n_kp].cpu().numpy()
            o = ch["d_out"][idx[0] * n_kp:(idx[-1] + 1) * n_kp].cpu().numpy()
        else:
            m = np.concatenate([ch["d_matches"][i * n_kp:(i + 1) * n_kp].cpu().numpy() for i in idx])
            o = np.concatenate([ch["d_out"][i * n_kp:(i + 1) * n_kp].cpu().numpy() for i in idx])
        sel["match_off"] = np.arange(len(idx), dtype=np.int64) * n_kp
        res = ch["d_res"].cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)[idx]
        return (sel, m.view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE), o.view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE), res)


def timed_steps(ctx, wl, stream, steps, warmup, rot, scale, dist, first_chunk=0, n_pairs=None):
    """W warm-up steps, then exactly K steps between barrier + synchronize brackets. Returns (wall seconds of the K steps,
    mean ms per launch from HIP events recorded on the launch stream)."""
    import torch
    with torch.cuda.stream(stream):
        for s in range(warmup):
            wl.launch(ctx, first_chunk + s, rot, scale, n_pairs)
    torch.cuda.synchronize()
    wl.dist.barrier(dist)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        for s in range(steps):
            ev[s][0].record(stream)
            wl.launch(ctx, first_chunk + warmup + s, rot, scale, n_pairs)
            ev[s][1].record(stream)
    torch.cuda.synchronize()
    wl.dist.barrier(dist)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return wall, float(np.mean([a.elapsed_time(b) for a, b in ev]))


DUMP_SEED = 0x6D5  # which pairs of the last step --dump-outputs writes in full
DUMP_SAMPLE_PAIRS = 256
DUMP_MATCH_BYTES = 48 << 20  # budget of the survivors' records (float32 x 4 per match; everything else is small)


def dump_outputs(wl, pkg, chunk, out_dir):
    """--dump-outputs: what the launch on `chunk` (the last timed step) handed its caller, as float arrays.
    results.npy          float64 [pairs, 4]   every pair's gms_result: n_inliers, best_scale, best_rot, status
    sample_pairs.npy     float64 [S, 4]       the sampled pairs: index in the step, frame_a, frame_b, survivors
    sample_matches.npy   float32 [sum, 4]     their surviving gms_dmatch records in order: queryIdx, trainIdx, imgIdx, distance
    The sample is a fixed, seeded choice of S pairs of the step, sized so that S x M records stay within DUMP_MATCH_BYTES."""
    import torch
    ch, n_kp = wl.chunks[chunk], wl.n_kp
    res = ch["d_res"].cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
    n_pairs = len(res)
    n_sample = max(1, min(DUMP_SAMPLE_PAIRS, n_pairs, DUMP_MATCH_BYTES // (16 * n_kp)))
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n_pairs, n_sample, replace=False))
    kept = res["n_inliers"][idx].astype(np.int64)
    rows = np.concatenate([np.arange(j * n_kp, j * n_kp + k, dtype=np.int64) for j, k in zip(idx, kept)])
    recs = ch["d_out"].index_select(0, torch.from_numpy(rows).to(ch["d_out"].device)).cpu().numpy()
    recs = recs.view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
    pairs = ch["pairs"][idx]
    arrays = {
        "results": np.stack([res[f].astype(np.float64) for f in pkg.RESULT_DTYPE.names], axis=1),
        "sample_pairs": np.stack([idx, pairs["frame_a"], pairs["frame_b"], kept], axis=1).astype(np.float64),
        "sample_matches": np.stack([recs[f].astype(np.float32) for f in pkg.DMATCH_DTYPE.names], axis=1),
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {"dir": out_dir, "step_chunk": chunk, "pairs": n_pairs, "sample_pairs": n_sample,
            "bytes": int(sum(a.nbytes for a in arrays.values()))}


def opencv_on_box():
    """is there an OpenCV with the reference's own matchGMS on this box? (Only recorded; tests/test_gpu_opencv_probe.py uses it.)"""
    try:
        import cv2
    except Exception as e:  # noqa: BLE001
        return {"present": False, "found": f"no cv2 module ({type(e).__name__})"}
    has = hasattr(getattr(cv2, "xfeatures2d", None), "matchGMS")
    return {"present": bool(has), "found": f"cv2 {cv2.__version__} " + ("with" if has else "without") + " xfeatures2d.matchGMS"}


def oracle_module():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gms_oracle
    return gms_oracle


def check_parity(wl, pkg, chunk_ids, rot, scale, sample=None):
    """Every 997th global pair among the given chunks (or `sample` = {chunk: [local indices]}) against the CPU oracle, from
    what the last launch on those chunks left in d_out / d_res. Returns (pairs checked, pairs that differ)."""
    oracle = oracle_module()
    kp_all = np.concatenate(wl.frames)
    foff = wl.table.frame_off_host
    wh = np.array([SIZE] * len(wl.frames), dtype=np.int32).reshape(-1)
    checked = bad = 0
    for c in chunk_ids:
        idx = sample[c] if sample is not None else [j for _, j in wl.plan.chunk_sample(c)]
        if not idx:
            continue
        sel, m, gpu_out, gpu_res = wl.host_pairs(pkg, c, idx)
        failed, out, res, _ = oracle.batch(kp_all, foff, wh, sel, m, rot, scale, 6.0, 1)
        for i in range(len(idx)):
            k, o = int(res["n_inliers"][i]), int(sel["match_off"][i])
            same = (failed == 0 and gpu_res["status"][i] == 0 and res[i].tobytes() == gpu_res[i].tobytes() and
                    out[o:o + k].tobytes() == gpu_out[o:o + k].tobytes())
            checked += 1
            bad += 0 if same else 1
    return checked, bad


def cgroup_cpu_quota():
    """The container's CPU time limit in CPUs (cgroup v2 cpu.max, v1 cfs quota / period), or None when unlimited / unreadable."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def cpu_threads_available():
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = cgroup_cpu_quota()
    return affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))


def cpu_baseline(args, wl, pkg, rot, scale, budget_s):
    """The oracle (CPU restatement of the reference's matchGMS, one pair per thread) on the first pairs of chunk 0, at 1, 16 and
    all threads; median of --cpu-reps repetitions each, sample sizes chosen for about `budget_s` seconds of CPU work in all."""
    oracle = oracle_module()
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = cgroup_cpu_quota()  # CPUs' worth of time the container may use (a GPU box hands a one-GPU job a share of the host)
    avail = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    all_threads = args.cpu_threads if args.cpu_threads > 0 else avail
    kp_all = np.concatenate(wl.frames)
    foff = wl.table.frame_off_host
    wh = np.array([SIZE] * len(wl.frames), dtype=np.int32).reshape(-1)
    reps = max(1, args.cpu_reps)

    def run(n, threads):
        n = max(1, min(n, wl.n_pairs))
        sel, m, _, _ = wl.host_pairs(pkg, 0, list(range(n)))
        # output arrays allocated and touched once: the timed calls fault no fresh pages (oracle/gms_ref_mt.c keeps its working
        # storage per thread for the same reason: nothing but the algorithm inside the timed region)
        bufs = (np.ones(len(m), dtype=pkg.DMATCH_DTYPE), np.ones(len(m), dtype=np.uint8), np.ones(n, dtype=pkg.RESULT_DTYPE))
        times = []
        for _ in range(reps + 1):  # one warm-up
            t0 = time.perf_counter()
            failed, _, _, _ = oracle.batch(kp_all, foff, wh, sel, m, rot, scale, 6.0, threads, bufs=bufs)
            times.append(time.perf_counter() - t0)
            assert failed == 0
        return n / float(np.median(times[1:])), n

    # size the samples from a quick single-thread probe: each of the three legs gets a third of the budget, and every thread of a
    # leg at least eight pairs
    r_probe, n_probe = run(8, 1)
    per_leg = budget_s / 3.0 / (reps + 1)
    legs = {}
    for threads in sorted({1, min(16, all_threads), all_threads, min(affinity, 256) if args.cpu_oversubscribe else 1}):
        n = int(min(wl.n_pairs, max(8 * threads, r_probe * per_leg * min(threads, avail) ** 0.9)))
        rate, n_used = run(n, threads)
        legs[threads] = {"pairs_per_s": rate, "pairs": n_used}
    best = max(legs, key=lambda t: legs[t]["pairs_per_s"])
    return {"value": legs[best]["pairs_per_s"], "unit": "pairs/s", "cores": best, "kind": "port",
            "sample": f"first {legs[best]['pairs']} pairs of the rank's first chunk, oracle/gms_ref.c (per-thread reusable storage, atomic work "
                      f"counter), one pair per thread, median of {reps}",
            "by_threads": {str(t): legs[t] for t in legs}, "cpus_available": avail, "cpu_affinity": affinity, "cgroup_cpu_quota": quota,
            "host_cpus": os.cpu_count()}


def bf_gms_leg(ctx, wl, pkg, stream, kind, n_frames=64, n_pairs=1024, steps=3):
    """Descriptors resident in HBM -> brute-force matches (gms_bfmatch_device) -> filtered matches (gms_filter_device), the
    pipeline of FeatureMatchUtil.cpp:58-69 with the match array never leaving the GPU: the first `n_pairs` pairs of the first
    `n_frames` frames of the sequence. Returns the record for the JSON line."""
    import torch
    batch = importlib.import_module(PKG + ".batch")
    dev = wl.table.device
    n_frames = min(n_frames, len(wl.frames))
    n_kp = wl.n_kp
    n_pairs = min(n_pairs, n_frames * (n_frames - 1) // 2)
    frames = wl.frames[:n_frames]
    table = batch.FrameTable(ctx, frames, [SIZE] * n_frames, device=dev)
    d_desc = wl.dist.synth_descriptors_device(n_frames, n_kp, kind, 0.3, dev)
    code = pkg.GMS_DESC_HAMMING256 if kind == "orb" else pkg.GMS_DESC_L2_F32X128
    d_prep = torch.zeros(max(ctx.bf_prepared_bytes(code, table.total, n_frames), 16), dtype=torch.uint8, device=dev)
    pairs = wl.dist.pair_table(n_frames, 0, n_pairs, n_kp)
    d_pairs = torch.from_numpy(pairs.view(np.uint8).reshape(-1)).to(dev)
    d_matches = torch.zeros((n_pairs * n_kp, 4), dtype=torch.int32, device=dev)
    d_out = torch.zeros((n_pairs * n_kp, 4), dtype=torch.int32, device=dev)
    d_res = torch.zeros((n_pairs, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * steps)]
    t0 = None
    with torch.cuda.stream(stream):
        ctx.bf_prepare_device(code, d_desc.data_ptr(), table.d_frame_off.data_ptr(), n_frames, table.total, d_prep.data_ptr())
        for s in range(-1, steps):  # one warm-up
            if s == 0:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if s >= 0:
                ev[3 * s].record(stream)
            ctx.bfmatch_device(code, d_desc.data_ptr(), d_prep.data_ptr(), table.total, table.d_frame_off.data_ptr(), n_frames,
                               d_pairs.data_ptr(), n_pairs, n_kp, d_matches.data_ptr())
            if s >= 0:
                ev[3 * s + 1].record(stream)
            ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), n_frames, d_pairs.data_ptr(), n_pairs, n_kp,
                              d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, False, False, 6.0)
            if s >= 0:
                ev[3 * s + 2].record(stream)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    match_ms = float(np.mean([ev[3 * s].elapsed_time(ev[3 * s + 1]) for s in range(steps)]))
    filter_ms = float(np.mean([ev[3 * s + 1].elapsed_time(ev[3 * s + 2]) for s in range(steps)]))
    res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
    # parity on two pairs, end to end: the oracle's brute-force matcher, then the oracle's filter
    oracle = oracle_module()
    desc_h = d_desc.cpu().numpy()
    kp_all = np.concatenate(frames)
    wh = np.array([SIZE] * n_frames, dtype=np.int32).reshape(-1)
    idx = sorted(set(int(v) for v in np.linspace(0, n_pairs - 1, 16)))      # sixteen pairs spread over the launch, first and last included

    def check(i):   # (the C oracle releases the GIL: the sixteen checks run on the box's cores side by side)
        a, b = int(pairs["frame_a"][i]), int(pairs["frame_b"][i])
        want_m = oracle.bf_match(desc_h[a * n_kp:(a + 1) * n_kp], desc_h[b * n_kp:(b + 1) * n_kp], kind == "orb")
        got_m = d_matches[i * n_kp:(i + 1) * n_kp].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
        sel = pairs[i:i + 1].copy()
        sel["match_off"] = 0
        failed, wout, wres, _ = oracle.batch(kp_all, table.frame_off_host, wh, sel, want_m, False, False, 6.0, 1)
        k = int(wres["n_inliers"][0])
        got_o = d_out[i * n_kp:i * n_kp + k].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
        return bool(failed or got_m.tobytes() != want_m.tobytes() or res[i].tobytes() != wres[0].tobytes() or got_o.tobytes() != wout[:k].tobytes())
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(16, cpu_threads_available())) as pool:
        bad = int(sum(pool.map(check, idx)))
    evals = float(n_pairs) * n_kp * n_kp
    if kind == "orb":  # hamming = |a| + |b| - 2 a.b over the 256 bits as 0/1 FP4 elements on v_mfma_scale_f32_32x32x64_f8f6f4: 2 x 256 ops per evaluation
        roof = {"bound": "mfma", "achieved": evals * 512 / (match_ms * 1e-3) / 1e12, "peak": 10000.0, "unit": "TFLOP/s (fp4)",
                "note": "FP4 dense peak = 4 x the bf16 dense peak (MI355X_MICROARCH.md, Matrix cores); HBM traffic of the matcher is 2.6 MB per pair"}
    else:  # d^2 = w(a) + 2 a'.~b' + c(b) with the cross term on v_mfma_i32_32x32x32_i8: 2 x 128 int8 ops per evaluation
        roof = {"bound": "mfma", "achieved": evals * 256 / (match_ms * 1e-3) / 1e12, "peak": 5000.0, "unit": "TOP/s (int8)",
                "note": "int8 dense peak = 2 x the bf16 dense peak; 2 x 128 ops per distance evaluation"}
    roof["frac"] = roof["achieved"] / roof["peak"]
    roof["kernel_ms_per_launch"] = match_ms
    return {"workload": f"{kind}: descriptors of {n_frames} frames x {n_kp} keypoints resident in HBM -> BFMatcher::match (no cross-check, "
                        f"M = N1) -> matchGMS(false, false, 6.0) for {n_pairs} pairs per step; matches never leave the GPU",
            "value": n_pairs * steps / wall, "unit": "pairs/s", "pairs_per_step": n_pairs, "matcher_ms_per_step": match_ms,
            "filter_ms_per_step": filter_ms, "mean_kept_per_pair": float(res["n_inliers"].mean()), "roofline": roof,
            "parity": {"pairs_checked": len(idx), "mismatches": bad, "bit_exact": bad == 0,
                       "rule": "matches and filtered output of sixteen pairs spread over the launch vs oracle/bf_ref.c + oracle/gms_ref.c"}}


def zoom_leg(ctx, pkg, stream, dev, n_frames=64, n_kp=10000, n_pairs=1024, steps=6):
    """matchGMS(true, true, 6.0) on pairs whose right image shows the scene at half the left image's magnification
    (synth.make_zoom_sequence, zoom 2: odd frame -> even frame): the winner is scale hypothesis 3 (28 x 28 right grid), one of the
    scales the probe tries to bound out -- here it cannot."""
    import torch
    synth = importlib.import_module(PKG + ".synth")
    batch = importlib.import_module(PKG + ".batch")
    distmod = importlib.import_module(PKG + ".dist")
    frames = synth.make_zoom_sequence(1000, n_frames, size=SIZE, n_kp=n_kp, zoom=2.0)
    table = batch.FrameTable(ctx, frames, [SIZE] * n_frames, device=dev)
    pairs = np.zeros(n_pairs, dtype=pkg.PAIR_DTYPE)
    k = 0
    for a in range(1, n_frames, 2):
        for b in range(0, n_frames, 2):
            if k < n_pairs:
                pairs[k] = (a, b, n_kp, 0, k * n_kp)
                k += 1
    n_pairs = k
    pairs = pairs[:n_pairs]
    d_pairs = torch.from_numpy(pairs.view(np.uint8).reshape(-1)).to(dev)
    d_matches = distmod.synth_matches_device(0, n_pairs, n_kp, 0.5, dev)
    d_out = torch.zeros((n_pairs * n_kp, 4), dtype=torch.int32, device=dev)
    d_res = torch.zeros((n_pairs, 4), dtype=torch.int32, device=dev)
    ctx.reserve(n_pairs, n_kp, True, True)
    out = {"workload": f"{n_pairs} pairs (zoomed frame, plain frame) of a zooming sequence (the right image at half the magnification), "
                       "10k matches per pair, flags (true, true, 6.0)"}
    for name, val in (("auto", -1), ("off", 0), ("on", 1)):
        ctx.set_option(2, val)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        # "auto" is the library's steady state on this sequence: it measures every sixteenth launch which scales' probes pay and follows
        # that, scale by scale, from the next launch that finds the verdict complete -- so two measuring cycles run before the clock does
        warm = 36 if name == "auto" else 2
        with torch.cuda.stream(stream):
            for s in range(-warm, steps):
                if s < 0 and s % 4 == 0:
                    torch.cuda.synchronize()
                if s >= 0:
                    ev[s][0].record(stream)
                ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), n_frames, d_pairs.data_ptr(), n_pairs, n_kp,
                                  d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, True, True, 6.0)
                if s >= 0:
                    ev[s][1].record(stream)
        torch.cuda.synchronize()
        ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
        out[name] = {"pairs_per_s": n_pairs / (ms * 1e-3), "ms_per_launch": ms, "probe_mask": ctx.query(2)}
    ctx.set_option(2, -1)
    res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
    out["winning_scales"] = {str(sc): int((res["best_scale"] == sc).sum()) for sc in range(-1, 5) if (res["best_scale"] == sc).any()}
    oracle = oracle_module()
    kp_all = np.concatenate(frames)
    wh = np.array([SIZE] * n_frames, dtype=np.int32).reshape(-1)
    bad = 0
    idx = [0, n_pairs // 2, n_pairs - 1]
    for i in idx:
        sel = pairs[i:i + 1].copy()
        sel["match_off"] = 0
        m = d_matches[i * n_kp:(i + 1) * n_kp].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
        failed, wout, wres, _ = oracle.batch(kp_all, table.frame_off_host, wh, sel, m, True, True, 6.0, 1)
        kk = int(wres["n_inliers"][0])
        got = d_out[i * n_kp:i * n_kp + kk].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
        bad += 0 if (failed == 0 and res[i].tobytes() == wres[0].tobytes() and got.tobytes() == wout[:kk].tobytes()) else 1
    out["parity"] = {"pairs_checked": len(idx), "mismatches": bad, "bit_exact": bad == 0}
    return out


def config4_leg(ctx, pkg, stream, dev, n_kp=50000, steps=5):
    """BASELINE config 4: 3840 x 2160 pairs with 50k features, M = 50k putative matches per pair -- at its stated flags (rotation + scale
    hypotheses, 8 rot x 5 scale x 4 grids; 64 pairs per launch, and 256) and at the default flags (256 pairs per launch), device-resident."""
    import torch
    synth = importlib.import_module(PKG + ".synth")
    batch = importlib.import_module(PKG + ".batch")
    distmod = importlib.import_module(PKG + ".dist")
    size, n_frames = (3840, 2160), 24
    frames = synth.make_sequence(1000, n_frames, size=size, n_kp=n_kp)
    table = batch.FrameTable(ctx, frames, [size] * n_frames, device=dev)
    oracle = oracle_module()
    kp_all = np.concatenate(frames)
    wh = np.array([size] * n_frames, dtype=np.int32).reshape(-1)
    out = {"workload": f"config4: {size[0]} x {size[1]} pairs, {n_kp} keypoints per frame, M = {n_kp} putative matches per pair, device-resident"}
    for tag, n_pairs, rot, scale in (("rot_scale", 64, True, True), ("rot_scale_256_pairs", 256, True, True), ("default_flags", 256, False, False)):
        pairs = distmod.pair_table(n_frames, 0, n_pairs, n_kp)
        d_pairs = torch.from_numpy(pairs.view(np.uint8).reshape(-1)).to(dev)
        d_matches = distmod.synth_matches_device(0, n_pairs, n_kp, 0.5, dev)
        d_out = torch.zeros((n_pairs * n_kp, 4), dtype=torch.int32, device=dev)
        d_res = torch.zeros((n_pairs, 4), dtype=torch.int32, device=dev)
        ctx.reserve(n_pairs, n_kp, rot, scale)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        with torch.cuda.stream(stream):
            for s in range(-2, steps):
                if s >= 0:
                    ev[s][0].record(stream)
                ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), n_frames, d_pairs.data_ptr(), n_pairs, n_kp,
                                  d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, rot, scale, 6.0)
                if s >= 0:
                    ev[s][1].record(stream)
        torch.cuda.synchronize()
        ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
        res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
        kept = float(res["n_inliers"].astype(np.int64).sum())
        alg = 32.0 * n_kp * n_pairs + 16.0 * kept
        bad = 0
        for i in (0, n_pairs - 1):
            sel = pairs[i:i + 1].copy()
            sel["match_off"] = 0
            m = d_matches[i * n_kp:(i + 1) * n_kp].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
            failed, wout, wres, _ = oracle.batch(kp_all, table.frame_off_host, wh, sel, m, rot, scale, 6.0, 1)
            k = int(wres["n_inliers"][0])
            got = d_out[i * n_kp:i * n_kp + k].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
            bad += 0 if (failed == 0 and res[i].tobytes() == wres[0].tobytes() and got.tobytes() == wout[:k].tobytes()) else 1
        out[tag] = {"flags": [rot, scale, 6.0], "pairs_per_launch": n_pairs, "value": n_pairs / (ms * 1e-3), "unit": "pairs/s", "ms_per_launch": ms,
                    "mean_kept_per_pair": kept / n_pairs,
                    "roofline": {"bound": "hbm", "achieved": alg / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                 "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                                 "kernel": "all kernels of the launch (HIP events around gms_filter_device)",
                                 "kernel_ms_per_launch": ms, "algorithmic_bytes_per_launch": alg},
                    "parity": {"pairs_checked": 2, "mismatches": bad, "bit_exact": bad == 0}}
    return out


def poses_leg(ctx, pkg, stream, dev, n_frames=46, n_kp=10000, n_pairs=1024, steps=3):
    """Descriptors resident in HBM -> poses, the reference's SIFT_matchGMS + structureFromMotion per pair (FeatureMatchUtil.cpp:58-69 ->
    SfMUtil.cpp:25-82) for a batch, nothing leaving the GPU in between: gms_bfmatch_device -> gms_filter_device(true, true, 6.0) ->
    gms_two_view_batch_device (gather, findEssentialMat(RANSAC, 0.7, 1.0), recoverPose, undistort + triangulate). Input: n_frames
    calibrated views of one rigid scene (synth.make_multi_view_scene), the first n_pairs of its pairs."""
    import torch
    synth = importlib.import_module(PKG + ".synth")
    batch = importlib.import_module(PKG + ".batch")
    types = importlib.import_module(PKG + ".types")
    distmod = importlib.import_module(PKG + ".dist")
    sc = synth.make_multi_view_scene(77, n_frames, size=SIZE, n_kp=n_kp, dist=(-0.12, 0.05, 0.001, -0.0007, 0.01))
    n_pairs = min(n_pairs, n_frames * (n_frames - 1) // 2)
    table = batch.FrameTable(ctx, sc["frames"], sc["sizes"], device=dev)
    d_desc = distmod.synth_descriptors_device(n_frames, n_kp, "orb", 0.3, dev)
    code = pkg.GMS_DESC_HAMMING256
    d_prep = torch.zeros(max(ctx.bf_prepared_bytes(code, table.total, n_frames), 16), dtype=torch.uint8, device=dev)
    pairs = distmod.pair_table(n_frames, 0, n_pairs, n_kp)
    d_pairs = torch.from_numpy(pairs.view(np.uint8).reshape(-1)).to(dev)
    total = n_pairs * n_kp
    d_matches = torch.zeros((total, 4), dtype=torch.int32, device=dev)
    d_out = torch.zeros((total, 4), dtype=torch.int32, device=dev)
    d_res = torch.zeros((n_pairs, 4), dtype=torch.int32, device=dev)
    d_c1, d_c2 = torch.zeros(2 * total, dtype=torch.float32, device=dev), torch.zeros(2 * total, dtype=torch.float32, device=dev)
    d_mask = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_p3 = torch.zeros(3 * total, dtype=torch.float64, device=dev)
    d_tv = torch.zeros(n_pairs * types.TWO_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    cam = types.make_camera(sc["camera"], sc["dist"])
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4 * steps)]
    t0 = None
    with torch.cuda.stream(stream):
        ctx.bf_prepare_device(code, d_desc.data_ptr(), table.d_frame_off.data_ptr(), n_frames, table.total, d_prep.data_ptr())
        for s in range(-1, steps):  # one warm-up
            if s == 0:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            if s >= 0:
                ev[4 * s].record(stream)
            ctx.bfmatch_device(code, d_desc.data_ptr(), d_prep.data_ptr(), table.total, table.d_frame_off.data_ptr(), n_frames,
                               d_pairs.data_ptr(), n_pairs, n_kp, d_matches.data_ptr())
            if s >= 0:
                ev[4 * s + 1].record(stream)
            ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), n_frames, d_pairs.data_ptr(), n_pairs, n_kp,
                              d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, True, True, 6.0)
            if s >= 0:
                ev[4 * s + 2].record(stream)
            ctx.two_view_batch_device(cam, table.d_kp.data_ptr(), table.d_frame_off.data_ptr(), n_frames, d_pairs.data_ptr(), n_pairs, n_kp,
                                      d_out.data_ptr(), d_res.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), d_mask.data_ptr(), d_p3.data_ptr(),
                                      d_tv.data_ptr(), 0.7, 1.0, 1000)
            if s >= 0:
                ev[4 * s + 3].record(stream)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [float(np.mean([ev[4 * s + k].elapsed_time(ev[4 * s + k + 1]) for s in range(steps)])) for k in range(3)]
    res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
    tv = d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE)
    ok = tv["status"] == 0
    # how good the poses are: rotation error against the scene's relative rotation
    rot_err = []
    for i in np.flatnonzero(ok):
        a, b = int(pairs["frame_a"][i]), int(pairs["frame_b"][i])
        Rrel = sc["R"][b] @ sc["R"][a].T
        rot_err.append(np.degrees(np.arccos(np.clip((np.trace(tv["R"][i] @ Rrel.T) - 1) / 2, -1, 1))))
    # parity on the first and the last pair, end to end: oracle matcher -> oracle filter -> numpy two-view chain
    oracle = oracle_module()
    import sfm_ref
    desc_h = d_desc.cpu().numpy()
    bad = 0
    failed_checks = []
    checked = sorted(set(int(v) for v in np.linspace(0, n_pairs - 1, 16)))   # sixteen pairs spread over the launch, first and last included
    for i in checked:
        a, b = int(pairs["frame_a"][i]), int(pairs["frame_b"][i])
        want_m = oracle.bf_match(desc_h[a * n_kp:(a + 1) * n_kp], desc_h[b * n_kp:(b + 1) * n_kp], True)
        rc, want, _, wres = oracle.match(SIZE, SIZE, sc["frames"][a], sc["frames"][b], want_m, True, True, 6.0)
        k = len(want)
        got_o = d_out[i * n_kp:i * n_kp + k].cpu().numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
        _, w1, w2 = oracle.gather(sc["frames"][a], sc["frames"][b], want)
        ref = sfm_ref.two_view(w1, w2, sc["camera"], sc["dist"], 0.7, 1.0)
        checks = {"filter": rc == 0 and res[i].tobytes() == wres.tobytes() and got_o.tobytes() == want.tobytes(),
                  "model": ref["E"] is not None and int(tv["status"][i]) == 0}
        if checks["model"]:
            checks.update(ransac_count=int(tv["n_ransac"][i]) == ref["n_ransac"], ransac_iters=int(tv["ransac_iters"][i]) == ref["iters"],
                          E=bool(np.abs(tv["E"][i] - ref["E"]).max() < 1e-9), R=bool(np.abs(tv["R"][i] - ref["R"]).max() < 1e-9),
                          mask=bool(np.array_equal(d_mask[i * n_kp:i * n_kp + k].cpu().numpy(), ref["mask"])))
        failed_checks += [f"pair {i}: {name}" for name, good in checks.items() if not good]
        bad += 0 if all(checks.values()) else 1
    return {"workload": f"{n_frames} calibrated 1080p views of one rigid scene x {n_kp} keypoints, ORB rows resident in HBM -> BFMatcher::match -> "
                        f"matchGMS(true, true, 6.0) -> gather -> findEssentialMat(RANSAC, 0.7, 1.0) -> recoverPose -> undistortPoints -> "
                        f"triangulatePoints for {n_pairs} pairs per step (SfMUtil.cpp:17-82 per pair); nothing leaves the GPU in between",
            "value": n_pairs * steps / wall, "unit": "pairs/s", "pairs_per_step": n_pairs, "matcher_ms_per_step": ms[0],
            "filter_ms_per_step": ms[1], "two_view_ms_per_step": ms[2], "poses_found": int(ok.sum()),
            "mean_kept_per_pair": float(res["n_inliers"].mean()), "mean_ransac_iters": float(tv["ransac_iters"][ok].mean()) if ok.any() else None,
            "mean_triangulated_per_pair": float(tv["n_triangulated"][ok].mean()) if ok.any() else None,
            "median_rotation_error_deg": float(np.median(rot_err)) if rot_err else None,
            "parity": {"pairs_checked": len(checked), "mismatches": bad, "ok": bad == 0, "failed_checks": failed_checks,
                       "rule": "sixteen pairs spread over the launch: matches, survivors and results bit-exact vs oracle/bf_ref.c + oracle/gms_ref.c; RANSAC decisions "
                               "(iterations, masks, counts) equal and E, R within 1e-9 of oracle/sfm_ref.py (fp64, parity unpinned: OpenCV's calib3d "
                               "is an import library in the reference)"}}


def pixels_leg(ctx, pkg, stream, dev, n_images=32, max_kp=10000, threshold=20, steps=5):
    """f2: pixels resident in HBM -> keypoints + 32-byte rows for a batch of 1080p frames (the place of SIFT::create(10000)->
    detectAndCompute, FeatureMatchUtil.cpp:9-12): gms_detect_batch_device, FAST-9 + steered BRIEF of the library's own. Synthetic
    textured frames; image 0 and the last image checked against the CPU statement of the definition (oracle/detect_ref.c)."""
    import torch
    synth = importlib.import_module(PKG + ".synth")
    imgs = synth.make_textured_images(5, n_images, size=SIZE)
    w, h = SIZE
    d_imgs = torch.from_numpy(imgs).to(dev)
    nb = ctx.detect_workspace_bytes(w, h, n_images, max_kp)
    d_ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_kp = torch.zeros(n_images * max_kp * 28, dtype=torch.uint8, device=dev)
    d_desc = torch.zeros(n_images * max_kp * 32, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(n_images, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def run():
        ctx.detect_batch_device(d_imgs.data_ptr(), n_images, w, h, threshold, max_kp, d_ws.data_ptr(), nb, d_kp.data_ptr(), d_desc.data_ptr(),
                                d_counts.data_ptr())
    with torch.cuda.stream(stream):
        run()
        ctx.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            run()
        e1.record(stream)
        ctx.synchronize()
    ms = e0.elapsed_time(e1) / steps
    counts = d_counts.cpu().numpy()
    kp = d_kp.cpu().numpy().view(importlib.import_module(PKG + ".types").KEYPOINT_DTYPE).reshape(n_images, max_kp)
    desc = d_desc.cpu().numpy().reshape(n_images, max_kp, 32)
    oracle = oracle_module()
    bad = 0
    for i in (0, n_images - 1):
        wk, wr = oracle.detect(imgs[i], threshold, max_kp)
        same = len(wk) == counts[i] and wk.tobytes() == kp[i, :counts[i]].tobytes() and wr.tobytes() == desc[i, :counts[i]].tobytes()
        bad += 0 if same else 1
    algo = float(n_images) * w * h + float(counts.sum()) * 60.0     # pixels in, records + rows out
    return {"workload": f"{n_images} frames of {w} x {h} (synthetic textured), threshold {threshold}, at most {max_kp} keypoints per frame",
            "value": n_images / (ms * 1e-3), "unit": "frames/s", "ms_per_step": ms, "mpixels_per_s": n_images * w * h / (ms * 1e-3) / 1e6,
            "mean_keypoints_per_frame": float(counts.mean()),
            "roofline": {"bound": "hbm", "achieved": algo / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": algo / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                         "kernel": "all seven kernels of the launch (HIP events around gms_detect_batch_device)",
                         "algorithmic_bytes_per_launch": algo,
                         "note": "1 byte per pixel in, 60 bytes per keypoint out; the launch also writes and re-reads 4 bytes per pixel of "
                                 "score / candidate / box-sum planes"},
            "parity": {"images_checked": 2, "mismatches": bad, "bit_exact": bad == 0,
                       "rule": "keypoint records, their order and the descriptor bits vs oracle/detect_ref.c (the definition; not cv::ORB)"}}


def real_pixels_leg(ctx, pkg, stream, dev, copies=2048, steps=6):
    """The reference's own main() scenario (main.cpp:19-47 -> SIFT_matchGMS, FeatureMatchUtil.cpp:52-84) from real pixels: the 1920 x 1080
    pair Disparity_L / Disparity_R as it is, with the right image turned by 180 degrees, and with the right image resized to 1000 x 1000
    (tests/golden/image_main_scenario_1080p.npz). Pixels -> gms_detect_batch_device (10 000 keypoints) -> gms_bfmatch_device -> the
    filter's rate on those matches: `copies` copies of the pair per launch (every copy its own match array), at the wrapper's flags
    (true, true) and at the defaults. What the headline's uniformly random keypoints do not show: a detector's raster order and clustering."""
    import torch
    batch = importlib.import_module(PKG + ".batch")
    path = os.path.join(ROOT, "tests", "golden", "image_main_scenario_1080p.npz")
    if not os.path.exists(path):
        return {"skipped": "tests/golden/image_main_scenario_1080p.npz not found"}
    z = np.load(path)
    left, right = np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])
    images = [left, right, np.ascontiguousarray(right[::-1, ::-1]), np.ascontiguousarray(z["right_1000"])]
    thr, max_kp = 3, 10000
    kps, rows = [], []
    for img in images:
        k, r = batch.detect_images(ctx, img[None], thr, max_kp)
        kps.append(k[0])
        rows.append(r[0])
    sizes = [(im.shape[1], im.shape[0]) for im in images]
    table = batch.FrameTable(ctx, kps, sizes, device=dev)
    dt = batch.DescriptorTable(ctx, table, rows, pkg.GMS_DESC_HAMMING256)
    oracle = oracle_module()
    out = {"workload": f"main.cpp:19-47: Disparity_L / Disparity_R (1920 x 1080) from pixels, FAST threshold {thr}, at most {max_kp} keypoints per image "
                       f"(the build's FAST/BRIEF detector, not SIFT), BFMatcher::match, then {copies} copies of the pair per launch",
           "keypoints": [int(len(k)) for k in kps]}
    cx = np.minimum((kps[0]["x"] / sizes[0][0] * 20).astype(np.int64), 19)
    cy = np.minimum((kps[0]["y"] / sizes[0][1] * 20).astype(np.int64), 19)
    cells = np.bincount(cy * 20 + cx, minlength=400)
    out["left_image_cells"] = {"occupied": int((cells > 0).sum()), "max_keypoints_in_a_cell": int(cells.max()),
                               "note": "keypoints come in raster order; the byte-matrix kernel goes crowded above 255 matches in a cell of any grid type"}
    ok = True
    for name, b in (("normal", 1), ("rotated_180", 2), ("resized_1000", 3)):
        m = len(kps[0])
        one = np.zeros(1, dtype=pkg.PAIR_DTYPE)
        one[0] = (0, b, m, 0, 0)
        matches = batch.match_pairs(ctx, dt, one)
        pairs = np.zeros(copies, dtype=pkg.PAIR_DTYPE)
        pairs["frame_a"], pairs["frame_b"], pairs["m"] = 0, b, m
        pairs["match_off"] = np.arange(copies, dtype=np.int64) * m
        d_pairs = torch.from_numpy(pairs.view(np.uint8).reshape(-1)).to(dev)
        d_matches = torch.from_numpy(np.ascontiguousarray(matches).view(np.uint8).reshape(-1)).to(dev).repeat(copies)
        d_out = torch.zeros(copies * m * 16, dtype=torch.uint8, device=dev)
        d_res = torch.zeros((copies, 4), dtype=torch.int32, device=dev)
        rec = {}
        for tag, rot, scale in (("rot_scale", True, True), ("default_flags", False, False)):
            ctx.reserve(copies, m, rot, scale)
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            with torch.cuda.stream(stream):
                for s in range(-20, steps):
                    # the library picks its lane mapping (and which scales it probes) from what earlier launches of the context saw, every
                    # sixteenth launch: the timed launches are its steady state on THIS input, so a verdict cycle runs -- and lands -- first
                    if s < 0 and s % 4 == 0:
                        torch.cuda.synchronize()
                    if s >= 0:
                        ev[s][0].record(stream)
                    ctx.filter_device(table.d_pts.data_ptr(), table.d_frame_off.data_ptr(), table.n_frames, d_pairs.data_ptr(), copies, m,
                                      d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, rot, scale, 6.0)
                    if s >= 0:
                        ev[s][1].record(stream)
            torch.cuda.synchronize()
            ms = float(np.median([a.elapsed_time(bb) for a, bb in ev]))
            res = d_res.cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
            t_cpu = []
            for _ in range(3):  # the oracle on the same pair, one thread of the box's host (median of three)
                t0 = time.perf_counter()
                rc, want, _, want_res = oracle.match(sizes[0], sizes[b], kps[0], kps[b], matches, rot, scale, 6.0)
                t_cpu.append(time.perf_counter() - t0)
            k = len(want)
            bad = 0
            for i in (0, copies - 1):
                got = d_out[i * m * 16:(i * m + k) * 16].cpu().numpy().view(pkg.DMATCH_DTYPE)
                bad += 0 if (rc == 0 and int(res["n_inliers"][i]) == k and got.tobytes() == want.tobytes()
                             and (int(res["best_scale"][i]), int(res["best_rot"][i])) == (int(want_res[1]), int(want_res[2]))) else 1
            ok = ok and bad == 0
            alg = (32.0 * m + 16.0 * k) * copies
            rec[tag] = {"flags": [rot, scale, 6.0], "value": copies / (ms * 1e-3), "unit": "pairs/s", "ms_per_launch": ms, "kept": k,
                        "winner": [int(want_res[1]), int(want_res[2])], "dealt_lane_mapping": bool(ctx.query(1)),
                        "cpu_oracle_pairs_per_s_1_thread": 1.0 / float(np.median(t_cpu)),
                        "roofline": {"bound": "hbm", "achieved": alg / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                     "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                                     "kernel": "all kernels of the launch (HIP events around gms_filter_device)", "kernel_ms_per_launch": ms,
                                     "algorithmic_bytes_per_launch": alg},
                        "parity": {"pairs_checked": 2, "mismatches": bad, "bit_exact": bad == 0}}
        rec["matches"] = int(m)
        rec["image_sizes"] = [list(sizes[0]), list(sizes[b])]
        out[name] = rec
    out["parity_ok"] = ok
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)")

    import torch
    pkg = importlib.import_module(PKG)
    distmod = importlib.import_module(PKG + ".dist")
    # GMS_BENCH_ONE_DEVICE=1 is a rehearsal mode for a one-GPU box: every rank uses cuda:0. The driver never sets it.
    one_device = os.environ.get("GMS_BENCH_ONE_DEVICE", "0") == "1"
    dev_index = 0 if one_device else local_rank
    dist = distmod.init_rendezvous(world)  # gloo; None for one rank
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)

    ctx = pkg.GmsContext(dev_index)  # raises if the HIP extension is missing: no fallback
    stream = torch.cuda.Stream(device=dev)
    wl = Workload(args, rank, world, dev, pkg, ctx)
    ctx.set_stream(stream.cuda_stream)
    n_res = len(wl.chunks)

    wall, kern_ms = timed_steps(ctx, wl, stream, args.steps, args.warmup, False, False, dist)
    wall_max = distmod.max_over_ranks(wall, dist)  # whole-job time = the slowest rank
    variant = {"dealt": bool(ctx.query(1)), "matches_per_thread": ctx.query(3),  # which bit-identical instantiation the timed launches ran
               "touch_ahead": {"before_grid_type": ctx.query(6), "pairs_ahead": ctx.query(7)}, "first_round_stagger_us": ctx.query(8) / 100.0}
    value = wl.n_pairs * world * args.steps / wall_max
    dumped = None
    if args.dump_outputs and rank == 0:  # before anything else launches on the chunks
        dumped = dump_outputs(wl, pkg, (args.warmup + args.steps - 1) % n_res, args.dump_outputs)

    # ---- --full: parity on every rank, the sampled pairs of every resident chunk, as the timed launches left them
    ok = True
    if args.full:
        checked, bad = check_parity(wl, pkg, range(n_res), False, False)
        checked_all, bad_all = distmod.sum_over_ranks([checked, bad], dist)
        ok = bad_all == 0
    if rank == 0:
        n_kp = wl.n_kp
        kept = 0
        for ch in wl.chunks:
            res = ch["d_res"].cpu().numpy().view(pkg.RESULT_DTYPE).reshape(-1)
            assert (res["status"] == 0).all()
            kept += int(res["n_inliers"].astype(np.int64).sum())
        kept_per_launch = kept / n_res
        # algorithmic bytes per launch: 32*M + 16*K per pair
        alg_bytes = 32.0 * n_kp * wl.n_pairs + 16.0 * kept_per_launch
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
        line = {
            "metric": "gms_filtered_image_pairs_per_sec", "value": value, "unit": "pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": wall_max / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "i32", "data": "synthetic",
            "config": {"workload": "config3: one 1080p sequence, all N(N-1)/2 pairs in lexicographic order, 10k keypoints/frame, "
                                   "M=10k putative matches/pair, matchGMS(withRotation=false, withScale=false, thresholdFactor=6.0)",
                       "image_size": list(SIZE), "frames": args.frames, "features": n_kp,
                       "frame_table_bytes": wl.frame_table_bytes, "total_pairs": wl.plan.total_pairs,
                       "pairs_per_step_per_gpu": wl.n_pairs, "resident_chunks_per_gpu": n_res,
                       "inlier_frac": args.inlier_frac, "mean_kept_per_pair": kept_per_launch / wl.n_pairs,
                       "sharding": f"contiguous blocks of the pair list x{world}, no collective; rendezvous over gloo"},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "traffic": None,
                         "kernel": f"gms::filter_kernel_dense<{variant['matches_per_thread']}, false, 1024, {str(variant['dealt']).lower()}>",
                         "kernel_ms_per_launch": kern_ms, "algorithmic_bytes_per_launch": alg_bytes},
            "variant": dict(variant, note="the library picks between bit-identical instantiations from what earlier launches saw "
                                          "(gms_ctx_query); GMS_DEAL=0|1 forces one"),
            "frame_table_build_ms": wl.frame_table_build_ms,
            "frame_table_note": f"gms_normalize_device over {args.frames} frames x {n_kp} keypoints (normalizePoints + per-keypoint cell codes), "
                                "once per sequence, outside the timed steps: every frame serves frames - 1 pairs",
        }
        if args.full:
            line["parity"] = {"pairs_checked": checked_all, "mismatches": bad_all, "bit_exact": ok,
                              "rule": f"every {distmod.PARITY_EVERY}th global pair of every resident chunk, on every rank, vs oracle/gms_ref.c"}
            line["opencv_on_box"] = opencv_on_box()
        if dumped is not None:
            line["dump_outputs"] = dumped
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if args.full and os.path.exists(tpath):  # measured in a separate rocprofv3 --pmc run (tools/pmc_collect.sh), not in this one
            try:
                tj = json.load(open(tpath))
                line["roofline"]["traffic_from_profiles"] = tj
                # the counter figure belongs to a named kernel at a named batch size: it is this launch's traffic only when both agree
                if tj.get("kernel") == line["roofline"]["kernel"] and tj.get("pairs_per_launch") == wl.n_pairs:
                    line["roofline"]["traffic"] = float(tj["hbm_bytes_per_launch"])
                    line["roofline"]["traffic_source"] = ("profiles/traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over this command "
                                                          "(tools/pmc_collect.sh), FETCH_SIZE x2 per MI355X_MICROARCH.md, bytes per launch of this kernel")
            except Exception:
                pass
        if args.full and not args.no_cpu and world == 1:
            line["cpu_baseline"] = cpu_baseline(args, wl, pkg, False, False, budget_s=12.0)
            line["gpu_vs_cpu"] = value / line["cpu_baseline"]["value"]
        if args.full and not args.no_extra and world == 1:
            # the reference's SfM call-site flags on the head of the same chunks
            n_sub = min(wl.n_pairs, 2048)
            w2, k2 = timed_steps(ctx, wl, stream, 8, 2, True, True, None, n_pairs=n_sub)
            probe_mask = ctx.query(2)
            used = sorted({(2 + s) % n_res for s in range(8)})
            c2, b2 = check_parity(wl, pkg, used, True, True, sample={c: list(range(0, n_sub, 389)) for c in used})
            kept2 = np.mean([int(wl.chunks[c]["d_res"][:n_sub, 0].sum().item()) for c in used])
            alg2 = 32.0 * n_kp * n_sub + 16.0 * kept2
            extra = {"workload": "head of the same chunks, matchGMS(withRotation=true, withScale=true, 6.0) "
                                 "(FeatureMatchUtil.cpp:69 flags), 8 rot x 5 scale x 4 grids",
                     "pairs_per_step": n_sub, "value": n_sub * 8 / w2, "unit": "pairs/s", "ms_per_step": k2,
                     "scale_probe": {"mask": probe_mask, "note": "bit s set = scale hypothesis s was bounded by a probe before being "
                                     "evaluated in the timed launches (the library's own choice, gms_ctx_query; gms_ctx_set_option / GMS_SCALE_PROBE force it)"},
                     "roofline": {"bound": "hbm", "achieved": alg2 / (k2 * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                  "frac": alg2 / (k2 * 1e-3) / 1e9 / HBM_PEAK_GBPS, "traffic": None,
                                  "kernel": "all kernels of the launch (HIP events around gms_filter_device)",
                                  "kernel_ms_per_launch": k2, "algorithmic_bytes_per_launch": alg2},
                     "parity": {"pairs_checked": c2, "mismatches": b2, "bit_exact": b2 == 0}}
            ok = ok and b2 == 0
            # the scale probe is the library's own choice (it pays when most probed scales cannot win): the same launches with it
            # forced off and on, here and on a zooming sequence where a probed scale wins (the 28 x 28 grid: the probe cannot bound it out)
            extra["by_probe"] = {}
            for name, val in (("off", 0), ("on", 1)):
                ctx.set_option(2, val)
                wv, kv = timed_steps(ctx, wl, stream, 6, 2, True, True, None, n_pairs=n_sub)
                extra["by_probe"][name] = {"pairs_per_s": n_sub * 6 / wv, "ms_per_step": kv}
            ctx.set_option(2, -1)
            extra["zoom"] = zoom_leg(ctx, pkg, stream, dev)
            ok = ok and extra["zoom"]["parity"]["bit_exact"]
            if not args.no_cpu:
                extra["cpu_baseline"] = cpu_baseline(args, wl, pkg, True, True, budget_s=12.0)
                extra["gpu_vs_cpu"] = extra["value"] / extra["cpu_baseline"]["value"]
            line["rot_scale"] = extra
            # f1: the producer in front of the filter (FeatureMatchUtil.cpp:66-68), ORB rows (BASELINE's wording) and SIFT rows
            # (what the reference feeds)
            line["descriptors_to_filtered_matches"] = {k: bf_gms_leg(ctx, wl, pkg, stream, k) for k in ("orb", "sift")}
            ok = ok and all(v["parity"]["bit_exact"] for v in line["descriptors_to_filtered_matches"].values())
            line["config4"] = config4_leg(ctx, pkg, stream, dev)
            ok = ok and all(line["config4"][t]["parity"]["bit_exact"] for t in ("rot_scale", "default_flags"))
            # f3: the consumer behind the filter, batched (SfMUtil.cpp:25-82)
            line["descriptors_to_poses"] = poses_leg(ctx, pkg, stream, dev)
            ok = ok and line["descriptors_to_poses"]["parity"]["ok"]
            # f2: the keypoint source in front of the matcher
            line["pixels_to_keypoints"] = pixels_leg(ctx, pkg, stream, dev)
            ok = ok and line["pixels_to_keypoints"]["parity"]["bit_exact"]
            # BASELINE configs 1 / 2 on real pixels: the reference's own main() scenario
            line["real_pixels"] = real_pixels_leg(ctx, pkg, stream, dev)
            ok = ok and line["real_pixels"].get("parity_ok", True)
        print(json.dumps(line))
        sys.stdout.flush()
    distmod.barrier(dist)
    if dist is not None:
        dist.destroy_process_group()
    ctx.close()
    if not ok:
        sys.exit("bench.py: GPU output differs from the oracle on the parity sample")


if __name__ == "__main__":
    main()
