#!/usr/bin/env python3
"""Diagnostic A/B: the headline bench on two (or more) builds of the library in ONE session on ONE device (timings from different
boxes differ by 1-3 %). python tools/ab_bench.py [--rounds N] libA.so libB.so [more libs] [bench args...]; alternates A, B, A, B, ...
N times (default 2). A library may carry environment settings of its own in front, comma-separated: GMS_IDENT=0,libB.so (the same
build twice with different switches). Ends with each entry's fastest / slowest / mean kernel time."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
argv = sys.argv[1:]
rounds = 2
if argv[:1] == ["--rounds"]:
    rounds, argv = int(argv[1]), argv[2:]
n_libs = next((i for i, a in enumerate(argv) if a.startswith("-")), len(argv))
entries, extra = argv[:n_libs], argv[n_libs:]
code = """
import importlib, sys
sys.path.insert(0, {root!r}); sys.argv = ['bench.py', '--full', '--no-cpu', '--no-extra'] + {extra!r}
capi = importlib.import_module('sfm-gms_amd.capi'); capi.library_path = lambda: {lib!r}
import torch, ctypes; built = ctypes.CDLL({lib!r})  # (an older build: the entry points it does not have yet are not bound)
for name in [n for n in capi.SIGNATURES if not hasattr(built, n)]: del capi.SIGNATURES[name]
import bench; bench.main()
"""
times = {e: [] for e in entries}
for rnd in range(rounds):
    for entry in entries:
        *settings, lib = entry.split(",")
        env = dict(os.environ, **dict(s.split("=", 1) for s in settings))
        r = subprocess.run([sys.executable, "-c", code.format(root=ROOT, extra=extra, lib=os.path.abspath(lib))], capture_output=True, text=True, env=env, timeout=600)
        label = " ".join(settings + [os.path.basename(lib)])
        try:
            d = json.loads(r.stdout.strip().splitlines()[-1])
            times[entry].append(d["roofline"]["kernel_ms_per_launch"])
            print(label, round(d["roofline"]["kernel_ms_per_launch"], 4), "ms/launch", round(d["value"]), "pairs/s", d["parity"]["bit_exact"],
                  "frame_table_build_ms", round(d.get("frame_table_build_ms", float("nan")), 3), flush=True)
        except Exception:
            print(label, "failed", r.returncode, r.stderr[-300:], flush=True)
            sys.exit(1)  # (nothing more is started on a device behind a run that failed)
for entry, t in times.items():
    if t:
        print("summary", entry, "n", len(t), "min", round(min(t), 4), "max", round(max(t), 4), "mean", round(sum(t) / len(t), 4), flush=True)
