"""-m gpu: bench.py on a small sequence -- --steps sets the timed steps the line reports, and --dump-outputs writes the same
arrays from run to run (the inputs are a pure function of the arguments), which agree with the line's own parity check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "64",
           "--features", "2000", "--pairs", "256", "--no-cpu", "--no-extra", "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_dump_outputs_are_reproducible(tmp_path):
    a, b = _bench(tmp_path / "a"), _bench(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["parity"]["bit_exact"]
        assert line["dump_outputs"]["step_chunk"] == 3 and line["dump_outputs"]["pairs"] == 256
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["results.npy", "sample_matches.npy", "sample_pairs.npy"]
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    res = np.load(tmp_path / "a" / "results.npy")
    sp = np.load(tmp_path / "a" / "sample_pairs.npy")
    assert res.shape == (256, 4) and (res[:, 3] == 0).all() and res[:, 0].sum() > 0  # status 0, something survives
    assert np.array_equal(sp[:, 3], res[sp[:, 0].astype(np.int64), 0])
    assert len(np.load(tmp_path / "a" / "sample_matches.npy")) == sp[:, 3].sum()
