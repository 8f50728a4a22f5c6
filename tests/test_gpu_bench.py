"""-m gpu: bench.py on a small sequence -- --steps sets the timed steps the line reports, and --dump-outputs writes the same
arrays from run to run (the inputs are a pure function of the arguments), which agree with the --full line's parity check;
a plain run writes the same arrays and a line with the headline alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, full=True):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "64",
           "--features", "2000", "--pairs", "256", "--dump-outputs", str(out_dir)]
    if full:
        cmd += ["--full", "--no-cpu", "--no-extra"]
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


def test_plain_bench_is_the_headline_alone(tmp_path):
    plain, full = _bench(tmp_path / "plain", full=False), _bench(tmp_path / "full")
    assert plain["metric"] == full["metric"] == "gms_filtered_image_pairs_per_sec" and plain["value"] > 0
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert (plain["unit"], plain["higher_is_better"], plain["dtype"]) == (full["unit"], full["higher_is_better"], full["dtype"])
    assert plain["roofline"]["kernel_ms_per_launch"] > 0 and "traffic_from_profiles" not in plain["roofline"]
    assert not {"parity", "opencv_on_box", "cpu_baseline", "rot_scale"} & set(plain)
    assert full["parity"]["bit_exact"]
    assert plain["dump_outputs"] == dict(full["dump_outputs"], dir=str(tmp_path / "plain"))
    files = sorted(os.listdir(tmp_path / "full"))
    assert sorted(os.listdir(tmp_path / "plain")) == files
    for f in files:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "full" / f).read_bytes(), f
