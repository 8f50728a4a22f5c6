"""The header-only C++ shim's bruteForceMatch entry points (sfm-gms_amd/include/mi355_gms.hpp): mi355::bruteForceMatch on flat
128-float and 32-byte rows, and mi355::bruteForceMatchBatch. CPU: they compile and link against libgms_hip.so. GPU: both give the
survivors of tests/bf_select_ref.py."""

import numpy as np
import pytest

import bf_select_ref
import hostbuild as hb


def test_bf_shim_compiles_and_links():
    exe = hb.shim_exe("bf_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_bf_shim_matches_restatement(tmp_path, kind):
    exe = hb.shim_exe("bf_shim_main.cpp")
    rng = np.random.default_rng(71 + kind)
    if kind == 0:
        rows = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (400, 65, 1025)]
    else:
        rows = [np.where(rng.uniform(size=(n, 128)) < 0.4, rng.integers(0, 30, (n, 128)), 0).astype(np.float32) for n in (400, 65, 1025)]
    rows[2][:300] = rows[0][:300]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (2, 1)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([kind, len(rows)], np.int32).tobytes())
        for r in rows:
            f.write(np.int32(len(r)).tobytes() + r.tobytes())
        f.write(np.int32(len(pairs)).tobytes() + np.asarray(pairs, np.int32).tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 2 * len(pairs)
    for k, (a, b) in enumerate(pairs):
        want, _, _, _ = bf_select_ref.bf_match_select(rows[a], rows[b], kind == 0)
        assert lines[k].split() == [str(len(want)), str(hb.fnv1a(want.tobytes(), words=True))]
        assert lines[len(pairs) + k].split() == [str(len(want)), str(hb.fnv1a(want.tobytes(), words=True)), "1"]
