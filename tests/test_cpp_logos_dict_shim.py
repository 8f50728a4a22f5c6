"""The header-only C++ shim's dictionary trainer (sfm-gms_amd/include/mi355_gms.hpp): mi355::trainLogosDictionary on flat 128-float
and 32-byte rows. CPU: it compiles and links against libgms_hip.so. GPU: it gives the dictionary, labels and record of
tests/logos_dict_ref.py."""

import numpy as np
import pytest

import logos_dict_ref as ref
import hostbuild as hb


def test_logos_dict_shim_compiles_and_links():
    exe = hb.shim_exe("logos_dict_shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 2 and "usage" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_logos_dict_shim_equals_the_statement(tmp_path, kind):
    exe = hb.shim_exe("logos_dict_shim_main.cpp")
    rng = np.random.default_rng(5 + kind)
    n, n_words, attempts, max_iters, seed = 700, 20, 2, 25, 2**63 + 5
    if kind == 0:
        rows = rng.integers(0, 256, (8, 32), dtype=np.uint8)[rng.integers(0, 8, n)] ^ np.packbits(rng.random((n, 256)) < 0.1, axis=1)
    else:
        rows = (rng.uniform(0, 200, (8, 128))[rng.integers(0, 8, n)] + rng.normal(0, 10, (n, 128))).astype(np.float32)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([kind, n, n_words, attempts, max_iters], np.int32).tobytes() + np.uint64(seed).tobytes() + rows.tobytes())
    res = hb.run(exe, path, timeout=600)
    assert res.returncode == 0, res.stderr
    dic, rec, labels = ref.train_set(rows, kind, n_words, attempts, max_iters, seed)
    lines = res.stdout.splitlines()
    assert lines[0].split() == [str(hb.fnv1a(dic.tobytes())), str(hb.fnv1a(labels.tobytes())), str(rec["attempt"]), str(rec["iterations"]),
                                str(rec["empty_clusters"]), str(rec["compactness"])]
    assert lines[1].split() == ["1"]
