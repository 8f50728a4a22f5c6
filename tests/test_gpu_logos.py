"""GPU: gms_logos_match / matchLOGOS (the LOGOS match filter, sfm-gms_amd/csrc/logos_kernels.hip) against the reference DLL's own
outputs (tests/golden/refdll_logos.npz) and the numpy restatement tests/logos_ref.py."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import logos_ref
from logos_gpu import kp_records as _kp, want_dmatch as _want_dmatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("sfm-gms_amd")
Z = np.load(os.path.join(ROOT, "tests", "golden", "refdll_logos.npz"))
NAMES = sorted(k[: -len("_matches")] for k in Z.files if k.endswith("_matches"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_equals_dll_fixture(name):
    got = pkg.matchLOGOS(_kp(Z[name + "_kp1"]), _kp(Z[name + "_kp2"]), Z[name + "_nn1"], Z[name + "_nn2"])
    assert got.tobytes() == _want_dmatch(Z[name + "_matches"]).tobytes()


def _moved(kp, theta, scale, t):
    c, s = np.cos(theta), np.sin(theta)
    out = kp.copy()
    out[:, 0] = scale * (c * kp[:, 0] - s * kp[:, 1]) + t[0]
    out[:, 1] = scale * (s * kp[:, 0] + c * kp[:, 1]) + t[1]
    out[:, 2] = kp[:, 2] * scale
    out[:, 3] = np.mod(kp[:, 3] - np.degrees(theta), 360.0)
    return out.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_equals_restatement_seeded(seed):
    rng = np.random.default_rng(1000 + seed)
    n1, n2 = [(1, 40), (3, 7), (40, 1), (500, 450), (1500, 1600), (800, 800)][seed]
    kp1 = np.stack([rng.integers(0, 200, n1), rng.integers(0, 150, n1), rng.uniform(2, 20, n1), rng.uniform(0, 360, n1)],
                   1).astype(np.float32)
    if n1 == n2:
        kp2 = _moved(kp1, rng.uniform(-3, 3), rng.uniform(0.6, 1.6), (4.0, -3.0))
        l1 = rng.integers(0, 12, n1)
        l2 = l1.copy()
        l2[: n2 // 4] = rng.integers(0, 12, n2 // 4)
    else:
        kp2 = np.stack([rng.uniform(0, 200, n2), rng.uniform(0, 150, n2), rng.uniform(2, 20, n2), rng.uniform(0, 360, n2)],
                       1).astype(np.float32)
        l1, l2 = rng.integers(0, 4, n1), rng.integers(0, 4, n2)
    want = logos_ref.match(kp1, kp2, l1, l2)
    got = pkg.matchLOGOS(_kp(kp1), _kp(kp2), l1, l2)
    assert got.tobytes() == _want_dmatch(want).tobytes()
    if n1 == n2:
        assert len(want) > 0


@pytest.mark.gpu
def test_overflow_reports_needed_count_and_result_record():
    lib = pkg.load_library()
    name = "rot30_s1.3"
    kp1, kp2 = _kp(Z[name + "_kp1"]), _kp(Z[name + "_kp2"])
    l1, l2 = Z[name + "_nn1"].astype(np.int32), Z[name + "_nn2"].astype(np.int32)
    need = len(Z[name + "_matches"])
    _, (n_cand, n_supp, peak) = logos_ref.match(Z[name + "_kp1"], Z[name + "_kp2"], l1, l2, detail=True)

    class Res(C.Structure):
        _fields_ = [("n_candidates", C.c_int64), ("n_supported", C.c_int64), ("n_out", C.c_int64), ("peak_bin", C.c_int32),
                    ("status", C.c_int32)]

    out = np.zeros(need, pkg.DMATCH_DTYPE)
    n = C.c_int64(-1)
    res = Res()
    rc = lib.gms_logos_match(kp1.ctypes.data, len(kp1), kp2.ctypes.data, len(kp2), l1.ctypes.data, l2.ctypes.data,
                             out.ctypes.data, need - 1, C.byref(n), C.byref(res))
    assert rc == pkg.types.GMS_ERR_CAPACITY and n.value == need and res.n_out == need and res.status == rc
    assert not out.view(np.uint8).any()
    rc = lib.gms_logos_match(kp1.ctypes.data, len(kp1), kp2.ctypes.data, len(kp2), l1.ctypes.data, l2.ctypes.data,
                             out.ctypes.data, need, C.byref(n), C.byref(res))
    assert rc == 0 and n.value == need
    assert (res.n_candidates, res.n_supported, res.peak_bin) == (n_cand, n_supp, peak)
    assert out.tobytes() == _want_dmatch(Z[name + "_matches"]).tobytes()


@pytest.mark.gpu
def test_bad_arguments():
    lib = pkg.load_library()
    n = C.c_int64(0)
    assert lib.gms_logos_match(None, -1, None, 0, None, None, None, 0, C.byref(n), None) == pkg.types.GMS_ERR_BAD_ARG
    assert lib.gms_logos_match(None, 3, None, 0, None, None, None, 0, C.byref(n), None) == pkg.types.GMS_ERR_BAD_ARG
    with pytest.raises(ValueError):
        pkg.matchLOGOS(_kp(np.zeros((2, 4))), _kp(np.zeros((2, 4))), [0], [0, 1])


@pytest.mark.gpu
def test_no_support_reports_peak_minus_one():
    lib = pkg.load_library()
    name = "random_n300"
    kp1, kp2 = _kp(Z[name + "_kp1"]), _kp(Z[name + "_kp2"])
    l1, l2 = Z[name + "_nn1"].astype(np.int32), Z[name + "_nn2"].astype(np.int32)
    _, (n_cand, n_supp, peak) = logos_ref.match(Z[name + "_kp1"], Z[name + "_kp2"], l1, l2, detail=True)
    res = (C.c_int64 * 4)()
    n = C.c_int64(-1)
    out = np.zeros(1, pkg.DMATCH_DTYPE)
    assert lib.gms_logos_match(kp1.ctypes.data, len(kp1), kp2.ctypes.data, len(kp2), l1.ctypes.data, l2.ctypes.data,
                               out.ctypes.data, 1, C.byref(n), C.byref(res)) == 0
    peak_bin = np.frombuffer(bytes(res), np.int32)[6]
    assert n.value == 0 and n_supp == 0 and peak == -1 and peak_bin == -1 and res[0] == n_cand
