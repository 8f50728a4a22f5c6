"""CPU: the restatement of the reference's bruteForceMatch (tests/bf_select_ref.py) and the host build of the kernels' sort
(sfm-gms_amd/csrc/bf_select_core.h through tests/cpp/bf_select_host.cpp).

The sort is pinned by tests/golden/refdll_logos.npz: its sort_* cases are full orders out of the reference DLL's own std::sort
instance (predicate a.d < b.d on a float alone -- the shape of DMatch::operator<). The reference's executable is not at hand, so its
own instance of the template cannot be run; the cross-check rule is restated from OpenCV's published batchDistance."""
import ctypes as C
import os

import numpy as np
import pytest

import bf_select_ref
import logos_ref
import hostbuild as hb

Z = np.load(os.path.join(hb.ROOT, "tests", "golden", "refdll_logos.npz"))
SORTS = sorted(int(k.split("_")[1]) for k in Z.files if k.startswith("sort_") and k.endswith("_order"))


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(hb.host_lib("bf_select_host.cpp"))
    lib.bf_host_sort_prefix.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long]
    return lib


def _ref_prefix(d, k):
    dl, il = [np.float32(x) for x in d], list(range(len(d)))
    bf_select_ref.msvc_sort_prefix(dl, il, k)
    return np.asarray(il, np.int32), np.asarray(dl, np.float32)


def _host_prefix(host, d, k):
    dc = np.ascontiguousarray(d, np.float32).copy()
    ic = np.arange(len(d), dtype=np.int32)
    host.bf_host_sort_prefix(dc.ctypes.data, ic.ctypes.data, len(d), k)
    return ic, dc


def test_fixture_sorts_are_full_orders():
    assert SORTS and max(len(Z[f"sort_{t}_d"]) for t in SORTS) >= 20000
    for t in SORTS:
        d, order = Z[f"sort_{t}_d"], Z[f"sort_{t}_order"]
        assert sorted(order.tolist()) == list(range(len(d)))
        assert np.all(np.diff(d[order]) >= 0)


@pytest.mark.parametrize("t", SORTS)
def test_general_sort_reproduces_dll_order(host, t):
    """The whole permutation of the DLL's std::sort, from the restatement and from the kernels' header alike."""
    d, want = Z[f"sort_{t}_d"], Z[f"sort_{t}_order"].astype(np.int32)
    n = len(d)
    got, _ = _ref_prefix(d, n)
    assert got.tobytes() == want.tobytes()
    got_h, d_h = _host_prefix(host, d, n)
    assert got_h.tobytes() == want.tobytes()
    assert d_h.tobytes() == d[want].tobytes()
    if n > 40:  # the ties really are broken in an order of the sort's own, not the stable one
        assert got.tolist() != np.argsort(d, kind="stable").tolist()


@pytest.mark.parametrize("t", SORTS)
def test_general_sort_prefixes(host, t):
    d, want = Z[f"sort_{t}_d"], Z[f"sort_{t}_order"].astype(np.int32)
    n = len(d)
    for k in sorted({0, 1, 5, 31, 32, 33, 100, 500, n // 3, n - 1, n}):
        if k > n or (k > 600 and n > 6000):
            continue
        got, _ = _ref_prefix(d, k)
        assert got[:k].tobytes() == want[:k].tobytes(), k
        got_h, _ = _host_prefix(host, d, k)
        assert got_h[:k].tobytes() == want[:k].tobytes(), k
    for k in (1000, n // 2, n - 3):  # the host build alone on the long prefixes of the big cases
        if 0 <= k <= n:
            got_h, _ = _host_prefix(host, d, k)
            assert got_h[:k].tobytes() == want[:k].tobytes(), k


def test_general_sort_agrees_with_head_below_33():
    rng = np.random.default_rng(5)
    for n in (50, 300, 3000):
        d = rng.integers(0, 20, n).astype(np.float32)
        for k in (1, 5, 32):
            dl, il = [np.float32(x) for x in d], list(range(n))
            logos_ref.msvc_sort_head(dl, il, k)
            got, _ = _ref_prefix(d, k)
            assert got[:k].tolist() == il[:k]


def test_host_sort_heap_fallback_and_dmatch_shapes(host):
    """Integer Hamming distances and sqrtf of integers with many repeats, up to 20k records: restatement == header."""
    rng = np.random.default_rng(11)
    cases = [rng.integers(0, 257, 20000).astype(np.float32), np.sqrt(rng.integers(0, 60, 12000).astype(np.float32)),
             np.zeros(5000, np.float32), np.arange(4000, 0, -1).astype(np.float32),
             np.tile(np.arange(7, dtype=np.float32), 900)]  # organ-pipe-like inputs drive ranges to the heap sort
    for d in cases:
        for k in (500, len(d)):
            got, dd = _ref_prefix(d, k)
            got_h, dd_h = _host_prefix(host, d, k)
            assert got[:k].tobytes() == got_h[:k].tobytes()
            assert np.all(np.diff(dd_h[:k]) >= 0)


def _encode_1d(vals):
    """1-D points as 128-float rows (value in dimension 0): L2 distance = |a - b|."""
    rows = np.zeros((len(vals), 128), np.float32)
    rows[:, 0] = vals
    return rows


def test_one_sided_cross_check_example():
    """A = {0, 3}, B = {2, -5}: b0 prefers a1 (1), b1 prefers a0 (5); a0's own nearest is b0, so a0 is not mutual -- OpenCV keeps
    (a0, b1, 5) and (a1, b0, 1) all the same."""
    A, B = _encode_1d([0.0, 3.0]), _encode_1d([2.0, -5.0])
    q, t, d = bf_select_ref.candidates(A, B, hamming=False, cross=True)
    assert q.tolist() == [0, 1] and t.tolist() == [1, 0] and d.tolist() == [5.0, 1.0]
    out, n_cand, n_ratio, dm = bf_select_ref.bf_match_select(A, B, False, True, 1e30, 500)
    assert n_cand == 2 and n_ratio == 2 and dm == 1.0
    assert [(int(r["queryIdx"]), int(r["trainIdx"]), float(r["distance"])) for r in out] == [(1, 0, 1.0), (0, 1, 5.0)]
    # a mutual-nearest test would drop (a0, b1)
    fwd = bf_select_ref.gms_oracle.bf_match(A, B, False)
    assert int(fwd["trainIdx"][0]) == 0


def test_cross_check_keeps_lowest_train_row_on_ties():
    q, t, d = bf_select_ref.cross_check(np.array([1, 1, 0, 1]), np.array([3, 2, 7, 2], np.float32), 3)
    assert q.tolist() == [0, 1] and t.tolist() == [2, 1] and d.tolist() == [7.0, 2.0]


def test_prune_boundaries():
    f32 = np.float32
    coef = 4.0
    at = f32(2.5) * f32(coef)  # exactly coef * d_min
    above = np.nextafter(at, f32(np.inf))
    d = np.array([2.5, at, above, 3.0], np.float32)
    k, n_ratio, dm = bf_select_ref.prune_count(d, coef, 500)
    assert (k, n_ratio, dm) == (3, 3, f32(2.5))  # d == coef * d_min is kept, the next float above it is not
    assert bf_select_ref.prune_count(np.array([0, 0, 1], np.float32), coef, 500)[:2] == (2, 2)  # d_min == 0 keeps the zeros only
    d = np.array([1, 1, 1, 1, 2], np.float32)
    assert bf_select_ref.prune_count(d, coef, 0)[0] == 0
    assert bf_select_ref.prune_count(d, coef, 1)[0] == 1
    assert bf_select_ref.prune_count(d, coef, 3)[0] == 3  # ties straddling max_size: the sort decides which of them stay
    assert bf_select_ref.prune_count(d, coef, 100)[0] == 5
    assert bf_select_ref.prune_count(d, 1.0, 100)[0] == 4
    # the product is taken in double: 0.1f * 3.0 in double lies below float(0.1f * 3.0f), so that float is dropped
    dmin = f32(0.1)
    pf = f32(dmin * f32(3.0))
    assert float(dmin) * 3.0 < float(pf)
    assert bf_select_ref.prune_count(np.array([dmin, pf], np.float32), 3.0, 10)[0] == 1


def test_ties_straddling_max_size_follow_the_sort():
    d = np.array([4, 2, 2, 3, 2, 2, 1, 2] * 10, np.float32)
    q = np.arange(len(d))
    out, n_ratio, _ = bf_select_ref.select(q, q, d, 1e30, 7)
    order, _ = _ref_prefix(d, len(d))
    assert out["queryIdx"].tolist() == order[:7].tolist()
    assert n_ratio == len(d)
