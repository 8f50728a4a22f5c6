"""CPU: the gradient descriptor's numpy statement (tests/grad_desc_ref.py) against the host build of the kernel's header
(sfm-gms_amd/csrc/grad_desc_core.h through tests/cpp/grad_desc_host.cpp), byte for byte, and the properties the definition implies
(DESIGN.md §4.7c)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import grad_desc_ref as gd
import pyramid_ref
import hostbuild as hb

STEREO = os.path.join(hb.ROOT, "tests", "golden", "image_stereo_pair_450x375.npz")
SRC = "grad_desc_host.cpp"


@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(SRC)
    lib = C.CDLL(so)
    lib.gd_host_window_table.argtypes = [C.c_void_p]
    lib.gd_host_dir_table.argtypes = [C.c_void_p, C.c_void_p]
    lib.gd_host_box.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.gd_host_direction.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.gd_host_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def _host_rows(host, S, xs, ys, bins, fill=None):
    S = np.ascontiguousarray(S, dtype=np.uint16)
    xyb = np.ascontiguousarray(np.stack([xs, ys, bins], axis=1), dtype=np.int32)
    out = np.zeros((len(xyb), 128), dtype=np.float32) if fill is None else np.full((len(xyb), 128), fill, dtype=np.float32)
    refused = host.gd_host_rows(S.ctypes.data, S.shape[1], S.shape[0], xyb.ctypes.data, len(xyb), out.ctypes.data)
    return refused, out


def _check_invariants(rows, n2):
    """float32 integers 0..255; with r = isqrt(sum of squares): a row is all zero exactly when n' = 0; otherwise each value is within
    1/2 of 512 v / n' unless cut at 255, and n'^2 <= sum v^2 < (n' + 1)^2, so by the triangle inequality over 128 values
    r <= 512 (n' + 1) / n' + sqrt(128) / 2 < 512 + 512 / n' + 6, and r >= 512 - 6 = 506 when no value was cut, r >= 255 when one was."""
    assert rows.dtype == np.float32 and rows.shape[1] == 128
    assert (rows == np.rint(rows)).all() and rows.min() >= 0 and rows.max() <= 255
    q = rows.astype(np.int64)
    for row, n in zip(q, n2):
        r = math.isqrt(int((row * row).sum()))
        if n == 0:
            assert r == 0
            continue
        assert r <= 512 + 512 // int(n) + 6, (r, n)
        assert r >= (506 if row.max() < 255 else 255), (r, n)


def _compare(host, img, xs, ys, bins):
    S = gd.box_sum(img)
    want, acc, n2 = gd.rows_parts(S, xs, ys, bins)
    refused, got = _host_rows(host, S, xs, ys, bins)
    assert refused == 0 and got.tobytes() == want.tobytes()
    assert acc.min() >= 0 and acc.max() <= gd.max_cell_weight() * host.gd_host_max_part()
    _check_invariants(want, n2)
    return want, acc


def _all_positions(img):
    h, w = img.shape
    ys, xs = np.mgrid[gd.BORDER:h - gd.BORDER, gd.BORDER:w - gd.BORDER]
    return xs.ravel(), ys.ravel()


def test_tables_and_constants(host):
    win = np.zeros(170, dtype=np.int32)
    host.gd_host_window_table(win.ctypes.data)
    assert win.tolist() == gd.WIN.tolist()
    assert win.tolist() == [round(256 * math.exp(-r2 / 288.0)) for r2 in range(170)]       # what the numbers are
    c, s = np.zeros(32, dtype=np.int32), np.zeros(32, dtype=np.int32)
    host.gd_host_dir_table(c.ctypes.data, s.ctypes.data)
    assert c.tolist() == gd.DIR_C.tolist() and s.tolist() == gd.DIR_S.tolist()
    assert gd.max_cell_weight() <= host.gd_host_max_cell_weight()                           # the header's overflow bound
    assert host.gd_host_max_cell_weight() * host.gd_host_max_part() < 1 << 27
    assert host.gd_host_max_part() == ((25 * 255 * 5793 >> 12) * 5793) >> 12


def test_box_and_direction_are_the_detectors(host, oracle):
    """The statement's and the host build's box sum and direction equal the detector's CPU statement (oracle/detect_ref.c)."""
    img = np.random.default_rng(3).integers(0, 256, (65, 97), dtype=np.uint8)
    S = gd.box_sum(img)
    got = np.zeros_like(S)
    host.gd_host_box(img.ctypes.data, 97, 65, got.ctypes.data)
    assert np.array_equal(got, S) and np.array_equal(oracle.detect_maps(img)[1], S)
    xs, ys = _all_positions(img)
    kp = np.zeros(len(xs), dtype=oracle.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = xs, ys
    rc, want_kp, _ = oracle.describe(img, kp)
    bins = gd.direction(img, xs, ys)
    assert rc == len(kp) and np.array_equal(want_kp["angle"], np.float32(11.25) * bins.astype(np.float32))
    assert [host.gd_host_direction(img.ctypes.data, 97, int(x), int(y)) for x, y in zip(xs, ys)] == bins.tolist()


def test_stereo_fixture_all_levels(host, oracle):
    left = np.load(STEREO)["left"]
    levels = pyramid_ref.build(left, 8)
    sizes = [(l.shape[1], l.shape[0]) for l in levels]
    assert len(levels) == 8
    total = 0
    for level, q in zip(levels, pyramid_ref.quotas(sizes, 700)):
        kp = oracle.detect(level, 8, q)[0]
        assert len(kp) > 0
        bins = np.rint(kp["angle"] / np.float32(11.25)).astype(np.int64)
        _compare(host, level, kp["x"].astype(np.int64), kp["y"].astype(np.int64), bins)
        total += len(kp)
    assert total > 300
    # the statement's pyramid form is those rows behind one another
    kp, _, counts, rows = gd.detect(oracle, left, 8, 700, 8)
    assert len(rows) == len(kp) == counts.sum() == total and rows.any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_noise_33x33_has_one_legal_position(host, seed):
    img = np.random.default_rng(seed).integers(0, 256, (33, 33), dtype=np.uint8)
    xs, ys = _all_positions(img)
    assert xs.tolist() == [16] and ys.tolist() == [16]
    bins = np.arange(32)
    _compare(host, img, np.full(32, 16), np.full(32, 16), bins)
    S = gd.box_sum(img)
    for x, y in ((15, 16), (16, 15), (17, 16), (16, 17)):                                   # the host build refuses the neighbours
        refused, out = _host_rows(host, S, [x], [y], [0], fill=-1.0)
        assert refused == 1 and (out == -1.0).all()
        with pytest.raises(AssertionError):
            gd.rows(S, [x], [y], [0])


def test_noise_97x65(host):
    img = np.random.default_rng(97065).integers(0, 256, (65, 97), dtype=np.uint8)
    xs, ys = _all_positions(img)
    _compare(host, img, xs, ys, gd.direction(img, xs, ys))
    _compare(host, img, xs, ys, (xs * 7 + ys * 3) % 32)


def test_two_grey_levels_flat_patches_give_zero_rows(host):
    rng = np.random.default_rng(5)
    img = (np.kron(rng.integers(0, 2, (4, 5)), np.ones((40, 40), dtype=np.int64)) * 90 + 60).astype(np.uint8)
    img[:40, :40], img[:40, 40:80] = 60, 150                                                # one edge and flat blocks for certain
    ys, xs = (a.ravel() for a in np.mgrid[16:img.shape[0] - 16:4, 16:img.shape[1] - 16:4])
    rows, _ = _compare(host, img, xs, ys, (xs // 4 + ys // 4) % 32)
    flat = ~rows.any(axis=1)
    assert flat.any() and (~flat).any()
    at = {(int(x), int(y)): i for i, (x, y) in enumerate(zip(xs, ys))}
    assert flat[at[(20, 20)]] and not flat[at[(40, 20)]]


def test_saturated_steps_stay_inside_the_overflow_bound(host):
    """0 / 255 steps of several widths at all 32 directions: the largest gradients the box sum can give."""
    top = 0
    for period in (1, 2, 3, 5, 6, 12):
        yy, xx = np.mgrid[0:35, 0:35]
        for img in ((((xx // period + yy // period) & 1) * 255), ((xx // period) & 1) * 255, ((xx + yy) // period & 1) * 255):
            img = img.astype(np.uint8)
            for x, y in ((16, 16), (17, 18)):
                _, acc = _compare(host, img, np.full(32, x), np.full(32, y), np.arange(32))
                top = max(top, int(acc.max()))
    print(f"\nlargest accumulator {top} of a bound of {gd.max_cell_weight() * host.gd_host_max_part()}")
    assert top > 1 << 23                                                                     # well past what 24 bits would hold


def test_rot90_with_eight_bins_more_is_the_same_row():
    """np.rot90(img, -1) puts old (x, y) at (H - 1 - y, x), an offset (dx, dy) at (-dy, dx) and a gradient (gx, gy) at (-gy, gx); bin
    b + 8 has (c, s) -> (-s, c). So every sample's frame coordinates and frame gradient are the same integers, and so is the row."""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (70, 83), dtype=np.uint8)
    img[20:50, 30:60] = (rng.integers(0, 2, (30, 30)) * 255).astype(np.uint8)
    h, w = img.shape
    xs, ys = _all_positions(img)
    pick = rng.choice(len(xs), 64, replace=False)
    xs, ys = xs[pick], ys[pick]
    S, S_rot = gd.box_sum(img), gd.box_sum(np.rot90(img, -1))
    assert np.array_equal(S_rot, np.rot90(S, -1))
    for b in range(32):
        bins = np.full(len(xs), b)
        a = gd.rows(S, xs, ys, bins)
        r = gd.rows(S_rot, h - 1 - ys, xs, (bins + 8) % 32)
        assert a.tobytes() == r.tobytes(), b
    assert a.any()


def test_sanitizer_run_of_the_stand_alone_program():
    exe = hb.host_exe_sanitized(SRC, defines=("GRAD_DESC_MAIN",))
    out = hb.run(exe)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("grad_desc_host: noise ")
