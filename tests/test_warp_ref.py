"""CPU: resize / warpAffine / getRotationMatrix2D as tests/warp_ref.py states them against the host build of the
header the kernels compile (sfm-gms_amd/csrc/warp_core.h through tests/cpp/warp_host.cpp), byte for byte, and the properties that do
not depend on the statement."""
import ctypes as C

import numpy as np
import pytest

import warp_ref
import hostbuild as hb

SRC = "warp_host.cpp"
ll = C.c_longlong


@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(SRC)
    lib = C.CDLL(so)
    lib.warp_host_resize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ll, C.c_void_p, C.c_int, C.c_int, ll]
    lib.warp_host_warp_affine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ll, C.c_void_p, C.c_void_p, C.c_int, C.c_int, ll]
    lib.warp_host_rotation_matrix.argtypes = [C.c_double] * 4 + [C.c_void_p]
    lib.warp_host_args_ok.argtypes = [C.c_int] * 4 + [ll, C.c_int, C.c_int, ll]
    return lib


def _noise(seed, h, w, c=None):
    return np.random.default_rng(seed).integers(0, 256, (h, w) if c is None else (h, w, c), dtype=np.uint8)


def _chan(im):
    return 1 if im.ndim == 2 else im.shape[2]


def _host_resize(host, im, dsize):
    im = np.ascontiguousarray(im)
    c = _chan(im)
    out = np.zeros((dsize[1], dsize[0]) + im.shape[2:], np.uint8)
    host.warp_host_resize(im.ctypes.data, im.shape[1], im.shape[0], c, im.shape[1] * c, out.ctypes.data, dsize[0], dsize[1], dsize[0] * c)
    return out


def _host_warp(host, im, M, dsize):
    im = np.ascontiguousarray(im)
    c = _chan(im)
    M = np.ascontiguousarray(M, dtype=np.float64).reshape(6)
    out = np.full((dsize[1], dsize[0]) + im.shape[2:], 77, np.uint8)
    host.warp_host_warp_affine(im.ctypes.data, im.shape[1], im.shape[0], c, im.shape[1] * c, M.ctypes.data, out.ctypes.data, dsize[0],
                               dsize[1], dsize[0] * c)
    return out


IMAGES = {"1x1": (1, 1, None), "2x5": (5, 2, None), "37x23x3": (23, 37, 3), "64x64": (64, 64, None)}   # name: (h, w, c)
MATRICES = [warp_ref.getRotationMatrix2D((10, 7), 30, 1.0), warp_ref.getRotationMatrix2D((3.3, 40.1), -75, 0.6),
            np.array([[1, 0, -40.25], [0, 1, 300.0]]), np.array([[1., 0, 0], [0, 1, 0]]), np.array([[1., 2, 3], [2, 4, 5]])]


@pytest.mark.parametrize("name", list(IMAGES))
def test_host_build_equals_the_statement_on_small_images(host, name):
    h, w, c = IMAGES[name]
    im = _noise(10 + list(IMAGES).index(name), h, w, c)
    for dsize in [(w, h), (1, 1), (2 * w + 3, 3 * h + 1), (max(w // 2, 1), max(h // 2, 1)), (max(w // 3, 1), h + 2), (w // 2 or 1, h)]:
        assert np.array_equal(_host_resize(host, im, dsize), warp_ref.resize(im, dsize)), dsize
    for M in MATRICES:
        for dsize in [(w, h), (w + 9, h + 4)]:
            assert np.array_equal(_host_warp(host, im, M, dsize), warp_ref.warpAffine(im, M, dsize)), (M, dsize)
    for angle in (0, 30, 90, 180, 270.5):
        M = warp_ref.getRotationMatrix2D((w / 2., h / 2.), angle, 1.0)
        assert np.array_equal(_host_warp(host, im, M, (w, h)), warp_ref.img_rotate(im, angle))


@pytest.mark.parametrize("dsize", [(300, 200), (901, 751)])
def test_host_build_equals_the_statement_450x375(host, dsize):
    im = _noise(5, 375, 450, 3)
    assert np.array_equal(_host_resize(host, im, dsize), warp_ref.resize(im, dsize))
    grey = np.ascontiguousarray(im[:, :, 1])
    assert np.array_equal(_host_resize(host, grey, dsize), warp_ref.resize(grey, dsize))


def test_rotation_matrix_host_equals_the_statement(host):
    for cx, cy, angle, scale in [(960, 540, 180, 1.0), (0.1, 1 / 3, 30, 0.6), (225.0, 187.5, -75, 2.5), (18.5, 11.5, 90, 1.0)]:
        M = np.zeros(6)
        host.warp_host_rotation_matrix(cx, cy, angle, scale, M.ctypes.data)
        assert M.tobytes() == warp_ref.getRotationMatrix2D((cx, cy), angle, scale).tobytes()
    # the centre is rounded to float32 first
    M = warp_ref.getRotationMatrix2D((0.1, 0.0), 90, 1.0)
    assert M[0, 2] == (1 - M[0, 0]) * float(np.float32(0.1)) and M[0, 2] != (1 - M[0, 0]) * 0.1


@pytest.mark.parametrize("shape", [(1080, 1920), (375, 450, 3), (23, 37, 3), (5, 2)])
def test_resize_to_the_same_size_is_the_identity(shape):
    im = _noise(1, *shape)
    assert np.array_equal(warp_ref.resize(im, (im.shape[1], im.shape[0])), im)


def test_exact_halving_is_the_2x2_mean_and_halving_x_alone_is_not(host):
    im = _noise(2, 46, 74, 3)
    a = im.astype(np.int64)
    mean = ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    assert np.array_equal(warp_ref.resize(im, (37, 23)), mean)
    assert np.array_equal(_host_resize(host, im, (37, 23)), mean)
    # x alone: the linear taps (sx = 2 dx, fx = 0.5, rows untouched) give (a + b + 1) >> 1 by way of the 11-bit weights, not the mean
    # of four; written out from the formula for a0 = a1 = 1024, b0 = 2048, b1 = 0
    H = a[:, 0::2] * 1024 + a[:, 1::2] * 1024
    want = ((((2048 * (H >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
    got = warp_ref.resize(im, (37, 46))
    assert np.array_equal(got, want) and np.array_equal(_host_resize(host, im, (37, 46)), want)
    assert not np.array_equal(got[0::2], mean)


@pytest.mark.parametrize("shape", [(1080, 1920), (375, 450, 3), (23, 37, 3), (5, 2)])
def test_rotation_by_180_is_the_flip_shifted_by_one_pixel(shape):
    im = _noise(3, *shape)
    got = warp_ref.img_rotate(im, 180)
    assert np.array_equal(got[1:, 1:], im[::-1, ::-1][:-1, :-1])
    assert not got[0].any() and not got[:, 0].any()


def test_rotation_by_90_of_a_square(host):
    im = _noise(4, 64, 64)
    got = warp_ref.img_rotate(im, 90)
    assert np.array_equal(got[1:, :], np.rot90(im)[:-1, :])
    M = warp_ref.getRotationMatrix2D((32., 32.), 90, 1.0)
    assert np.array_equal(_host_warp(host, im, M, (64, 64)), got)


def test_identity_and_singular_matrices(host):
    im = _noise(6, 23, 37, 3)
    eye = np.array([[1., 0, 0], [0, 1, 0]])
    assert np.array_equal(warp_ref.warpAffine(im, eye, (37, 23)), im)
    assert np.array_equal(_host_warp(host, im, eye, (37, 23)), im)
    sing = np.array([[1., 2, 3], [2, 4, 5]])
    for got in (warp_ref.warpAffine(im, sing, (11, 9)), _host_warp(host, im, sing, (11, 9))):
        assert np.array_equal(got, np.broadcast_to(im[0, 0], (9, 11, 3)))


def test_a_ramp_resized():
    ramp = np.array([[0, 60, 120, 180]], np.uint8)
    assert warp_ref.resize(ramp, (7, 1))[0].tolist() == [0, 21, 56, 90, 124, 159, 180]
    assert warp_ref.resize(ramp, (3, 1))[0].tolist() == [10, 90, 170]


def test_weights_sum_to_one_so_a_constant_image_stays_constant():
    c = np.full((9, 7, 3), 200, np.uint8)
    for dsize in [(5, 4), (31, 40), (7, 4)]:
        assert np.unique(warp_ref.resize(c, dsize)).tolist() == [200]


def test_accepted_arguments(host):
    ok = lambda *a: host.warp_host_args_ok(*a)   # (n, sw, sh, channels, src_pitch, dw, dh, dst_pitch)
    assert ok(1, 1, 1, 1, 1, 8192, 8192, 8192) and ok(65535, 8192, 8192, 3, 3 * 8192, 1, 1, 3)
    assert not ok(0, 4, 4, 1, 4, 4, 4, 4) and not ok(65536, 4, 4, 1, 4, 4, 4, 4)
    assert not ok(1, 4, 4, 2, 8, 4, 4, 8) and not ok(1, 4, 4, 4, 16, 4, 4, 16)
    assert not ok(1, 0, 4, 1, 4, 4, 4, 4) and not ok(1, 4, 8193, 1, 4, 4, 4, 4)
    assert not ok(1, 4, 4, 1, 4, 0, 4, 4) and not ok(1, 4, 4, 1, 4, 4, 8193, 4)
    assert not ok(1, 4, 4, 3, 11, 4, 4, 12) and not ok(1, 4, 4, 3, 12, 4, 4, 11)


def test_stand_alone_program_under_sanitizers():
    exe = hb.host_exe_sanitized(SRC, defines=("WARP_HOST_MAIN",))
    out = hb.run(exe)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("warp_host: checksum ")


def test_warp_shim_compiles_and_links():
    res = hb.run(hb.shim_exe("warp_shim_main.cpp"))
    assert res.returncode == 2 and "usage" in res.stderr
