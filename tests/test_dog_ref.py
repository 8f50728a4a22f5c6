"""CPU: the DoG detector's numpy statement (tests/dog_ref.py) against the host build of the kernel's header
(sfm-gms_amd/csrc/dog_core.h through tests/cpp/dog_host.cpp), on every pixel, and the properties the definition implies
(DESIGN.md §4.7d)."""
import ctypes as C

import numpy as np
import pytest

import dog_ref
import pyramid_ref
import hostbuild as hb

SRC = "dog_host.cpp"


@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(SRC)
    lib = C.CDLL(so)
    lib.dog_host_table.argtypes = [C.c_int, C.c_void_p]
    lib.dog_host_blur.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.dog_host_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def small_images(w, h):
    """The five images of the GPU test's batches (tests/test_gpu_dog.py uses this function): uniform noise, 4 x 4 blocks of 60 / 150 and
    of 20 / 220, 60 sparse dots, flat."""
    rng = np.random.default_rng(w * 1000 + h)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cells = np.kron(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), dtype=np.int64))[:h, :w]
    sparse = np.full((h, w), 40, dtype=np.uint8)
    sparse[rng.integers(0, h, 60), rng.integers(0, w, 60)] = 200
    return np.stack([noise, (cells * 90 + 60).astype(np.uint8), (cells * 200 + 20).astype(np.uint8), sparse, np.full((h, w), 77, dtype=np.uint8)])


def _host_candidates(host, img, contrast):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    out = np.full(img.shape, 9, dtype=np.uint8)
    n = host.dog_host_candidates(img.ctypes.data, img.shape[1], img.shape[0], contrast, out.ctypes.data)
    assert n == np.count_nonzero(out)
    return out


def blob(size, sigma, sign=1, cx=None, cy=None):
    """A Gaussian blob of 100 grey levels on 110 (bright) or under 110 (dark), centred on a pixel."""
    cx, cy = size // 2 if cx is None else cx, size // 2 if cy is None else cy
    y, x = np.mgrid[0:size, 0:size]
    return np.rint(110 + sign * 100 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))).astype(np.uint8)


def test_tables_equal_the_rule_and_sum_to_4096(host):
    for j in range(4):
        r = host.dog_host_radius(j)
        assert r == 4 + j == int(np.ceil(3 * dog_ref.SIGMAS[j])) and len(dog_ref.TABLES[j]) == 2 * r + 1
        got = np.zeros(2 * r + 1, dtype=np.int32)
        host.dog_host_table(j, got.ctypes.data)
        assert got.tolist() == dog_ref.TABLES[j] == dog_ref.table_rule(j)
        assert sum(dog_ref.TABLES[j]) == 4096 and dog_ref.TABLES[j] == dog_ref.TABLES[j][::-1]
    assert [round(s, 3) for s in dog_ref.SIGMAS] == [1.217, 1.461, 1.753, 2.103]
    assert [host.dog_host_score(c) for c in (0, 15, -16, 31, 32, -4080, 4095, 65280, -65280)] == [1, 1, 1, 1, 2, 255, 255, 255, 255]


@pytest.mark.parametrize("w,h", [(33, 33), (97, 65), (64, 48), (130, 97)])
def test_host_build_equals_the_statement_on_every_pixel(host, w, h):
    imgs = small_images(w, h)
    for j in range(4):                                                  # the blur planes first: a wrong tap shows up here
        got = np.zeros((h, w), dtype=np.uint16)
        host.dog_host_blur(imgs[0].ctypes.data, w, h, j, got.ctypes.data)
        want = dog_ref.blur(imgs[0], j)
        assert want.max() <= 65280 and np.array_equal(got, want)
    counts = []
    for img in imgs:
        for contrast in (0, 128, 2000, 65535):
            want = dog_ref.candidates(img, contrast)
            assert np.array_equal(_host_candidates(host, img, contrast), want)
            counts.append(np.count_nonzero(want))
            assert not want[:16].any() and not want[-16:].any() and not want[:, :16].any() and not want[:, -16:].any()
    counts = np.array(counts).reshape(5, 4)
    assert (counts[:, 3] == 0).all() and (counts[4] == 0).all()         # contrast 65535; the flat image
    assert (np.diff(counts, axis=1) <= 0).all()                         # a higher contrast only removes candidates
    if (w, h) == (33, 33):
        assert counts.sum() == 0                                        # one legal pixel; the statement gives no candidate there
    else:
        assert (counts[:3, 0] > 0).all()
    if (w, h) == (130, 97):
        assert (dog_ref.candidates(imgs[2], 128) == 255).sum() > 0      # the 20 / 220 blocks saturate the score


def test_sizes_the_detector_refuses(host):
    img = np.zeros((65, 32), dtype=np.uint8)
    out = np.zeros_like(img)
    assert host.dog_host_candidates(img.ctypes.data, 32, 65, 0, out.ctypes.data) == -1
    assert host.dog_host_candidates(img.ctypes.data, 65, 32, 0, out.ctypes.data) == -1
    big = np.zeros((40, 40), dtype=np.uint8)
    for contrast in (-1, 65536):
        assert host.dog_host_candidates(big.ctypes.data, 40, 40, contrast, big.ctypes.data) == -1
        with pytest.raises(ValueError):
            dog_ref.candidates(big, contrast)
    assert not dog_ref.candidates(img, 0).any()


def test_adding_a_constant_changes_nothing(host):
    """The taps sum to 4096, so a constant k adds exactly 256 k to every H and every B (k * 4096 * 16 >> 4 and k * 256 * 4096 >> 12 are
    exact) and nothing to a layer."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 200, (100, 130), dtype=np.uint8)
    base = dog_ref.candidates(img, 64)
    assert base.any()
    for k in (1, 17, 55):
        shifted = img + np.uint8(k)
        assert shifted.max() <= 255 and shifted.min() >= k
        assert np.array_equal(dog_ref.blur(shifted, 3)[7:-7, 7:-7], dog_ref.blur(img, 3)[7:-7, 7:-7] + 256 * k)
        assert np.array_equal(dog_ref.candidates(shifted, 64), base)
        assert np.array_equal(_host_candidates(host, shifted, 64), base)


def _lowest_level_with(img, cx, cy):
    """(lowest pyramid level on which a candidate maps to within 2 level-0 pixels of (cx, cy), the levels that report one)."""
    h, w = img.shape
    found = []
    for l, level in enumerate(pyramid_ref.build(img, 16)):
        ys, xs = np.nonzero(dog_ref.candidates(level, 128))
        fx, fy = w / level.shape[1], h / level.shape[0]
        px, py = (xs + 0.5) * fx - 0.5, (ys + 0.5) * fy - 0.5
        if len(xs) and (np.hypot(px - cx, py - cy) <= 2.0).any():
            found.append(l)
    return (found[0] if found else None), found


@pytest.mark.parametrize("sign", [1, -1])
def test_gaussian_blobs_are_found_at_a_level_that_grows_with_them(sign):
    """100 grey levels on 110, bright and dark, on 240 x 240: found within 2 level-0 pixels of the centre, and the lowest level that
    reports the blob does not decrease as its standard deviation grows."""
    lowest = []
    for sigma in (1.5, 2, 3, 4, 5, 6.5):
        first, found = _lowest_level_with(blob(240, sigma, sign), 120, 120)
        assert first is not None, sigma
        lowest.append(first)
    print(f"\nsign {sign}: lowest levels {lowest}")
    assert lowest == sorted(lowest) and lowest[0] == 0 and lowest[-1] > lowest[0]


def test_flat_and_tied_images_have_no_candidate(host):
    flat = np.full((50, 60), 123, dtype=np.uint8)
    assert not dog_ref.candidates(flat, 0).any() and not _host_candidates(host, flat, 0).any()
    stripes = np.tile((np.arange(60) // 6 % 2 * 100 + 50).astype(np.uint8), (50, 1))     # every column's neighbours above and below tie
    assert not dog_ref.candidates(stripes, 0).any() and not _host_candidates(host, stripes, 0).any()


def test_select_takes_the_strongest_in_raster_order():
    cand = np.zeros((6, 7), dtype=np.uint8)
    cand[1, 2], cand[1, 5], cand[3, 0], cand[4, 4], cand[5, 1] = 9, 4, 4, 4, 30
    xs, ys, sc = dog_ref.select(cand, 3)
    assert list(zip(xs, ys, sc)) == [(2, 1, 9), (5, 1, 4), (1, 5, 30)] and dog_ref.cut_has_tie(cand, 3)
    xs, ys, sc = dog_ref.select(cand, 10)
    assert len(xs) == 5 and not dog_ref.cut_has_tie(cand, 10) and not dog_ref.cut_has_tie(cand, 2)
    assert len(dog_ref.select(cand, 0)[0]) == 0


def test_sanitizer_run_of_the_stand_alone_program():
    exe = hb.host_exe_sanitized(SRC, defines=("DOG_HOST_MAIN",))
    out = hb.run(exe)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("dog_host: tiny ")
