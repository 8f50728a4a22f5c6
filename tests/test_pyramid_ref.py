"""CPU: the numpy statement of the pyramid keypoint source (tests/pyramid_ref.py) -- level sizes, resize, quotas,
n_levels = 1 against the single-scale statement -- and what the pyramid is for: on committed pixels, a photograph against a shrunk
copy of itself, exact Hamming nearest neighbours find at least twice as many correct matches with the pyramid's keypoints as with
the single-scale detector's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_level_sizes_and_the_stop_rule():
    s = pyramid_ref.level_sizes(1920, 1080, 8)
    assert s == [(1920, 1080), (1600, 900), (1333, 750), (1111, 625), (926, 521), (772, 434), (643, 362), (536, 302)]
    assert pyramid_ref.level_sizes(1920, 1080, 1) == [(1920, 1080)]
    assert pyramid_ref.level_sizes(33, 33, 8) == [(33, 33)]                    # (5 * 33 + 3) // 6 = 28: refused by the detector
    assert pyramid_ref.level_sizes(32, 500, 8) == []                           # level 0 itself is refused
    assert pyramid_ref.level_sizes(1030, 50, 16) == [(1030, 50), (858, 42), (715, 35)]
    for w, h in ((97, 65), (641, 479), (450, 375), (65535, 65535)):
        s = pyramid_ref.level_sizes(w, h, 16)
        assert s[0] == (w, h) and all(a[0] > b[0] and a[1] > b[1] for a, b in zip(s, s[1:]))          # strictly smaller
        assert all(b[0] > 32 and b[1] > 32 for b in s)
        assert all(6 * b[0] <= 5 * a[0] + 3 and 5 * a[0] <= 6 * b[0] + 2 for a, b in zip(s, s[1:]))   # the ratio stays at 1.2
        nxt = ((5 * s[-1][0] + 3) // 6, (5 * s[-1][1] + 3) // 6)
        assert len(s) == 16 or nxt[0] <= 32 or nxt[1] <= 32
    for bad in (0, 17):
        with pytest.raises(ValueError):
            pyramid_ref.level_sizes(100, 100, bad)


def test_quotas():
    sizes = pyramid_ref.level_sizes(1920, 1080, 8)
    for m in (10000, 4000, 37, 8, 5, 1, 0):
        q = pyramid_ref.quotas(sizes, m)
        assert sum(q) == m and all(v >= 0 for v in q)
        assert all(a >= b for a, b in zip(q, q[1:]))                           # larger levels get at least as much
        total = sum(w * h for w, h in sizes)
        assert all(q[l] == m * sizes[l][0] * sizes[l][1] // total for l in range(1, 8))
    assert pyramid_ref.quotas(sizes, 5) == [4, 1, 0, 0, 0, 0, 0, 0]            # fewer keypoints than levels
    assert pyramid_ref.quotas(sizes[:1], 123) == [123]
    big = pyramid_ref.level_sizes(65535, 65535, 16)
    assert sum(pyramid_ref.quotas(big, 2 ** 31 - 1)) == 2 ** 31 - 1


def test_resize_properties():
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (75, 131), dtype=np.uint8)
    assert np.array_equal(pyramid_ref.resize(noise, 131, 75), noise)          # equal sizes: the identity
    for v in (0, 1, 127, 255):
        assert (pyramid_ref.resize(np.full((60, 85), v, np.uint8), 71, 50) == v).all()      # a constant image stays constant
    ramp = np.broadcast_to(np.minimum(np.arange(200) * 3 // 2, 255).astype(np.uint8), (40, 200))
    out = pyramid_ref.resize(ramp, 167, 34)
    assert (np.diff(out.astype(int), axis=1) >= 0).all() and (out == out[0]).all() and out[0, 0] <= 2 and out[0, -1] == 255
    blocks = rng.integers(0, 256, (30, 41), dtype=np.uint8)
    assert np.array_equal(pyramid_ref.resize(np.kron(blocks, np.ones((2, 2), np.uint8)), 41, 30), blocks)   # 2 : 1 on 2 x 2 blocks
    # a hand-computed pixel: 6 -> 5 columns, output 1 reads source 1.3 -> fixed 332 = (1, weight 76)
    row = np.array([[0, 100, 200, 50, 10, 250]] * 6, np.uint8)
    assert pyramid_ref.resize(row, 5, 5)[0, 1] == (180 * 100 + 76 * 200 + 128) >> 8
    with pytest.raises(ValueError):
        pyramid_ref.resize(noise, 132, 75)


def test_one_level_is_the_single_scale_detector(oracle):
    z = np.load(os.path.join(GOLDEN, "image_stereo_pair_450x375.npz"))
    for threshold, max_kp in ((20, 10000), (8, 700), (20, 1)):
        kp, rows, counts = pyramid_ref.detect(oracle, z["left"], threshold, max_kp, 1)
        want_kp, want_rows = oracle.detect(z["left"], threshold, max_kp)
        assert kp.tobytes() == want_kp.tobytes() and rows.tobytes() == want_rows.tobytes() and counts.tolist() == [len(want_kp)]


def test_records_of_the_levels(oracle):
    img = np.load(os.path.join(GOLDEN, "image_stereo_pair_450x375.npz"))["left"]
    kp, rows, counts = pyramid_ref.detect(oracle, img, 12, 3000, 8)
    sizes = pyramid_ref.level_sizes(450, 375, 8)
    q = pyramid_ref.quotas(sizes, 3000)
    assert len(kp) == len(rows) == counts.sum() and (counts <= q).all() and (counts[:6] > 0).all()
    assert (np.diff(kp["octave"]) >= 0).all() and np.array_equal(np.bincount(kp["octave"], minlength=8), counts)
    lvl0 = kp[kp["octave"] == 0]
    want, want_rows = oracle.detect(img, 12, q[0])
    assert lvl0.tobytes() == want.tobytes() and rows[: len(want)].tobytes() == want_rows.tobytes()
    for l in range(1, 8):
        k = kp[kp["octave"] == l]
        f = np.float32(450) / np.float32(sizes[l][0])
        assert (k["size"] == np.float32(31) * f).all() and (k["class_id"] == -1).all()
        # centres aligned: a level pixel's centre maps into the image, at least 16 level pixels from every edge
        assert (k["x"] >= 16 * f - 1).all() and (k["x"] <= 450 - 16 * f).all() and (k["y"] >= 0).all() and (k["y"] <= 375).all()


def _hamming_nn(a, b):
    """Index of the exact Hamming nearest row of b for every row of a (lowest index on ties)."""
    bits = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint16)
    best = np.zeros(len(a), dtype=np.int64)
    for i0 in range(0, len(a), 256):
        d = bits[a[i0:i0 + 256, None, :] ^ b[None, :, :]].sum(axis=2)
        best[i0:i0 + 256] = d.argmin(axis=1)
    return best


def _correct(kp_l, rows_l, kp_r, rows_r, sx, sy):
    """Left keypoints whose nearest right row sits within 3 pixels of where the shrink puts them (centres aligned)."""
    nn = _hamming_nn(rows_l, rows_r)
    ex, ey = (kp_l["x"] + 0.5) * sx - 0.5, (kp_l["y"] + 0.5) * sy - 0.5
    return int((np.hypot(kp_r["x"][nn] - ex, kp_r["y"][nn] - ey) <= 3.0).sum())


@pytest.mark.parametrize("wr,hr", [(1152, 648), (1000, 1000)], ids=["0.6x", "1000x1000"])
def test_scale_robustness_on_committed_pixels(oracle, wr, hr):
    """The 1080p left photograph against a shrunk copy of itself (0.6 x; main.cpp:44's 1000 x 1000), threshold 20, 4000 keypoints,
    exact Hamming nearest neighbour. The pyramid (8 levels) must give at least twice the single-scale detector's correct matches.
    Measured with this definition: 0.6 x: single scale 47 correct of 245 left keypoints, pyramid 860 of 1350; 1000 x 1000: 83 of 245
    against 622 of 1350."""
    left = np.load(os.path.join(GOLDEN, "image_main_scenario_1080p.npz"))["left"]
    h, w = left.shape
    right = pyramid_ref.resize(left, wr, hr)
    sx, sy = wr / w, hr / h
    single = [oracle.detect(im, 20, 4000) for im in (left, right)]
    pyr = [pyramid_ref.detect(oracle, im, 20, 4000, 8)[:2] for im in (left, right)]
    n_single = _correct(single[0][0], single[0][1], single[1][0], single[1][1], sx, sy)
    n_pyr = _correct(pyr[0][0], pyr[0][1], pyr[1][0], pyr[1][1], sx, sy)
    print(f"\n{wr}x{hr}: single scale {len(single[0][0])}/{len(single[1][0])} keypoints, {n_single} correct; "
          f"pyramid {len(pyr[0][0])}/{len(pyr[1][0])} keypoints, {n_pyr} correct")
    assert n_single > 0 and n_pyr >= 2 * n_single
