"""CPU: what the constructed images of tests/value_limit_cases.py reach, from the CPU statements alone (oracle/detect_ref.c,
tests/pyramid_ref.py, grad_desc_ref.py, dog_ref.py, dog_refine_ref.py), so that equal bytes in tests/test_gpu_value_limits.py mean
something: FAST score 255 and a quota inside its tie, the gradient descriptor's extremes, the DoG contrast placed on a candidate's own
|D_1|, refinement terms beyond those of the noise and block images. The host builds of the kernels' headers equal the statements on
these inputs byte for byte. Every property is asserted and its number printed."""
import ctypes as C

import numpy as np
import pytest

import dog_ref
import dog_refine_ref
import gms_oracle
import grad_desc_ref as gd
import pyramid_ref
import value_limit_cases as vc
from test_dog_ref import small_images
import hostbuild as hb

SMALL_SIZES = [(33, 33), (97, 65), (64, 48), (130, 200), (641, 479), (1030, 50)]     # those of tests/test_dog_refine_ref.py


@pytest.fixture(scope="module")
def grad_host():
    lib = C.CDLL(hb.host_lib("grad_desc_host.cpp"))
    lib.gd_host_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def dog_host():
    lib = C.CDLL(hb.host_lib("dog_host.cpp"))
    lib.dog_host_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def refine_host():
    lib = C.CDLL(hb.host_lib("dog_refine_host.cpp"))
    lib.dog_refine_host_offsets.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _centres():
    return np.array([c[0] for c in vc.MOSAIC_CENTRES]), np.array([c[1] for c in vc.MOSAIC_CENTRES])


# ---- the images themselves ---------------------------------------------------------------------------------------------------------------
def test_mosaic_layout():
    m = vc.mosaic()
    assert m.shape == (264, 198) == (vc.MOSAIC_H, vc.MOSAIC_W) and m.dtype == np.uint8
    assert 198 % 64 != 0 and 264 % 16 != 0 and 198 > 3 * 64 and 264 > 16 * 16          # crosses the 64 x 16 tiles, no multiple of them
    assert vc.MOSAIC_CENTRES[0] == (16, 16) and vc.MOSAIC_CENTRES[-1] == (198 - 17, 264 - 17) == (181, 247)      # the legal region's corners
    p = vc.patches()
    for i, (x, y) in enumerate(vc.MOSAIC_CENTRES):                                       # a centre's 16-pixel reach is its own patch
        assert np.array_equal(m[y - 16:y + 17, x - 16:x + 17], p[i]), i
    assert (p[vc.FLAT] == 77).all() and sorted(set(p[vc.SMALLEST_STEP].ravel().tolist())) == [100, 101]
    assert p[vc.BRIGHT_PIXEL].sum() == 255 and p[vc.BRIGHT_PIXEL][16, 16] == 255 and (255 - p[vc.DARK_PIXEL]).sum() == 255
    assert all(set(p[i].ravel().tolist()) == {0, 255} for i in [*vc.HALF_PLANES, *vc.FAR_EDGES, *vc.CHECKERBOARDS])
    assert np.array_equal(vc.mosaic_batch()[1], m[::-1]) and np.array_equal(vc.mosaic_batch()[2], 255 - m)


def test_dots_and_discs_layout():
    for w, h in vc.DOTS_SIZES:
        d = vc.dots(w, h, 255, 0)
        ys, xs = np.nonzero(d)
        assert d.shape == (h, w) and xs.min() == ys.min() == 18 and xs.max() < w - 16 and ys.max() < h - 16
        assert np.array_equal(vc.dots(w, h, 0, 255), 255 - d) and vc.dots_batch(w, h).shape == (4, h, w)
    d = vc.discs()
    assert d.shape == (97, 130) and set(d.ravel().tolist()) == {0, 255}
    c = np.array(vc.DISC_CENTRES)
    assert len(c) == 8 and c[:, 0].min() >= 24 and c[:, 1].min() >= 24 and c[:, 0].max() <= 129 - 24 and c[:, 1].max() <= 96 - 24
    gaps = np.hypot(c[:, None, 0] - c[None, :, 0], c[:, None, 1] - c[None, :, 1])
    assert gaps[~np.eye(8, dtype=bool)].min() >= 24
    for i, (cx, cy) in enumerate(vc.DISC_CENTRES):                                       # bright on 0, dark on 255; the area is a disc's
        x, y, r = int(cx), int(cy), vc.DISC_RADII[i % 4]
        box = d[y - 12:y + 13, x - 12:x + 13]
        inside = int((box == (255 if i < 4 else 0)).sum())
        assert d[y, x] == (255 if i < 4 else 0) and d[y - 12, x - 12] == (0 if i < 4 else 255)
        assert np.pi * r * r <= inside <= np.pi * (r + 0.5) ** 2, (i, inside)


# ---- the gradient descriptor at the mosaic's centres ----------------------------------------------------------------------------------------
def test_mosaic_centres_reach_the_descriptor_limits(grad_host):
    m = vc.mosaic()
    xs, ys = _centres()
    bins = gd.direction(m, xs, ys)
    S = gd.box_sum(m)
    rows, acc, n2 = gd.rows_parts(S, xs, ys, bins)
    n1 = gd.isqrt((acc * acc).sum(1))
    clipped = (acc > (n1 // 5)[:, None]).any(1)
    with_255 = (rows == 255).any(1)
    zero = ~rows.any(1)
    print(f"\nbins {sorted(set(bins.tolist())) == list(range(32))}, largest accumulator {int(acc.max())}, rows with a 255 {np.flatnonzero(with_255).tolist()}, "
          f"all-zero rows {np.flatnonzero(zero).tolist()}, clipped rows {int(clipped.sum())}, n' of the 100 / 101 patch {int(n2[vc.SMALLEST_STEP])}, "
          f"largest n' {int(n2.max())}")
    assert bins[:32].tolist() == list(range(32))                                     # half-plane k has direction bin k: all 32 occur
    assert acc.max() > 1 << 23                                                       # past what 24 bits hold
    assert acc.max() < 1 << 27                                                       # (the header's bound on the LDS accumulators)
    assert with_255.sum() >= 1 and with_255[list(vc.FAR_EDGES)].all()                # the min(255, ...) cut
    assert zero.sum() >= 2 and zero[vc.FLAT] and zero[vc.CHECKERBOARDS[0]]           # no gradient in the box sums: n' = 0
    assert (n2[zero] == 0).all() and (n2[~zero] > 0).all() and (acc[zero] == 0).all()
    assert clipped[list(vc.HALF_PLANES)].all()                                       # v > n // 5 in every half-plane row
    assert n2[vc.SMALLEST_STEP] == n2[~zero].min() and 0 < n2[vc.SMALLEST_STEP] < 1 << 16
    # the host build of grad_desc_core.h on the same positions
    xyb = np.ascontiguousarray(np.stack([xs, ys, bins], axis=1), dtype=np.int32)
    got = np.full((len(xyb), 128), -3.0, dtype=np.float32)
    assert grad_host.gd_host_rows(S.ctypes.data, S.shape[1], S.shape[0], xyb.ctypes.data, len(xyb), got.ctypes.data) == 0
    assert got.tobytes() == rows.tobytes()
    # describe() -- what the GPU test compares with -- is those rows, and refuses the four records that test interleaves
    status, kp, want = gd.describe(m, vc.centre_records(gms_oracle.KEYPOINT_DTYPE))
    assert status == 0 and want.tobytes() == rows.tobytes() and np.array_equal(kp["angle"], np.float32(11.25) * bins.astype(np.float32))
    mixed, refused = vc.mixed_records(gms_oracle.KEYPOINT_DTYPE)
    status, kp, want = gd.describe(m, mixed)
    assert status == 1 and len(mixed) == 66 and np.array_equal(np.isnan(want).all(1), refused) and refused.sum() == 17
    assert want[~refused][:48].tobytes() == rows.tobytes() and kp[refused].tobytes() == mixed[refused].tobytes()
    groups = refused[:64].reshape(16, 4)
    assert (groups.sum(1) == 1).all() and (groups.sum(0) == 4).all()                 # every position of a workgroup, beside active ones
    at = np.flatnonzero(refused[:64])
    assert {(int(j % 4), float(mixed["x"][j]), float(mixed["y"][j])) for j in at} == {(p, float(x), float(y)) for p in range(4) for x, y in vc.REFUSED}


# ---- FAST ---------------------------------------------------------------------------------------------------------------------------------
def test_mosaic_through_the_pyramid_reaches_score_255(oracle):
    m = vc.mosaic()
    kp, _, lc = pyramid_ref.detect(oracle, m, 20, 10000, 8)
    bins = np.rint(kp["angle"] / np.float32(11.25)).astype(np.int64)
    print(f"\n(20, 10000, 8): per level {lc.tolist()}, {int((kp['response'] == 255).sum())} of response 255, {len(set(bins.tolist()))} bins")
    assert (lc > 0).all() and (kp["response"] == 255).any() and sorted(set(bins.tolist())) == list(range(32))
    kp, _, lc = pyramid_ref.detect(oracle, m, 254, 10000, 8)
    print(f"(254, 10000, 8): per level {lc.tolist()}")
    assert len(kp) > 0 and (kp["response"] == 255).all()
    level0 = int(lc[0])
    levels = pyramid_ref.build(m, 8)
    quotas = pyramid_ref.quotas([(l.shape[1], l.shape[0]) for l in levels], 37)
    kp, _, lc = pyramid_ref.detect(oracle, m, 254, 37, 8)
    print(f"(254, 37, 8): quotas {quotas}, per level {lc.tolist()}; level 0 has {level0} candidates of score 255")
    assert 0 < quotas[0] < level0 and lc[0] == quotas[0] and (kp["response"] == 255).all()       # the cut falls inside the tie at 255
    full = oracle.detect(m, 254, 10000)[0]
    assert oracle.detect(m, 254, quotas[0])[0].tobytes() == full[:quotas[0]].tobytes()           # ... and keeps the first in raster order


@pytest.mark.parametrize("w,h", vc.DOTS_SIZES)
def test_dots_are_corners_of_score_255(oracle, w, h):
    for fg, bg in ((255, 0), (0, 255)):
        img = vc.dots(w, h, fg, bg)
        kp, rows = oracle.detect(img, 254, 10000)
        ys, xs = np.nonzero(img == fg)
        print(f"\n{w} x {h}, {fg} on {bg}: {len(kp)} keypoints of response {sorted(set(kp['response'].tolist()))}")
        assert len(kp) == len(xs) > 7 and (kp["response"] == 255).all()
        assert (w, h) != (97, 65) or len(kp) == 45
        assert np.array_equal(kp["x"], xs) and np.array_equal(kp["y"], ys)                       # every dot, raster order
        kp7, rows7 = oracle.detect(img, 254, 7)
        assert len(kp7) == 7 and kp7.tobytes() == kp[:7].tobytes() and rows7.tobytes() == rows[:7].tobytes()
        assert oracle.detect_maps(img)[0].max() == 255                                           # the score image's top


# ---- DoG -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosaic", "discs"])
def test_contrast_on_a_candidates_own_value_decides_at_equality(name):
    img = {"mosaic": vc.mosaic, "discs": vc.discs}[name]()
    D1 = dog_ref.layers(img)[1]
    n0 = int(np.count_nonzero(dog_ref.candidates(img, 0)))
    for which, (c, x, y) in vc.own_contrasts(name).items():
        at, below = dog_ref.candidates(img, c), dog_ref.candidates(img, c - 1)
        print(f"\n{name}, {which} of {n0} candidates: c* = {c} at ({x}, {y}); {int(np.count_nonzero(below))} candidates at c* - 1, {int(np.count_nonzero(at))} at c*")
        assert abs(int(D1[y, x])) == c and 1 <= c <= 65535
        assert np.count_nonzero(at) < np.count_nonzero(below) and below[y, x] > 0 and at[y, x] == 0
        assert (below[at > 0] == at[at > 0]).all()                                               # a higher contrast only removes
    weakest, strongest = vc.own_contrasts(name)["weakest"][0], vc.own_contrasts(name)["strongest"][0]
    assert weakest < strongest and np.count_nonzero(dog_ref.candidates(img, weakest - 1)) == n0
    assert not dog_ref.candidates(img, strongest).any()
    assert vc.contrast_set(name) == sorted({0, weakest - 1, weakest, strongest - 1, strongest, 65535})


def _largest_terms(imgs):
    best = dict(det16=0, nx=0, ny=0)
    for img in imgs:
        t = dog_refine_ref.terms(img, 0)
        if len(t["xs"]):
            best = {k: max(v, int(np.abs(t[k]).max())) for k, v in best.items()}
    return best


def test_discs_bring_the_refinement_terms_past_the_small_images():
    small = _largest_terms(img for w, h in SMALL_SIZES for img in small_images(w, h))
    got = _largest_terms([vc.discs()])
    print(f"\nlargest det16, |nx|, |ny|: discs {got['det16']}, {got['nx']}, {got['ny']}; small_images {small['det16']}, {small['nx']}, {small['ny']}; "
          f"mosaic {_largest_terms([vc.mosaic()])}")
    assert got["det16"] > small["det16"] and got["nx"] > small["nx"] and got["ny"] > small["ny"]
    xs, ys, ox, oy, os_ = dog_refine_ref.offsets_at(vc.discs(), 0)
    near = [(int(x), int(y)) for x, y in zip(xs, ys)]
    for cx, cy in (vc.DISC_CENTRES[0], vc.DISC_CENTRES[4]):                                      # the two discs of radius 2: found, and moved
        i = near.index((int(cx), int(cy)))                                                       # towards where the centre is, unclamped
        assert 0 < int(ox[i]) < 8 and 0 < int(oy[i]) < 8


@pytest.mark.parametrize("name", ["mosaic", "discs"])
def test_host_builds_equal_the_statements_on_the_planes(dog_host, refine_host, name):
    imgs = {"mosaic": vc.mosaic_batch, "discs": vc.discs_batch}[name]()
    n = 0
    for img in imgs:
        img = np.ascontiguousarray(img)
        h, w = img.shape
        for contrast in vc.contrast_set(name):
            cand = dog_ref.candidates(img, contrast)
            want = dog_refine_ref.offsets(img, contrast, cand)
            got = np.full((h, w), 9, dtype=np.uint8)
            assert dog_host.dog_host_candidates(img.ctypes.data, w, h, contrast, got.ctypes.data) == np.count_nonzero(cand)
            assert np.array_equal(got, cand), contrast
            got_cand, got_codes = np.full((h, w), 9, dtype=np.uint8), np.full((h, w), 9, dtype=np.uint16)
            rc = refine_host.dog_refine_host_offsets(img.ctypes.data, w, h, contrast, got_cand.ctypes.data, got_codes.ctypes.data)
            assert rc == np.count_nonzero(cand) and np.array_equal(got_cand, cand) and np.array_equal(got_codes, want), contrast
            n += rc
    assert n > 0
