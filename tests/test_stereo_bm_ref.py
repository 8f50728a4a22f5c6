"""CPU: the StereoBM statement (tests/stereo_bm_ref.py) -- hand-worked cases for each rule, the literal loop against
the vectorised form over a parameter sweep, the reference's parameters on its own 450 x 375 pair against the ground truth, and the
named edge cases of tests/stereo_bm_cases.py: each contains what it is named for, by the statement's own census."""
import os

import numpy as np
import pytest

import stereo_bm_cases as C
import stereo_bm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_stereo_pair_450x375.npz")


# ---- pre-filter -------------------------------------------------------------------------------------------------------------------
EVEN = np.array([[0, 1, 3, 6], [0, 2, 4, 8]], np.uint8)
ODD = np.array([[0, 1, 3, 6], [0, 2, 4, 8], [9, 0, 0, 9]], np.uint8)


@pytest.mark.parametrize("form", [R.prefilter_xsobel_loop, R.prefilter_xsobel])
def test_prefilter_even_height(form):
    # d(row 0) = (3, 5), d(row 1) = (4, 6); row 0 reflects to row 1 above, row 1 to row 0 below: 4 + 6 + 4 = 14, 6 + 10 + 6 = 22
    want = np.array([[31, 45, 53, 31], [31, 45, 53, 31]], np.uint8)
    assert (form(EVEN, 31) == want).all()


@pytest.mark.parametrize("form", [R.prefilter_xsobel_loop, R.prefilter_xsobel])
def test_prefilter_odd_height_last_row_constant(form):
    # row 1 now has row 2 below: 3 + 8 - 9 = 2, 5 + 12 + 9 = 26; row 2 is left over: all cap
    want = np.array([[31, 45, 53, 31], [31, 33, 57, 31], [31, 31, 31, 31]], np.uint8)
    assert (form(ODD, 31) == want).all()
    # saturation at cap: 14, 22 and 26 clamp to 5 (-> 10), 2 stays (-> 7)
    assert (form(ODD, 5)[:2, 1:3] == [[10, 10], [7, 10]]).all()


def test_prefilter_forms_agree_random():
    rng = np.random.default_rng(3)
    for h, w in ((1, 5), (2, 3), (7, 9), (8, 10), (33, 17)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        for cap in (1, 15, 31, 61, 63):
            assert (R.prefilter_xsobel_loop(img, cap) == R.prefilter_xsobel(img, cap)).all()


# ---- decision ---------------------------------------------------------------------------------------------------------------------
def test_cost_tie_goes_to_largest_disparity():
    p = R.make_params(num_disparities=16, min_disparity=0, texture_threshold=0)
    sad = [50] * 16
    sad[4] = sad[9] = 7                        # k = 4 means disparity 11, k = 9 disparity 6
    assert R.winner(sad) == (4, 7)
    d, c = R.decide(sad, 0, p)
    assert c == 7 and d >> 4 == 11             # subpixel: p = n = 50 -> no offset
    assert np.argmin(np.array(sad)) == 4       # the vectorised form's rule


@pytest.mark.parametrize("nd,md,mind,p,n,c,want", [
    (16, 0, 5, 10, 20, 4, 155),    # den 32, (p - n) 256 / den = -80: (2560 - 80 + 15) >> 4
    (16, 0, 5, 26, 29, 4, 160),    # -768 / 50 = -15.36 truncates to -15 (flooring would give 159)
    (16, -39, 5, 29, 26, 4, -463),  # 768 / 50 -> 15: (-7424 + 30) >> 4, an arithmetic shift (-462 if it truncated)
    (16, 0, 5, 9, 9, 9, 160),      # den 0: no offset
    (224, -39, 0, 100, 100, 10, 2944),  # (184 * 256 + 15) >> 4
])
def test_subpixel(nd, md, mind, p, n, c, want):
    assert R.subpixel(nd, md, mind, p, n, c) == want


def test_texture_and_uniqueness():
    p = R.make_params(num_disparities=16, min_disparity=0, texture_threshold=100, uniqueness_ratio=15)
    sad = [200] * 16
    sad[6], sad[7] = 100, 110                  # the neighbour of the winner may be close
    assert R.decide(sad, 99, p) is None        # texture below the threshold
    assert R.decide(sad, 100, p) is not None
    sad[12] = 115                              # 115 <= 100 + 100 * 15 // 100: not unique
    assert R.decide(sad, 100, p) is None
    sad[12] = 116
    assert R.decide(sad, 100, p) is not None
    assert R.decide(sad[:12] + [115] + sad[13:], 100, R.make_params(num_disparities=16, min_disparity=0, texture_threshold=100)) is not None


def _lr_row(maxdiff, c20, c21):
    p = R.make_params(num_disparities=16, min_disparity=0, disp12_max_diff=maxdiff)
    disp = np.full((1, 40), R.filtered_value(p), np.int16)
    cost = np.full((1, 40), -1, np.int32)
    disp[0, 20], cost[0, 20] = 64, c20         # x2 = 20 - 4 = 16
    disp[0, 21], cost[0, 21] = 80, c21         # x2 = 21 - 5 = 16
    a, b = disp.copy(), disp.copy()
    R.validate_loop(a, cost, p)
    R.validate(b, cost, p)
    assert (a == b).all()
    return a[0, 20], a[0, 21]


def test_left_right_tie_lowest_x_kept():
    F = R.filtered_value(R.make_params(min_disparity=0))
    assert _lr_row(0, 7, 7) == (64, F)         # equal costs: x = 20 takes column 16, x = 21 differs by 16 > 0
    assert _lr_row(0, 8, 7) == (F, 80)         # strictly cheaper x = 21 takes it
    assert _lr_row(1, 7, 7) == (64, 80)        # 16 > 16 is false


def test_width1_below_one_all_filtered():
    rng = np.random.default_rng(5)
    L = rng.integers(0, 256, (20, 100), dtype=np.uint8)
    for form in (R.stereo_bm_loop, R.stereo_bm):
        d, c = form(L, L, num_disparities=112, min_disparity=0)
        assert (d == -16).all() and (c == -1).all()


def test_bad_params_rejected():
    L = np.zeros((20, 40), np.uint8)
    for kw in (dict(block_size=6), dict(block_size=53), dict(num_disparities=24), dict(num_disparities=528), dict(pre_filter_cap=0),
               dict(pre_filter_cap=64), dict(speckle_window_size=100), dict(pre_filter_type=0), dict(block_size=21)):
        with pytest.raises(ValueError):
            R.stereo_bm(L, L, **kw)


# ---- the two forms agree ----------------------------------------------------------------------------------------------------------
def _pair(rng, h, w, shift):
    base = rng.integers(0, 256, (h, w + 16)).astype(np.int32)
    base = (base + np.roll(base, 1, axis=1) + np.roll(base, 1, axis=0)) // 3   # some spatial correlation
    left = base[:, 16:]
    right = base[:, 16 - shift:w + 16 - shift] + rng.integers(-3, 4, (h, w))
    return left.astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8)


SWEEP = [dict(block_size=5, num_disparities=16, min_disparity=0),
         dict(block_size=7, num_disparities=32, min_disparity=-5, pre_filter_cap=15, uniqueness_ratio=15, disp12_max_diff=0),
         dict(block_size=5, num_disparities=16, min_disparity=3, pre_filter_cap=31, texture_threshold=0, disp12_max_diff=-1),
         dict(block_size=9, num_disparities=16, min_disparity=-20, pre_filter_cap=63, texture_threshold=200, disp12_max_diff=4),
         dict(block_size=5, num_disparities=32, min_disparity=-39, texture_threshold=507, uniqueness_ratio=15, disp12_max_diff=1)]


@pytest.mark.parametrize("case", range(len(SWEEP)))
@pytest.mark.parametrize("hw", [(19, 44), (20, 45)])
def test_loop_equals_vectorised(case, hw):
    kw = SWEEP[case]
    rng = np.random.default_rng(100 * case + hw[0])
    left, right = _pair(rng, hw[0], hw[1], 4)
    a = R.stereo_bm_loop(left, right, **kw)
    b = R.stereo_bm(left, right, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- plausibility on the reference's pair -----------------------------------------------------------------------------------------
def test_reference_pair_plausible():
    z = np.load(GOLDEN)
    d, cost = R.stereo_bm(z["left"], z["right"])
    inv = R.filtered_value(R.REFERENCE_PARAMS)
    gt = z["gt"].astype(np.float64)
    m = (d != inv) & (gt > 0)
    err = np.abs(d[m] / 16.0 - gt[m] / 4.0)
    # the statement's own figures: 53 473 such pixels, 0.873 of them within 1 px, median error 0.125 px
    assert m.sum() > 40000
    assert (err <= 1.0).mean() >= 0.6
    assert np.median(err) < 0.5
    assert ((cost >= 0) | (cost == -1)).all()
    d8 = R.stereo_match(z["left"], z["right"])
    assert d8.dtype == np.uint8 and not (d8 == 0).any() and (d8[d == inv] == 255).all()


def test_normalize_rules():
    d = np.array([[-640, 0, 16], [3568, -640, 100]], np.int16)
    out = R.normalize_u8(d)
    assert out[0, 0] == 255 and out[1, 1] == 255            # the minimum maps to 0, then to 255
    assert out[1, 0] == 255
    flat = R.normalize_u8(np.full((2, 2), 7, np.int16))     # max == min: scale 0, everything 0 -> 255
    assert (flat == 255).all()


# ---- the named edge cases (tests/stereo_bm_cases.py) ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_cases_contain_what_they_are_for(name):
    """Conditions on the inputs, met by the statement alone: a case that stopped containing its rule would let the GPU test pass for
    nothing. A floor that fails for a new seed means another seed, not another floor."""
    left, right, kw = C.case(name)
    n = C.census(left, right, **kw)
    print(name, left.shape, n)
    assert n["computed"] > 0
    if name in ("const", "stripes8", "stripes64"):
        assert n["tied_across_slots"] == n["tied"] == n["computed"]
    if name in ("const_uniq", "stripes8_uniq"):
        assert n["uniqueness_cut"] == n["computed"] and n["valid"] == 0
    if name == "const_tex":
        assert n["texture_cut"] == n["computed"] and n["valid"] == 0
    if name == "const":
        assert n["denominator_zero"] >= 1000 and n["winner_first"] == n["computed"]
    if name == "stripes64":
        assert n["lr_contended"] >= 100 and n["lr_removed"] >= 100
    if name in ("stripes64_noise", "stripes64_noise2"):
        assert n["uniqueness_cut"] >= 500 and n["accepted"] >= 500
    if name == "stripes64_noise2":
        cost = C.expected(name)[1]
        assert cost[cost >= 0].min() > 0      # no exact match: every uniqueness threshold is above 0
    if name == "half_flat":
        assert 0.2 * n["computed"] <= n["texture_cut"] <= 0.6 * n["computed"] and n["accepted"] > 0
    if name.startswith("end_last"):
        assert n["winner_last"] >= 0.9 * n["accepted"] > 0
    if name.startswith("end_first"):
        assert n["winner_first"] >= 0.9 * n["accepted"] > 0
    if name in ("cap1", "widest") or name.startswith("largest_lds"):
        assert n["valid"] >= 300
    assert n["valid"] == int((C.expected(name)[0] != R.filtered_value(R.make_params(**kw))).sum())   # the census walks stereo_bm's path


def test_cases_reach_the_size_limits():
    left, _, kw = C.case("widest")
    assert left.shape[1] == R.MAX_WIDTH
    for name, lofs, rofs in (("largest_lds", 511, 0), ("largest_lds_rofs", 11, 0), ("largest_lds_rofs9", 0, 9)):
        left, _, kw = C.case(name)
        p = R.make_params(**kw)
        assert (p["block_size"], p["num_disparities"]) == (51, 512) and R.ranges(p, left.shape[1])[:2] == (lofs, rofs)
        assert left.shape[0] - 2 * (p["block_size"] // 2) <= 32     # one band: its LDS rows are the image's 60, not 32 + 50
    for nd, kpl, dead in ((80, 2, 48), (128, 2, 0), (256, 4, 0), (272, 8, 240)):
        assert C.case(f"end_last_{nd}")[2]["num_disparities"] == nd and (64 * kpl - nd, nd > 64 * kpl // 2) == (dead, True)


@pytest.mark.parametrize("name", C.CUT_DOWN)
def test_loop_equals_vectorised_on_cut_down_cases(name):
    left, right, kw = C.cut_down(name)
    n = C.census(left, right, **kw)
    if name in ("const", "const_uniq", "stripes8", "stripes64"):
        assert n["tied"] == n["computed"] > 0
    if name == "stripes64":
        assert n["lr_contended"] >= 20 and n["lr_removed"] >= 20    # validate_loop and validate on equal costs
    a = R.stereo_bm_loop(left, right, **kw)
    b = R.stereo_bm(left, right, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
