"""CPU: the named portrait cases (tests/portrait_cases.py) hold what they are named for. Every case's dilated mask
goes through the independent connected-components form, and every entry of its `facts` is asserted against the statement
(tests/portrait_ref.py) -- so the conditions that the GPU tests rely on (more than 1024 borders, exactly 64 chosen, tied or not tied
at the cut as declared, chains past 30 000, dilations 5 to 8, sides of 1 and 8192) are held here and no case is left out at run time."""
import numpy as np
import pytest

import portrait_cases as C
import portrait_ref as R


def test_names_are_the_cases():
    assert tuple(c["name"] for c in C.all_cases()) == C.NAMES and len(set(C.NAMES)) == len(C.NAMES)
    for c in C.all_cases():
        assert not c["disparity"].flags.writeable and not c["image"].flags.writeable
        assert c["image"].shape == c["disparity"].shape + (3,) and c["image"].dtype == c["disparity"].dtype == np.uint8
        assert set(c["params"]) == set(R.PARAM_NAMES)
        R.check(c["params"], c["disparity"].shape[1], c["disparity"].shape[0])


@pytest.mark.parametrize("name", C.NAMES)
def test_case_holds_its_facts(name):
    c = C.case(name)
    p, facts = c["params"], c["facts"]
    H, W = c["disparity"].shape
    want = C.expected(name)
    mask, info = want["mask"], want["info"]
    contours = info["contours"]
    if p["dilate_iterations"] == 0:
        assert np.array_equal(mask, want["thresh"])
    C.check_mask(mask, contours)
    areas = sorted((-k[0] for k in info["keys"]), reverse=True)
    got = dict(borders=len(contours), chosen=len(info["chosen"]), selected=int((want["selected"] != 0).sum()),
               longest_chain=max(len(ch) for _, ch in contours), tied=R.cut_is_tied(contours, W, p["num_contours"]),
               chosen_starts=[contours[i][1][0] for i in info["chosen"]], areas=areas)
    print(name, f"{W} x {H}", {k: got[k] for k in ("borders", "chosen", "selected", "longest_chain", "tied")})
    for k in ("borders", "chosen", "selected", "longest_chain", "tied"):
        assert got[k] == facts[k], (name, k, got[k], facts[k])
    for k in ("chosen_starts", "areas"):
        if k in facts:
            assert got[k] == list(facts[k]), (name, k)
    if "blob" in facts:
        y0, y1, x0, x1 = facts["blob"]
        assert (mask[y0:y1, x0:x1] != 0).all()
    assert set(facts) <= set(got) | {"blob"}
    if got["tied"]:      # the tie is real: the first border left out would be chosen by another order of equal areas
        order, keys = info["order"], info["keys"]
        n = p["num_contours"]
        assert keys[order[n - 1]][0] == keys[order[n]][0] and keys[order[n - 1]][1:] < keys[order[n]][1:]
    if H > 3 and W > 3:
        keep = want["selected"][:H - 3, :W - 3] != 0
        assert np.array_equal(want["out"][:H - 3, :W - 3][keep], c["image"][:H - 3, :W - 3][keep])
    else:
        assert np.array_equal(want["out"], want["blurred"])


def _facts(name):
    return C.case(name)["facts"]


def test_cases_cover_what_they_are_for():
    """The conditions of the issue, on the facts that test_case_holds_its_facts pins to the statement."""
    f = _facts("noise_64")
    assert f["borders"] > 1024 and f["chosen"] == 64 and not f["tied"]
    f = _facts("dots_lattice_64")
    assert f["borders"] > 1024 and f["chosen"] == 64 and f["tied"]
    tied = [n for n in C.NAMES if _facts(n)["tied"]]
    assert set(tied) == {"dots_lattice_64", "dots_lattice_5", "equal_squares_staggered_5", "equal_squares_staggered_1", "ring_then_blob",
                         "blob_then_ring", "serpentine_inverse", "row_8192_2", "column_8192_2"}
    assert [C.case(f"dilate_{it}")["params"]["dilate_iterations"] for it in (5, 6, 7, 8)] == [5, 6, 7, 8]
    assert _facts("serpentine")["longest_chain"] > 30000 and _facts("comb")["longest_chain"] > 30000
    shapes = {n: C.case(n)["disparity"].shape for n in C.NAMES}
    assert shapes["row_8192_2"] == shapes["row_8192_64"] == (1, 8192) and shapes["column_8192_2"] == shapes["column_8192_64"] == (8192, 1)
    assert shapes["row_3"] == (1, 3) and shapes["column_3"] == (3, 1)
    assert C.case("row_3")["params"]["median_ksize"] == C.case("column_3")["params"]["median_ksize"] == 31
    assert shapes["large_blobs"] == (515, 1030) and _facts("large_blobs")["borders"] > 1024
    assert _facts("ring_then_blob")["selected"] == 81 and _facts("blob_then_ring")["selected"] == 81 + 96


def test_dilation_cases_reach_every_edge_and_corner():
    H, W = 70, 150
    near = lambda y, x: (y <= 8, y >= H - 9, x <= 8, x >= W - 9)      # top, bottom, left, right
    sides = [near(y, x) for y, x in C.DOTS]
    for k in range(4):
        assert any(s[k] and sum(s) == 1 for s in sides)               # an edge alone
    for a, b in ((0, 2), (0, 3), (1, 2), (1, 3)):
        assert any(s[a] and s[b] for s in sides)                      # a corner
    for it in (5, 6, 7, 8):
        c = C.case(f"dilate_{it}")
        thresh = R.threshold_mask(c["disparity"], c["params"]["threshold"])
        assert int((thresh != 0).sum()) == len(C.DOTS) and (c["disparity"] == 255).any() and (c["disparity"] == 60).any()
        mask = C.expected(c["name"])["mask"]
        assert mask[0].any() and mask[-1].any() and mask[:, 0].any() and mask[:, -1].any()      # squares cut off at all four sides
        want = thresh.copy()
        for _ in range(it):                                           # literal 3 x 3 passes
            q = np.pad(want, 1, mode="edge")
            want = np.max([q[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)
        assert np.array_equal(mask, want)


def test_check_mask_equals_the_whole_map_form_on_small_cases():
    """portrait_cases.check_mask decides inside each border's box; test_portrait_ref._check_mask decides on the whole map. Both
    accept the small cases, and check_mask refuses a list or a chain that is not the mask's."""
    import test_portrait_ref as T
    for name in ("rings", "ring_then_blob", "equal_squares_staggered_5", "dilate_8"):
        mask = C.expected(name)["mask"]
        cs = T._check_mask(mask)
        assert cs == C.expected(name)["info"]["contours"]
    mask = C.expected("rings")["mask"]
    cs = list(C.expected("rings")["info"]["contours"])
    with pytest.raises(AssertionError):
        C.check_mask(mask, cs[:-1])                                   # a border missing
    hole, chain = cs[1]
    with pytest.raises(AssertionError):
        C.check_mask(mask, [cs[0], (hole, chain[:5] + chain[6:])] + cs[2:])     # a chain with a point left out
