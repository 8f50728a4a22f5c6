"""Inputs of the semi-global matching tests: every disparity count at which the kernels' lane layout changes, the
shortest paths, block sizes 7, 9, 21 and 51 across the cost kernel's tile and band seams, its largest LDS request, disparity ranges
wholly below 0, sloped winners at both ends of the range, a partial texture cut, regions whose diagonals start on each edge, exact
ties of the summed cost across lanes, sums in the upper half of the unsigned 16-bit range, the penalty extremes, and StereoBM's rules
(uniqueness, left-right check, minimum disparity) on the sums.
case(name) returns (left, right, params); expected(name) the statement's (disp, cost), computed once; census(left, right, **params)
counts on the statement's own pieces what a case is named for. tests/test_stereo_sgm_ref.py asserts FLOORS from the census on the
CPU, and tests/test_gpu_stereo_sgm.py holds the GPU to the statement's bytes on the same inputs.

A "shifted" right image is np.roll(left, -s, axis=1): the true disparity is s. Parameters not given are the reference's StereoBM
values, p1 = 8 block_size^2, p2 = 32 block_size^2 and eight paths."""
import functools
import os

import numpy as np

import stereo_bm_cases as BC
import stereo_bm_ref as B
import stereo_sgm_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_stereo_pair_450x375.npz")
# part of a wave; one full set of cost lanes; a partly filled last register slot; every lane of the path and decision kernels active at
# the run lengths 2 and 4 (128, 256); the first count of run length 8; the most
ND_SWEEP = (16, 48, 64, 80, 128, 256, 272, 512)


def _smooth(name, h, w):
    """Noise averaged with its left and upper neighbour: costs fall towards the true disparity instead of being flat around it."""
    base = BC._rng(name).integers(0, 256, (h, w)).astype(np.int32)
    return ((base + np.roll(base, 1, axis=1) + np.roll(base, 1, axis=0)) // 3).astype(np.uint8)


def _two_shifts(name, h, w, s_top, s_bottom, noise=3):
    """The upper half shifted by s_top, the lower by s_bottom, noise in [-noise, noise] on the right image: two disparity levels, a jump
    between them that the vertical and diagonal paths cross, and pixels the left-right check removes."""
    left = _smooth(name, h, w)
    right = np.concatenate([BC.shifted(left[:h // 2], s_top), BC.shifted(left[h // 2:], s_bottom)]).astype(np.int32)
    right = right + BC._rng(name + "_noise").integers(-noise, noise + 1, (h, w))
    return left, np.clip(right, 0, 255).astype(np.uint8)


def _nd(nd):
    left, right = _two_shifts(f"nd{nd}", 24, nd + 40, 1, nd - 5)
    return left, right, dict(num_disparities=nd, min_disparity=0, texture_threshold=0)


def _region(name, ny, wx, **kw):
    """A pair whose computed region is ny x wx with 16 disparities from 0 and block size 5."""
    left, right = _two_shifts(name, ny + 4, wx + 15, 2, 9)
    return left, right, dict(num_disparities=16, min_disparity=0, texture_threshold=0, **kw)


def _unsigned_range():
    return BC._noise("sgm_range_left", 24, 96), BC._noise("sgm_range_right", 24, 96), dict(
        num_disparities=32, min_disparity=0, pre_filter_cap=63, texture_threshold=0, p1=5041, p2=5041, n_paths=8)


def _bm_case(name, shift=None, **more):
    left, right, kw = BC.case(name)
    return left, (left if shift == 0 else right), dict(kw, **more)


def _md(md):
    left, right = _two_shifts("md", 30, 110, 4 + max(md, 0), 20 + max(md, 0))
    return left, right, dict(num_disparities=32, min_disparity=md, texture_threshold=0)


def _lr(maxdiff):
    left, right = _two_shifts("lr", 30, 120, 3, 25, noise=6)
    return left, right, dict(num_disparities=32, min_disparity=0, texture_threshold=0, disp12_max_diff=maxdiff)


def _block(name, bs, ny, wx, nd=16, shifts=(2, 9), **kw):
    """A two-shift pair whose computed region is ny x wx with nd disparities from 0 and block size bs. The texture threshold is the
    reference's, unless given."""
    left, right = _two_shifts(name, ny + bs - 1, wx + nd - 1, *shifts)
    return left, right, dict(num_disparities=nd, min_disparity=0, block_size=bs, **kw)


def _negative(name, h, w, nd, md, s_top, s_bottom):
    """A range at or below 0: the right image is the left shifted the other way, np.roll(left, +s), so the true disparities are -s_top
    and -s_bottom."""
    left, right = _two_shifts(name, h, w, -s_top, -s_bottom)
    return left, right, dict(num_disparities=nd, min_disparity=md, texture_threshold=0)


def _ends():
    left, right = _two_shifts("ends", 44, 75, 0, 15)
    return left, right, dict(num_disparities=16, min_disparity=0, texture_threshold=0, uniqueness_ratio=0)


def _bs51_nd512(**kw):
    left, right = _two_shifts("bs51_nd512", 60, 583, 0, 400)
    return left, right, dict(num_disparities=512, min_disparity=0, block_size=51, texture_threshold=0, p1=200, **kw)


BUILDERS = {
    # the shortest paths: two rows (H = block_size + 1), and one column (wx = 1)
    "two_rows": lambda: _region("two_rows", 2, 45),
    "one_column": lambda: _region("one_column", 20, 1),
    # diagonals that start on the top / bottom edge mostly, and on the side edges mostly
    "diag_wide": lambda: _region("diag_wide", 20, 45),
    "diag_tall": lambda: _region("diag_tall", 45, 20),
    "four_paths": lambda: _region("diag_wide", 20, 45, n_paths=4),
    # every cost 0: every S is 0, the winner is k = 0 everywhere
    "const": lambda: _bm_case("const"),
    # left = right stripes: equal S every 8 disparities (across lanes) and 64 apart: the lowest k must win
    "stripes8": lambda: _bm_case("stripes8", shift=0),
    "stripes64": lambda: _bm_case("stripes64", shift=0),
    # independent noise, the largest penalties the parameter rule admits: most S in the upper half of 16 unsigned bits
    "unsigned_range": _unsigned_range,
    # the penalty extremes
    "p1_zero": lambda: _region("penalty", 20, 45, p1=0, p2=300),
    "p1_eq_p2": lambda: _region("penalty", 20, 45, p1=150, p2=150),
    # StereoBM's rules on S
    "uniq_10": lambda: _bm_case("stripes64_noise", uniqueness_ratio=10),
    "uniq_15": lambda: _bm_case("stripes64_noise", uniqueness_ratio=15),
    # the same stripes with noise drawn apart for the two sides: the rule cuts about a fifth
    "uniq_10_noise2": lambda: _bm_case("stripes64_noise2", uniqueness_ratio=10),
    "uniq_15_noise2": lambda: _bm_case("stripes64_noise2", uniqueness_ratio=15),
    "lr_off": lambda: _lr(-1),
    "lr_0": lambda: _lr(0),
    "lr_2": lambda: _lr(2),
    "md_negative": lambda: _md(-7),
    "md_zero": lambda: _md(0),
    "md_positive": lambda: _md(5),
    # GMS_STEREO_BM_MAX_WIDTH: the longest horizontal paths, the shortest vertical ones
    "widest": lambda: _bm_case("widest"),
    # block sizes past 5 in the cost kernel. A region of 33 x 65 (34 x 66) is one row (two) into the second 32-row band and one column
    # (two) into the second 64-column tile: 8 (49 * 122 + 1568) = 60 368; 8 (81 * 62 + 2592) = 60 912 (cap 61 is rejected at block 9)
    "bs7_seams": lambda: _block("bs7_seams", 7, 33, 65),
    "bs9_seams": lambda: _block("bs9_seams", 9, 33, 65, pre_filter_cap=31),
    "bs21": lambda: _block("bs21", 21, 20, 89, nd=32, shifts=(3, 25), pre_filter_cap=3, p1=100, p2=1000),
    "bs51_seams": lambda: _block("bs51_seams", 51, 34, 66, pre_filter_cap=1, texture_threshold=0, p1=200, p2=2000),
    # the cost kernel's largest LDS request, (32 + 50) (128 + 100 + 511) = 60 598 bytes, with the last accepted p2 of 8 and of 4 paths:
    # 8 (2601 * 2 + 2989) = 65 528, 4 (2601 * 6 + 777) = 65 532
    "bs51_nd512": lambda: _bs51_nd512(pre_filter_cap=1, p2=2989),
    "bs51_nd512_four": lambda: _bs51_nd512(pre_filter_cap=3, p2=777, n_paths=4),
    # ranges wholly below 0 (rofs = -(nd - 1 + md) > 0, lofs = 0: the region starts at column 0), and nd - 1 + md = 0: both offsets 0
    "rofs_5": lambda: _negative("rofs_5", 30, 90, 16, -20, 6, 18),
    "rofs_1": lambda: _negative("rofs_1", 30, 110, 32, -32, 4, 27),
    "offsets_zero": lambda: _negative("offsets_zero", 30, 110, 32, -31, 2, 26),
    # winners at k = nd - 1 (disparity 0, the upper half) and at k = 0 (disparity 15) whose one neighbour differs from them: the subpixel
    # step's mirrored neighbour decides the map
    "ends": _ends,
    # StereoBM's case: the texture rule cuts the flat part and leaves the rest
    "half_flat": lambda: _bm_case("half_flat"),
}
for _n in ND_SWEEP:
    BUILDERS[f"nd_{_n}"] = functools.partial(_nd, _n)
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(left, right, params) of a named case; the arrays are read-only."""
    left, right, kw = BUILDERS[name]()
    for a in (left, right):
        a.setflags(write=False)
    return left, right, kw


def _frozen(pair):
    for a in pair:
        a.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def expected(name):
    """The statement's (disp int16, cost int32) of a named case, computed once per session; read-only."""
    left, right, kw = case(name)
    return _frozen(R.stereo_sgm(left, right, **kw))


@functools.lru_cache(maxsize=None)
def golden_pair():
    z = np.load(GOLDEN)
    return _frozen((z["left"], z["right"], z["gt"]))


@functools.lru_cache(maxsize=None)
def golden_expected(n_paths):
    """The statement on the committed 450 x 375 pair with the reference's parameters, computed once per session; read-only."""
    left, right, _ = golden_pair()
    return _frozen(R.stereo_sgm(left, right, n_paths=n_paths))


def run_length(nd):
    """The consecutive disparities a lane of the path and decision kernels holds."""
    return 2 if nd <= 128 else 4 if nd <= 256 else 8


def census(left, right, **kw):
    """What the statement's pieces count over the computed region (ny x wx pixels)."""
    p, left, right, H, W = R._prepare(left, right, kw)
    nd = p["num_disparities"]
    inv = B.filtered_value(p)
    disp, cost, dec = R.raw_maps(left, right, p)
    if dec is None:
        return dict(computed=0, valid=0)
    S, mind = dec["S"], dec["mind"]
    ny, wx, _ = S.shape
    at_min = S == S.min(axis=2, keepdims=True)
    lane = np.arange(nd) // run_length(nd)
    accepted = dec["tex_ok"] & dec["uniq_ok"]
    out = dict(computed=ny * wx, ny=ny, wx=wx,
               tied=int((at_min.sum(axis=2) > 1).sum()),
               tied_across_lanes=int((at_min & (lane[None, None, :] != lane[mind][:, :, None])).any(axis=2).sum()),
               all_zero=int((S.max(axis=2) == 0).sum()),
               upper_half_share=float((S >= 32768).mean()), s_max=int(S.max()),
               uniqueness_cut=int((dec["tex_ok"] & ~dec["uniq_ok"]).sum()),
               accepted=int(accepted.sum()),
               winner_first=int((accepted & (mind == 0)).sum()),
               winners_low=int((accepted & (mind < nd // 2)).sum()),
               winners_high=int((accepted & (mind >= nd // 2)).sum()),
               last_lane_wins=int((accepted & (lane[mind] == lane[-1])).sum()),
               moved_by_paths=int((mind != dec["C"].argmin(axis=2)).sum()),
               lofs=B.ranges(p, W)[0], rofs=B.ranges(p, W)[1],
               texture_cut=int((~dec["tex_ok"]).sum()),
               winner_first_sloped=int((accepted & (mind == 0) & (S[:, :, 1] != S[:, :, 0])).sum()),
               winner_last_sloped=int((accepted & (mind == nd - 1) & (S[:, :, nd - 2] != S[:, :, nd - 1])).sum()),
               lr_removed=0)
    if p["disp12_max_diff"] >= 0:
        checked = disp.copy()
        B.validate(checked, cost, p)
        out["lr_removed"] = int(((disp != inv) & (checked == inv)).sum())
        disp = checked
    B.roi_fill(disp, p, B.ranges(p, W)[0])
    out["valid"] = int((disp != inv).sum())
    return out


# name -> {census key: floor}: what the case is for; "==" keys are exact. tests/test_stereo_sgm_ref.py asserts them.
FLOORS = {
    "two_rows": dict(ny=("==", 2), accepted=1),
    "one_column": dict(wx=("==", 1), accepted=1),
    "diag_wide": dict(ny=("==", 20), wx=("==", 45), winners_low=1, winners_high=1, moved_by_paths=1),
    "diag_tall": dict(ny=("==", 45), wx=("==", 20), winners_low=1, winners_high=1, moved_by_paths=1),
    "four_paths": dict(winners_low=1, winners_high=1),
    "const": dict(all_zero=("==", "computed"), winner_first=("==", "computed")),
    "stripes8": dict(tied_across_lanes=1000),
    "stripes64": dict(tied_across_lanes=1000),
    "unsigned_range": dict(upper_half_share=0.5, s_max=32768),
    "p1_zero": dict(winners_low=1, winners_high=1),
    "p1_eq_p2": dict(winners_low=1, winners_high=1),
    "uniq_10": dict(uniqueness_cut=5, accepted=100),       # the sums are smooth where the two sides share their noise: few cuts
    "uniq_15": dict(uniqueness_cut=5, accepted=100),
    "uniq_10_noise2": dict(uniqueness_cut=500, accepted=500),
    "uniq_15_noise2": dict(uniqueness_cut=500, accepted=500),
    "lr_off": dict(lr_removed=("==", 0), accepted=100),
    "lr_0": dict(lr_removed=10),
    "lr_2": dict(lr_removed=1),
    "md_negative": dict(winners_low=1, winners_high=1),
    "md_zero": dict(winners_low=1, winners_high=1),
    "md_positive": dict(winners_low=1, winners_high=1),
    "widest": dict(wx=("==", B.MAX_WIDTH - 15), accepted=1000),
    "bs7_seams": dict(ny=("==", 33), wx=("==", 65), winners_low=100, winners_high=100, upper_half_share=0.3),
    "bs9_seams": dict(ny=("==", 33), wx=("==", 65), winners_low=100, winners_high=100),
    "bs21": dict(ny=("==", 20), wx=("==", 89), winners_low=100, winners_high=100),
    "bs51_seams": dict(ny=("==", 34), wx=("==", 66), winners_low=100, winners_high=100),
    "bs51_nd512": dict(ny=("==", 10), wx=("==", 72), upper_half_share=0.5, winners_low=20, winners_high=20, winner_last_sloped=20),
    "bs51_nd512_four": dict(ny=("==", 10), wx=("==", 72), upper_half_share=0.5, winners_low=20, winners_high=20, winner_last_sloped=20),
    "rofs_5": dict(rofs=("==", 5), lofs=("==", 0), ny=("==", 26), wx=("==", 70), winners_low=100, winners_high=100),
    "rofs_1": dict(rofs=("==", 1), lofs=("==", 0), winners_low=100, winners_high=100),
    "offsets_zero": dict(rofs=("==", 0), lofs=("==", 0), winners_low=100, winners_high=100),
    "ends": dict(winner_first_sloped=200, winner_last_sloped=200),
    "half_flat": dict(texture_cut=500, accepted=500),
}
for _n in ND_SWEEP:
    FLOORS[f"nd_{_n}"] = dict(winners_low=1, winners_high=1, last_lane_wins=1 if _n > 16 else 0)
for _n in (128, 256):      # every lane active: lane 63 owns the winner, next to a value that differs from it
    FLOORS[f"nd_{_n}"].update(last_lane_wins=50, winner_last_sloped=5)


def check_floors(name, got):
    """Assert the census `got` of a named case against its floors."""
    for key, floor in FLOORS[name].items():
        if isinstance(floor, tuple):
            want = got[floor[1]] if isinstance(floor[1], str) else floor[1]
            assert got[key] == want, (name, key, got[key], want)
        else:
            assert got[key] >= floor, (name, key, got[key], floor)
