"""Inputs of the StereoBM tests that make the kernel's decision rules run: exact cost ties across lanes and register
slots, the texture and uniqueness rules at their cut-offs, winners at both ends of the disparity range (the mirrored neighbour of the
subpixel step), equal costs on one target column of the left-right check, and the size limits (width 8192, the largest LDS request).
case(name) returns (left, right, params), generated from SEED. census(left, right, **params) counts, with the statement's own pieces
(stereo_bm_ref.window_costs, decisions, lr_sources, validate), how often each rule decides: tests/test_stereo_bm_ref.py asserts from
it that every case contains what it is named for, on the CPU, and tests/test_gpu_stereo_bm.py holds the GPU to the statement's bytes on
the same inputs.

A "shifted" right image is np.roll(left, -s, axis=1): the true disparity is s. Parameters not given are the reference's."""
import functools

import numpy as np

import stereo_bm_ref as R

SEED = 2026


def _rng(name):
    return np.random.default_rng([SEED] + [ord(c) for c in name])


def _noise(name, h, w):
    return _rng(name).integers(0, 256, (h, w)).astype(np.uint8)


def _stripes(name, h, w, period, noise=0):
    """Vertical stripes of `period` random levels; with noise, integers in [-noise, noise] on every pixel."""
    rng = _rng(name)
    img = np.tile(rng.integers(0, 256, period), (h, (w + period - 1) // period))[:, :w].astype(np.int32)
    if noise:
        img = img + rng.integers(-noise, noise + 1, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def shifted(img, s):
    return np.roll(img, -s, axis=1)


def _const():
    return np.full((40, 200), 90, np.uint8)


def _half_flat():
    img = _noise("half_flat", 50, 260)
    img[:, :130] = (img[:, :130] // 64) * 2 + 100
    return img


# ND -> (min_disparity, further parameters) of the end_last_ND / end_first_ND pairs: KPL 2 with a partly filled and a full last slot,
# KPL 4 full, KPL 8 with three dead slots
ENDS = {80: (5, {}), 128: (0, dict(block_size=7)), 256: (-10, {}), 272: (-200, dict(uniqueness_ratio=10))}
END_SHAPE = (40, 360)


def _end(nd, first):
    md, more = ENDS[nd]
    left = _noise("end", *END_SHAPE)           # one left image for all eight
    s = md + nd - 1 if first else md           # the largest disparity is k = 0, the smallest k = nd - 1
    return _pair(left, s, num_disparities=nd, min_disparity=md, texture_threshold=0, **more)


def _largest_lds(md, s):
    left = _noise("largest_lds", 60, 600)
    return _pair(left, s, block_size=51, num_disparities=512, min_disparity=md, texture_threshold=0)


def _stripes64_noise2():
    left = _stripes("stripes64_noise", 40, 400, 64, noise=2)
    right = shifted(_stripes("stripes64_noise", 40, 400, 64), 5).astype(np.int32) + _rng("stripes64_noise2").integers(-2, 3, (40, 400))
    return left, np.clip(right, 0, 255).astype(np.uint8), dict(_S64_KW, uniqueness_ratio=15)


_CONST_KW = dict(num_disparities=144, min_disparity=-3)
_S8_KW = dict(num_disparities=144, min_disparity=-70, texture_threshold=0)
_S64_KW = dict(num_disparities=272, min_disparity=-100, texture_threshold=0, disp12_max_diff=1)


def _pair(img, s, **kw):
    return img, (img if s == 0 else shifted(img, s)), kw


BUILDERS = {
    # every cost 0: all 144 disparities tie across three slots, the winner is k = 0 everywhere, the subpixel denominator is 0
    "const": lambda: _pair(_const(), 0, **_CONST_KW, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=0),
    # thresh = 0 and every other cost is 0: `<=` cuts every pixel, `<` none
    "const_uniq": lambda: _pair(_const(), 0, **_CONST_KW, texture_threshold=0, uniqueness_ratio=5),
    # texture sum 0 against threshold 1
    "const_tex": lambda: _pair(_const(), 0, **_CONST_KW, texture_threshold=1),
    # exact ties every 8 disparities, across lanes and slots: the lowest k must win
    "stripes8": lambda: _pair(_stripes("stripes8", 40, 300, 8), 0, **_S8_KW, uniqueness_ratio=0, disp12_max_diff=0),
    "stripes8_uniq": lambda: _pair(_stripes("stripes8", 40, 300, 8), 0, **_S8_KW, uniqueness_ratio=1),
    # ties exactly 64 apart (one lane, different slots), KPL = 8 with three dead slots, equal costs on one column of the left-right check
    "stripes64": lambda: _pair(_stripes("stripes64", 40, 400, 64), 5, **_S64_KW, uniqueness_ratio=0),
    # the same with noise in [-2, 2]: the pre-filter's cap swallows the noise on the steep edges and keeps it elsewhere
    "stripes64_noise": lambda: _pair(_stripes("stripes64_noise", 40, 400, 64, noise=2), 5, **_S64_KW, uniqueness_ratio=15),
    # the same stripes with noise drawn apart for the two sides: no cost is 0, near-ties on both sides of a threshold above 0
    "stripes64_noise2": _stripes64_noise2,
    # the texture rule cuts about a third and leaves the rest
    "half_flat": lambda: _pair(_half_flat(), 6, num_disparities=64, min_disparity=0, pre_filter_cap=31, texture_threshold=507,
                               uniqueness_ratio=10),
    # pre_filter_cap = 1, computed
    "cap1": lambda: _pair(_noise("cap1", 24, 80), 3, num_disparities=16, min_disparity=0, pre_filter_cap=1, texture_threshold=0,
                          disp12_max_diff=0),
    # GMS_STEREO_BM_MAX_WIDTH: the whole LDS row of the validate kernel
    "widest": lambda: _pair(_noise("widest", 12, R.MAX_WIDTH), 3, num_disparities=16, min_disparity=0, texture_threshold=0),
    # the largest dynamic LDS request of the match kernel, (32 + 50) (128 + 100 + 511) = 60 598 bytes: lofs = 511; lofs = 11; rofs = 9
    "largest_lds": lambda: _largest_lds(0, 7),
    "largest_lds_rofs": lambda: _largest_lds(-500, 7),
    "largest_lds_rofs9": lambda: _largest_lds(-520, -20),
}
for _nd in ENDS:
    BUILDERS[f"end_last_{_nd}"] = functools.partial(_end, _nd, False)
    BUILDERS[f"end_first_{_nd}"] = functools.partial(_end, _nd, True)
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(left, right, params) of a named case; the arrays are read-only."""
    left, right, kw = BUILDERS[name]()
    for a in (left, right):
        a.setflags(write=False)
    return left, right, kw


@functools.lru_cache(maxsize=None)
def expected(name):
    """The statement's (disp int16, cost int32) of a named case, computed once per session; read-only."""
    left, right, kw = case(name)
    d, c = R.stereo_bm(left, right, **kw)
    d.setflags(write=False)
    c.setflags(write=False)
    return d, c


def census(left, right, **kw):
    """How often each rule decides, over the computed region (the rows [w2, H - w2) and columns lofs + [0, wx)), from the statement's
    own pieces. `accepted` pixels pass the texture and the uniqueness rule."""
    p, left, right, H, W = R._prepare(left, right, kw)
    nd = p["num_disparities"]
    inv = R.filtered_value(p)
    disp, cost, dec = R.raw_maps(left, right, p)
    if dec is None:
        return dict(computed=0, valid=0)
    sad, mind = dec["sad"], dec["mind"]
    at_min = sad == dec["minsad"][None]
    slot = np.arange(nd)[:, None, None] >> 6
    accepted = dec["tex_ok"] & dec["uniq_ok"]
    out = dict(computed=int(mind.size),
               tied=int((at_min.sum(axis=0) > 1).sum()),
               tied_across_slots=int((at_min & (slot != (mind >> 6)[None])).any(axis=0).sum()),
               texture_cut=int((~dec["tex_ok"]).sum()),
               uniqueness_cut=int((dec["tex_ok"] & ~dec["uniq_ok"]).sum()),
               accepted=int(accepted.sum()),
               winner_first=int((accepted & (mind == 0)).sum()),
               winner_last=int((accepted & (mind == nd - 1)).sum()),
               denominator_zero=int((accepted & (dec["den"] == 0)).sum()),
               lr_removed=0, lr_contended=0)
    if p["disp12_max_diff"] >= 0:
        src = R.lr_sources(disp, cost, p)
        if src is not None:
            ys, x, d, c, x2 = src
            g = ys * W + x2
            lowest = np.full(H * W, np.iinfo(np.int64).max)
            np.minimum.at(lowest, g, c)
            out["lr_contended"] = int((np.bincount(g[c == lowest[g]], minlength=H * W) > 1).sum())
        checked = disp.copy()
        R.validate(checked, cost, p)
        out["lr_removed"] = int(((disp != inv) & (checked == inv)).sum())
        disp = checked
    R.roi_fill(disp, p, R.ranges(p, W)[0])
    out["valid"] = int((disp != inv).sum())
    return out


def cut_down(name):
    """About 14 x 40 with 16 disparities: what the literal loop can still walk, for the two forms of the statement to agree on."""
    z = np.full((14, 40), 90, np.uint8)
    if name == "const":
        return z, z, dict(num_disparities=16, min_disparity=-4, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=0)
    if name == "const_uniq":
        return z, z, dict(num_disparities=16, min_disparity=-4, texture_threshold=0, uniqueness_ratio=5)
    if name == "stripes8":
        s = _stripes("stripes8_small", 14, 40, 4)
        return s, s, dict(num_disparities=16, min_disparity=-4, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=0)
    if name == "stripes64":
        s = _stripes("s3", 14, 44, 8)     # a draw with contended target columns, found by a search on the CPU
        return s, shifted(s, 2), dict(num_disparities=16, min_disparity=-10, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=1)
    if name == "stripes64_noise":
        s = _stripes("stripes64_noise_small", 14, 44, 8, noise=2)
        return s, shifted(s, 2), dict(num_disparities=16, min_disparity=-6, texture_threshold=0, uniqueness_ratio=15, disp12_max_diff=1)
    if name == "cap1":
        s = _noise("cap1_small", 14, 40)
        return s, shifted(s, 3), dict(num_disparities=16, min_disparity=0, pre_filter_cap=1, texture_threshold=0, disp12_max_diff=0)
    raise KeyError(name)


CUT_DOWN = ("const", "const_uniq", "stripes8", "stripes64", "stripes64_noise", "cap1")
