"""The named cases of the speckle filter's tests (tests/test_speckle_ref.py on the CPU, tests/test_gpu_speckle.py on the GPU). A case
is a dict: name, disp (int16 [H, W], read-only), new_val, and runs: (max_speckle_size, max_diff, removed) with the number of pixels
the run changes as the case's construction gives it (None: only the two statements say). Sizes are 131 x 67 unless a name says
otherwise: 3 x 3 tiles of the kernels' 64 x 32."""
import functools
import struct

import numpy as np

W, H = 131, 67
NV = -16     # the matchers' FILTERED code at min_disparity 0


def _case(name, disp, runs, new_val=NV):
    disp = np.ascontiguousarray(disp, dtype=np.int16)
    disp.setflags(write=False)
    return dict(name=name, disp=disp, new_val=new_val, runs=tuple(runs))


def plus_on_lattice(w=W, h=H):
    """A 13-pixel plus (arm 3) centred on every lattice point (16 i, 16 j) at which it fits: every power-of-two tile corner and
    seam inside the map is straddled. At 135 x 71 the lattice reaches (128, 64)."""
    d = np.full((h, w), NV, np.int16)
    n = 0
    for cy in range(16, h - 3, 16):
        for cx in range(16, w - 3, 16):
            d[cy, cx - 3:cx + 4] = 200
            d[cy - 3:cy + 4, cx] = 200
            n += 1
    assert n == ((w - 4) // 16) * ((h - 4) // 16) and int((d != NV).sum()) == 13 * n
    return _case(f"plus_on_lattice_{w}x{h}", d, [(13, 0, 13 * n), (12, 0, 0)])


def serpentine(w, h):
    """A one-pixel-wide snake through the whole map: the even rows, joined alternately at the right and the left end."""
    d = np.full((h, w), NV, np.int16)
    d[0::2, :] = 50
    d[1::4, w - 1] = 50
    d[3::4, 0] = 50
    length = int((d != NV).sum())
    assert length == ((h + 1) // 2) * w + h // 2
    return _case(f"serpentine_{w}x{h}", d, [(length, 0, length), (length - 1, 0, 0)])


def constant():
    return _case("constant", np.full((H, W), 7, np.int16), [(W * H - 1, 0, 0), (W * H, 0, W * H)])


def singletons():
    y, x = np.mgrid[0:H, 0:W]
    return _case("singletons", ((x + y) & 1) * 100, [(1, 99, W * H), (0, 99, 0)])


def ramp_exact():
    """Horizontal neighbours differ by exactly max_diff = 5, vertical ones by 6: every row is one component of W pixels."""
    y, x = np.mgrid[0:H, 0:W]
    return _case("ramp_exact", 6 * y + 5 * x, [(W, 5, W * H), (W - 1, 5, 0)])


def ramp_one_more():
    """Steps of max_diff + 1: no links at all at max_diff 5 (at 6 the rows are linked again)."""
    y, x = np.mgrid[0:H, 0:W]
    return _case("ramp_one_more", 7 * y + 6 * x, [(1, 5, W * H), (0, 5, 0), (W - 1, 6, 0)])


def extremes():
    """32767 beside -32768 everywhere: linked at max_diff 65535 and 2^31 - 1, not at 65534."""
    y, x = np.mgrid[0:H, 0:W]
    d = np.where((x + y) & 1, 32767, -32768)
    n = W * H
    return _case("extremes", d, [(n, 65535, n), (n - 1, 65535, 0), (1, 65534, n), (0, 65534, 0), (n - 1, 2 ** 31 - 1, 0), (n, 2 ** 31 - 1, n)],
                 new_val=0)


def diagonal_only():
    """Two pairs of 5 x 5 blobs that touch at a corner only, one pair across the tile corner (64, 32): four components of 25."""
    d = np.full((H, W), NV, np.int16)
    for y0, x0 in ((10, 10), (27, 59)):
        d[y0:y0 + 5, x0:x0 + 5] = 300
        d[y0 + 5:y0 + 10, x0 + 5:x0 + 10] = 300
    return _case("diagonal_only", d, [(25, 0, 100), (24, 0, 0), (49, 0, 100)])


def new_val_inside():
    """A 20 x 30 blob of -15 cut by a column of new_val = -16 into 280 and 300 pixels (the cut lies on the tile seam x = 64), and a
    3 x 3 ring around one new_val pixel whose -15 half and -17 half link to each other at max_diff 2 but not through the centre."""
    d = np.full((H, W), NV, np.int16)
    d[20:40, 50:80] = -15
    d[20:40, 64] = NV
    d[49:52, 99], d[49, 100] = -15, -15
    d[49:52, 101], d[51, 100] = -17, -17
    assert d[50, 100] == NV
    return _case("new_val_inside", d, [(8, 2, 8), (7, 2, 0), (279, 2, 8), (280, 2, 288), (300, 2, 588), (4, 1, 8), (3, 1, 0)])


def random_map(seed, w, h):
    """A smooth ramp, +-3 noise, a quarter new_val, a tenth offset by 400."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = 300 + 2 * x + 3 * y + rng.integers(-3, 4, (h, w))
    d = np.where(rng.random((h, w)) < 0.1, d + 400, d)
    d = np.where(rng.random((h, w)) < 0.25, NV, d)
    return d.astype(np.int16)


def random_blobs(w, h):
    return _case(f"random_blobs_{w}x{h}", random_map(1000 + w, w, h), [(20, 16, None), (200, 0, None)])


def thin(w, h):
    return _case(f"thin_{w}x{h}", random_map(2000 + w + h, w, h), [(20, 16, None), (2, 3, None)])


@functools.lru_cache(maxsize=None)
def all_cases():
    return (plus_on_lattice(), plus_on_lattice(135, 71), serpentine(70, 40), serpentine(259, 131), constant(), singletons(), ramp_exact(),
            ramp_one_more(), extremes(), diagonal_only(), new_val_inside(), thin(1, 1), thin(1, 300), thin(300, 1), thin(8192, 1),
            random_blobs(131, 67), random_blobs(259, 131))


@functools.lru_cache(maxsize=None)
def expected(name, run):
    """The `literal` statement's (map, removed) of a run of a named case, computed once per session; read-only."""
    import speckle_ref
    case = next(c for c in all_cases() if c["name"] == name)
    size, diff, _ = case["runs"][run]
    out, removed = speckle_ref.literal(case["disp"], case["new_val"], size, diff)
    out.setflags(write=False)
    return out, removed


def case_bytes(disp, new_val, max_speckle_size, max_diff):
    """What tests/cpp/speckle_host.cpp reads: int32 width, height, new_val, max_speckle_size, max_diff, then the int16 map."""
    h, w = disp.shape
    return struct.pack("<5i", w, h, new_val, max_speckle_size, max_diff) + np.ascontiguousarray(disp, dtype="<i2").tobytes()


def result_bytes(out, removed):
    """What it writes: int32 removed, then the int16 map."""
    return struct.pack("<i", removed) + np.ascontiguousarray(out, dtype="<i2").tobytes()
