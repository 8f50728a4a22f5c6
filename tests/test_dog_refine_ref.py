"""CPU: the DoG refinement's numpy statement (tests/dog_refine_ref.py) against the host build of the kernel's header
(sfm-gms_amd/csrc/dog_core.h through tests/cpp/dog_refine_host.cpp) on every pixel, the properties the definition implies, and what
the refinement is for: more RANSAC inliers from the same matches on the committed SfM pair."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dog_ref
import dog_refine_ref as ref
from test_dog_ref import small_images
import hostbuild as hb

SRC = "dog_refine_host.cpp"
SIZES = [(33, 33), (97, 65), (64, 48), (130, 200), (641, 479), (1030, 50)]     # (width, height): those of tests/test_gpu_dog.py
CONTRASTS = (0, 128)
SFM_PAIR = os.path.join(hb.ROOT, "tests", "golden", "image_sfm_pair_1008x756.npz")


@pytest.fixture(scope="module")
def host():
    so = hb.host_lib(SRC)
    lib = C.CDLL(so)
    lib.dog_refine_host_scale.restype = lib.dog_refine_host_coord.restype = lib.dog_refine_host_size.restype = C.c_float
    lib.dog_refine_host_scale.argtypes = [C.c_int]
    lib.dog_refine_host_coord.argtypes = [C.c_int, C.c_int, C.c_float]
    lib.dog_refine_host_size.argtypes = [C.c_int, C.c_float]
    lib.dog_refine_host_sixteenths.argtypes = [C.c_int64, C.c_int64]
    lib.dog_refine_host_floor_div_clamped.argtypes = [C.c_int64, C.c_int64, C.c_int]
    lib.dog_refine_host_pack.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.dog_refine_host_unpack.argtypes = [C.c_int, C.c_void_p]
    lib.dog_refine_host_offsets.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@functools.lru_cache(maxsize=None)
def _terms():
    """The rule's integers at every candidate of the test set (six sizes, five images, contrasts 0 and 128), from the statement alone."""
    parts = [ref.terms(img, c) for w, h in SIZES for img in small_images(w, h) for c in CONTRASTS]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def test_the_set_needs_floor_division_and_the_clamp():
    """What equal planes below can show: candidates whose truncated quotient differs from the floor, clamped positions, and a scale
    offset that reaches 8 without a clamp."""
    t = _terms()
    assert len(t["xs"]) == 7622
    num, den = 32 * t["nx"] + t["det16"], 2 * t["det16"]
    floor = num // den
    trunc = np.where(num < 0, -((-num) // den), num // den)             # C++'s quotient
    differs = (num < 0) & (trunc != floor)
    raw_x, raw_y = floor, ref.floor_sixteenths(t["ny"], t["det16"])
    clamped = (np.abs(raw_x) > 8) | (np.abs(raw_y) > 8)
    os_ = ref.floor_sixteenths(t["n"], t["q"])
    print(f"\n{len(num)} candidates: truncation changes ox on {int(differs.sum())}, {int(clamped.sum())} positions clamped, max |os| {int(np.abs(os_).max())}")
    assert differs.sum() == 3562 and clamped.sum() == 276 and np.abs(os_).max() == 8
    ns, qs = 32 * t["n"] + t["q"], 2 * t["q"]
    assert ((ns < 0) & (ns % qs != 0)).any()                             # the scale's division meets a negative, inexact quotient too


@pytest.mark.parametrize("w,h", SIZES)
def test_host_build_equals_the_statement_on_every_pixel(host, w, h):
    n = 0
    for img in small_images(w, h):
        for contrast in CONTRASTS:
            cand = dog_ref.candidates(img, contrast)
            want = ref.offsets(img, contrast, cand)
            got_cand, got = np.full((h, w), 9, dtype=np.uint8), np.full((h, w), 9, dtype=np.uint16)
            rc = host.dog_refine_host_offsets(img.ctypes.data, w, h, contrast, got_cand.ctypes.data, got.ctypes.data)
            assert rc == np.count_nonzero(cand) and np.array_equal(got_cand, cand)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, f"contrast {contrast}: {len(bad)} wrong codes, the first (y, x) = {bad[0].tolist()}: got {got[tuple(bad[0])]}, " \
                                  f"want {want[tuple(bad[0])]}"
            assert ((want > 0) == (cand > 0)).all() and want.max() <= 17 ** 3
            n += rc
    assert n > 0 or (w, h) == (33, 33)


def test_divisions_are_floor_divisions(host):
    """The header divides without a 64-bit division (an fp32 guess, one exact remainder): against numpy's //, clamped, on random
    operands up to the rule's bounds, on small ones, and on quotients at, just below and just above every integer k = -9 .. 9 with
    divisors up to 2^41 ((32 n + q) / (2 q) = k + d / (2 m) for q = 32 m, n = (2 k - 1) m + d)."""
    rng = np.random.default_rng(5)
    q = rng.integers(1, 1 << 40, 3000, dtype=np.int64)
    n = rng.integers(-(1 << 39), 1 << 39, 3000, dtype=np.int64)
    q[:400], n[:400] = rng.integers(1, 50, 400), rng.integers(-400, 400, 400)
    n[400:1400] = (q[400:1400].astype(np.float64) * rng.uniform(-0.6, 0.6, 1000)).astype(np.int64)      # quotients inside the clamp
    edge = [((2 * k - 1) * m + d, 32 * m) for k in range(-9, 10) for m in (1, 3, 1 << 20, (1 << 35) - 1, 1 << 35) for d in (-1, 0, 1)]
    n, q = np.concatenate([n, [e[0] for e in edge]]), np.concatenate([q, [e[1] for e in edge]])
    got = np.array([host.dog_refine_host_sixteenths(int(a), int(b)) for a, b in zip(n, q)])
    want = np.clip(ref.floor_sixteenths(n, q), -8, 8)
    assert np.array_equal(got, want) and (got < 0).any() and len(set(got.tolist())) == 17
    assert [host.dog_refine_host_sixteenths(a, b) for a, b in ((-1, 3), (-1, 32), (1, 32), (-3, 32), (3, 32), (-1, 1))] == [-5, 0, 1, -1, 2, -8]
    a = rng.integers(-(1 << 45), 1 << 45, 2000, dtype=np.int64)
    b = rng.integers(1, 1 << 41, 2000, dtype=np.int64)
    b[:1000] = np.maximum(np.abs(a[:1000]) // rng.integers(1, 3000, 1000), 1)
    for lim in (8, 1000):
        got = np.array([host.dog_refine_host_floor_div_clamped(int(x), int(y), lim) for x, y in zip(a, b)])
        assert np.array_equal(got, np.clip(a // b, -lim, lim)) and (np.abs(got) < lim).sum() > 50


def test_scale_constants_codes_and_the_record(host):
    for i in range(17):
        assert ref.K_SCALE[i] == ref.scale_rule(i) == np.float32(host.dog_refine_host_scale(i - 8)), i
    assert ref.K_SCALE[8] == 1 and (np.diff(ref.K_SCALE) > 0).all() and ref.K_SCALE.dtype == np.float32
    assert abs(float(ref.K_SCALE[16]) / float(ref.K_SCALE[0]) - 1.2) < 1e-6          # one layer from end to end
    out = np.zeros(3, dtype=np.int32)
    seen = set()
    for os_ in range(-8, 9):
        for oy in range(-8, 9):
            for ox in (-8, -1, 0, 3, 8):
                code = host.dog_refine_host_pack(ox, oy, os_)
                assert code == ref.pack(ox, oy, os_) and 1 <= code <= 4913
                host.dog_refine_host_unpack(code, out.ctypes.data)
                assert out.tolist() == [ox, oy, os_] == [int(v) for v in ref.unpack(code)]
                seen.add(code)
    assert min(seen) == 1 and max(seen) == 4913
    # the record: all offsets zero gives the unrefined call's bytes; otherwise fp32, every operation rounded once
    rng = np.random.default_rng(6)
    half, step = np.float32(0.5), np.float32(0.0625)
    for _ in range(300):
        v, o, os_ = int(rng.integers(16, 5000)), int(rng.integers(-8, 9)), int(rng.integers(-8, 9))
        f = np.float32(1008) / np.float32(rng.integers(200, 1009))
        want = ((np.float32(v) + np.float32(o) * step) + half) * f - half
        assert np.float32(host.dog_refine_host_coord(v, o, f)) == want
        assert np.float32(host.dog_refine_host_coord(v, 0, f)) == (np.float32(v) + half) * f - half
        assert np.float32(host.dog_refine_host_size(os_, f)) == (np.float32(31.0) * f) * ref.K_SCALE[os_ + 8]
        assert np.float32(host.dog_refine_host_size(0, f)) == np.float32(31.0) * f


def _blob(cx, cy, sigma, size=65):
    """tests/test_dog_ref.py's blob() (100 grey levels on 110, bright) with a centre between pixels."""
    y, x = np.mgrid[0:size, 0:size]
    return np.rint(110 + 100 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma * sigma))).astype(np.uint8)


def test_sub_pixel_blobs_are_found_where_they_are():
    worst_int, scales = 0.0, {}
    for dx, dy in ((0, 0), (0.25, -0.375), (0.4375, 0.125), (-0.3125, 0.4375)):
        for sigma in (1.5, 1.6):
            img = _blob(32 + dx, 32 + dy, sigma)
            xs, ys, ox, oy, os_ = ref.offsets_at(img, 128)
            at = np.flatnonzero((xs == 32) & (ys == 32))
            assert len(at) == 1, (dx, dy, sigma)
            ex, ey = 32 + ox[at[0]] / 16.0 - (32 + dx), 32 + oy[at[0]] / 16.0 - (32 + dy)
            print(f"\ncentre (32 {dx:+}, 32 {dy:+}) sd {sigma}: offsets {int(ox[at[0]])} {int(oy[at[0]])} {int(os_[at[0]])} / 16, error {ex:+.4f} {ey:+.4f} px")
            assert abs(ex) <= 1 / 16 and abs(ey) <= 1 / 16
            worst_int = max(worst_int, float(np.hypot(dx, dy)))
            scales[(dx, dy, sigma)] = int(os_[at[0]])
        assert scales[(dx, dy, 1.6)] >= scales[(dx, dy, 1.5)]
    assert worst_int > 0.5                                              # what the integer position is off by


def test_refinement_changes_x_y_and_size_only(oracle):
    img = small_images(130, 200)[1]
    base = dog_ref.detect(oracle, img, 128, 37, 8)
    same = ref.detect(oracle, img, 128, 37, 8, refine=False)
    fine = ref.detect(oracle, img, 128, 37, 8)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base, same))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base[1:], fine[1:]))
    for f in ("angle", "response", "octave", "class_id"):
        assert np.array_equal(base[0][f], fine[0][f])
    assert len(fine[0]) > 0 and fine[0].tobytes() != base[0].tobytes()
    # half a level pixel at the most (the factor of level 7 is below 3.6), and a twelfth of a layer's factor 1.2 either way
    assert (np.abs(fine[0]["x"] - base[0]["x"]) <= 0.5 * 3.6 + 1e-3).all() and (np.abs(fine[0]["size"] / base[0]["size"] - 1) < 0.096).all()


def test_workspace_is_the_unrefined_one_and_a_code_plane(pkg):
    """The size functions are host arithmetic: the refined call's workspace is the DoG call's, on a 256-byte boundary, and one uint16
    plane of level 0's size per image behind it; the DoG call's own size is what the pyramid call with gradient rows needs, as before."""
    lib = pkg.load_library()
    for w, h, n, kp, levels in ((100, 100, 1, 10, 8), (33, 33, 5, 0, 1), (1920, 1080, 8, 10000, 8), (641, 479, 3, 37, 16), (1030, 50, 2, 5, 16)):
        plain = lib.gms_detect_dog_workspace_bytes(w, h, n, kp, levels)
        assert plain == lib.gms_detect_pyramid_grad_workspace_bytes(w, h, n, kp, levels) > 0
        plane = (2 * w * h * n + 255) // 256 * 256
        assert lib.gms_detect_dog_refined_workspace_bytes(w, h, n, kp, levels) == (plain + 255) // 256 * 256 + plane
    for args in ((32, 100, 1, 10, 8), (100, 32, 1, 10, 8), (100, 100, 0, 10, 8), (100, 100, 1, -1, 8), (100, 100, 1, 10, 0), (100, 100, 1, 10, 17),
                 (65536, 100, 1, 10, 8)):
        assert lib.gms_detect_dog_refined_workspace_bytes(*args) == 0 == lib.gms_detect_dog_workspace_bytes(*args)


def test_more_inliers_on_the_sfm_pair(oracle):
    """The committed SfM pair at 4000 keypoints, contrast 128, 8 levels, method gms, stated camera, deterministic: RANSAC inliers at
    0.5 px with refinement at least 1.15 x those without (measured 867 / 677), at 1.0 px not fewer (measured 1117 / 1013)."""
    z = np.load(SFM_PAIR)
    left, right = np.ascontiguousarray(z["left"], dtype=np.uint8), np.ascontiguousarray(z["right"], dtype=np.uint8)
    camera = tuple(float(v) for v in z["camera"])
    n = {}
    for refine in (False, True):
        detected = [ref.detect(oracle, img, 128, 4000, 8, refine=refine) for img in (left, right)]
        for thr in (0.5, 1.0):
            c = ref.sfm_chain(oracle, left, right, camera, 128, 4000, 8, ransac_threshold=thr, refine=refine, detected=detected)
            n[(refine, thr)] = (int(c["two_view"]["n_ransac"]), int(c["two_view"]["iters"]), len(c["survivors"]))
    print(f"\ninliers (iterations, survivors) at 0.5 px: {n[(False, 0.5)]} -> refined {n[(True, 0.5)]}; at 1.0 px: {n[(False, 1.0)]} -> refined {n[(True, 1.0)]}")
    assert n[(True, 0.5)][0] >= 1.15 * n[(False, 0.5)][0]
    assert n[(True, 1.0)][0] >= n[(False, 1.0)][0]


def test_sanitizer_run_of_the_stand_alone_program():
    exe = hb.host_exe_sanitized(SRC, defines=("DOG_REFINE_HOST_MAIN",))
    out = hb.run(exe)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("dog_refine_host: tiny ")
