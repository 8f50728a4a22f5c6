"""CPU: what the seven one-shot host entry points refuse, and with which code, before any device call -- gms_bf_match_select,
gms_bf_select_host_batch, gms_stereo_bm, gms_median_blur, gms_portrait, gms_logos_host_batch and gms_logos_dict_train (include/gms.h).
Every call here returns from its argument checks, so the module passes on a machine without a GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

NULL = None
OK, BAD_ARG, CAPACITY = 0, -1, -5


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def fake_ctx():
    """Stands in for a context where the checks behind `!c` are the subject: those checks never touch the context (zeroed memory, so
    that a call that slipped through would find an unlocked mutex and fail at its first device call instead of crashing)."""
    buf = C.create_string_buffer(1 << 16)
    return C.addressof(buf), buf


def _types():
    return importlib.import_module("sfm-gms_amd.types")


def test_bf_match_select_refusals(lib, pkg):
    d = np.zeros((4, 32), np.uint8)
    out = np.zeros(4, pkg.DMATCH_DTYPE)
    res = np.zeros(1, pkg.BF_RESULT_DTYPE)

    def call(kind=0, d1=d.ctypes.data, n1=4, d2=d.ctypes.data, n2=4, cross=1, coef=4.0, max_size=500, o=out.ctypes.data, cap=4, n_out=True):
        n = C.c_int64(77)
        res["n_out"] = 77
        rc = lib.gms_bf_match_select(kind, d1, n1, d2, n2, cross, coef, max_size, o, cap, C.byref(n) if n_out else None, res.ctypes.data)
        if n_out:
            assert n.value == 0            # cleared before the checks
        assert int(res["n_out"][0]) == 0 and int(res["status"][0]) == OK
        return rc

    assert call(n_out=False) == BAD_ARG
    assert call(n1=-1) == BAD_ARG and call(n2=-1) == BAD_ARG
    assert call(n1=(1 << 22) + 1) == BAD_ARG
    assert call(cap=-1) == BAD_ARG and call(cap=1 << 31) == BAD_ARG
    assert call(kind=2) == BAD_ARG and call(kind=-1) == BAD_ARG
    assert call(cross=2) == BAD_ARG
    for coef in (0.5, 0.999, float("nan"), float("inf")):
        assert call(coef=coef) == BAD_ARG
    assert call(max_size=-1) == BAD_ARG
    assert call(d1=NULL) == BAD_ARG and call(d2=NULL) == BAD_ARG
    assert call(o=NULL) == BAD_ARG


def test_bf_select_host_batch_refusals(lib, pkg, fake_ctx):
    ctx = fake_ctx[0]
    d = np.zeros((4, 32), np.uint8)
    off = np.array([0, 2, 4], np.int64)
    pairs = np.zeros(1, pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"], pairs["m"], pairs["match_off"] = 0, 1, 2, 0
    out = np.zeros(2, pkg.DMATCH_DTYPE)
    res = np.zeros(1, pkg.BF_RESULT_DTYPE)

    def call(c=ctx, kind=0, desc=d.ctypes.data, fo=off, nf=2, pr=pairs.ctypes.data, n_pairs=1, cross=1, coef=4.0, max_size=500,
             o=out.ctypes.data, r=res.ctypes.data):
        return lib.gms_bf_select_host_batch(c, kind, desc, None if fo is None else fo.ctypes.data, nf, pr, n_pairs, cross, coef, max_size, o, r)

    assert call(c=NULL) == BAD_ARG
    assert call(nf=-1) == BAD_ARG and call(n_pairs=-1) == BAD_ARG and call(fo=None) == BAD_ARG
    assert call(kind=2) == BAD_ARG and call(cross=-1) == BAD_ARG and call(coef=0.5) == BAD_ARG and call(max_size=-1) == BAD_ARG
    assert call(n_pairs=0) == OK                        # nothing to do -- but only behind the parameter checks:
    assert call(n_pairs=0, coef=0.5) == BAD_ARG
    assert call(pr=NULL) == BAD_ARG and call(r=NULL) == BAD_ARG
    assert call(desc=NULL) == BAD_ARG
    assert call(fo=np.array([0, 2, -1], np.int64)) == BAD_ARG      # a negative total
    assert call(fo=np.array([0, 5, 4], np.int64)) == BAD_ARG       # offsets that decrease
    assert call(fo=np.array([0, (1 << 22) + 1, (1 << 22) + 3], np.int64)) == CAPACITY
    assert call(o=NULL) == BAD_ARG                      # the pair has room for two matches and nowhere to put them


def test_stereo_bm_refusals(lib):
    t = _types()
    img = np.zeros((40, 64), np.uint8)
    d16 = np.zeros((40, 64), np.int16)

    def call(params=NULL, left=img.ctypes.data, right=img.ctypes.data, w=64, h=40, pitch=64):
        return lib.gms_stereo_bm(params, left, right, w, h, pitch, d16.ctypes.data, NULL, NULL)

    assert call(pitch=63) == BAD_ARG
    assert call(w=-64) == BAD_ARG and call(h=-40) == BAD_ARG and call(w=0) == BAD_ARG
    assert call(left=NULL) == BAD_ARG and call(right=NULL) == BAD_ARG
    for kw in (dict(block_size=6), dict(block_size=41), dict(num_disparities=24), dict(pre_filter_cap=0), dict(speckle_window_size=100)):
        rec = t.stereo_bm_params(kw)
        assert call(params=rec.ctypes.data) == BAD_ARG, kw


def test_median_blur_and_portrait_refusals(lib):
    t = _types()
    img = np.zeros((20, 30, 3), np.uint8)
    disp = np.zeros((20, 30), np.uint8)
    dst = np.zeros_like(img)
    src_p, dst_p = img.ctypes.data, dst.ctypes.data
    for ksize in (2, 4, 16, 1, 33, -3):
        assert lib.gms_median_blur(src_p, 30, 20, 3, ksize, dst_p) == BAD_ARG
    assert lib.gms_median_blur(src_p, -30, 20, 3, 5, dst_p) == BAD_ARG
    assert lib.gms_median_blur(src_p, 30, 0, 3, 5, dst_p) == BAD_ARG
    assert lib.gms_median_blur(src_p, 30, 20, 2, 5, dst_p) == BAD_ARG
    assert lib.gms_median_blur(NULL, 30, 20, 3, 5, dst_p) == BAD_ARG
    assert lib.gms_median_blur(src_p, 30, 20, 3, 5, NULL) == BAD_ARG

    def portrait(params=NULL, bgr=src_p, d=disp.ctypes.data, w=30, h=20, out=dst_p):
        return lib.gms_portrait(params, bgr, d, w, h, out, NULL, NULL, NULL)

    assert portrait(w=-30) == BAD_ARG and portrait(h=0) == BAD_ARG and portrait(w=8193) == BAD_ARG
    assert portrait(bgr=NULL) == BAD_ARG and portrait(d=NULL) == BAD_ARG and portrait(out=NULL) == BAD_ARG
    for kw in (dict(median_ksize=14), dict(median_ksize=33), dict(threshold=256), dict(dilate_iterations=9), dict(num_contours=0)):
        rec = t.portrait_params(kw)
        assert portrait(params=rec.ctypes.data) == BAD_ARG, kw


def test_logos_host_batch_refusals(lib, pkg, fake_ctx):
    ctx = fake_ctx[0]
    kp = np.zeros(4, pkg.KEYPOINT_DTYPE)
    off = np.array([0, 2, 4], np.int64)
    words = np.zeros(4, np.int32)
    pairs = np.zeros(1, pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"], pairs["m"], pairs["match_off"] = 0, 1, 2, 0
    out = np.zeros(2, pkg.DMATCH_DTYPE)
    res = np.zeros(1, pkg.LOGOS_RESULT_DTYPE)

    def call(c=ctx, k=kp.ctypes.data, fo=off, nf=2, w=words.ctypes.data, n_words=50, pr=pairs.ctypes.data, n_pairs=1, o=out.ctypes.data,
             r=res.ctypes.data):
        return lib.gms_logos_host_batch(c, k, None if fo is None else fo.ctypes.data, nf, w, n_words, pr, n_pairs, o, r)

    assert call(c=NULL) == BAD_ARG
    assert call(nf=-1) == BAD_ARG and call(n_pairs=-1) == BAD_ARG and call(fo=None) == BAD_ARG
    for n_words in (0, -1, 65536):
        assert call(n_words=n_words) == BAD_ARG
    assert call(n_pairs=0) == OK and call(n_pairs=0, n_words=0) == BAD_ARG
    assert call(pr=NULL) == BAD_ARG and call(r=NULL) == BAD_ARG
    assert call(k=NULL) == BAD_ARG and call(w=NULL) == BAD_ARG
    assert call(fo=np.array([0, 2, -1], np.int64)) == BAD_ARG
    assert call(fo=np.array([0, 2, 1 << 31], np.int64)) == BAD_ARG   # more keypoints than an int32 indexes
    assert call(fo=np.array([0, 5, 4], np.int64)) == BAD_ARG
    assert call(o=NULL) == BAD_ARG


def test_logos_dict_train_refusals(lib, pkg):
    rows = np.zeros((8, 32), np.uint8)
    off = np.array([0, 8], np.int64)
    dic = np.zeros((4, 32), np.uint8)
    rec = np.zeros(1, pkg.LOGOS_DICT_RESULT_DTYPE)

    def call(kind=0, desc=rows.ctypes.data, so=off, n_sets=1, n_words=4, attempts=3, max_iters=10, d=dic.ctypes.data, r=rec.ctypes.data):
        return lib.gms_logos_dict_train(kind, desc, None if so is None else so.ctypes.data, n_sets, n_words, attempts, max_iters, 0, d, r, NULL)

    assert call(n_sets=-1) == BAD_ARG and call(so=None) == BAD_ARG
    assert call(kind=2) == BAD_ARG and call(kind=-1) == BAD_ARG
    for n_words in (0, -4, 65536):
        assert call(n_words=n_words) == BAD_ARG
    assert call(attempts=0) == BAD_ARG and call(attempts=17) == BAD_ARG
    assert call(max_iters=0) == BAD_ARG and call(max_iters=1001) == BAD_ARG
    assert call(so=np.array([0, -8], np.int64)) == BAD_ARG          # a negative total
    assert call(so=np.array([0], np.int64), n_sets=0) == OK         # no sets: nothing to do -- behind the parameter checks:
    assert call(so=np.array([0], np.int64), n_sets=0, n_words=0) == BAD_ARG
    assert call(d=NULL) == BAD_ARG and call(r=NULL) == BAD_ARG and call(desc=NULL) == BAD_ARG
