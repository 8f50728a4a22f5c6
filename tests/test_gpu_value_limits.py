"""-m gpu: the image kernels of the keypoint source (detect_kernels.hip, grad_desc_kernels.hip, dog_kernels.hip) at the
ends of their value range, on the constructed images of tests/value_limit_cases.py, byte for byte against the statements the other GPU
tests use (oracle/detect_ref.c, tests/pyramid_ref.py, grad_desc_ref.py, dog_ref.py, dog_refine_ref.py). What the images reach is
asserted on the CPU in tests/test_value_limit_cases.py: FAST score 255 with a quota inside its tie; accumulators past 2^23, rows with
a 255, all-zero rows, the smallest n' and all 32 direction bins in the gradient descriptor, with refused keypoints at every position
of a workgroup; the DoG contrast on a candidate's own |D_1|; refinement terms past those of the noise and block images."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dog_ref  # noqa: E402
import dog_refine_ref  # noqa: E402
import grad_desc_ref  # noqa: E402
import value_limit_cases as vc  # noqa: E402

pytestmark = pytest.mark.gpu


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def _oracle():
    import gms_oracle
    gms_oracle.load()
    return gms_oracle


# ---- FAST, single scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", vc.DOTS_SIZES)
def test_fast_dots_of_score_255(ctx, oracle, w, h):
    """Every dot scores 255: the uint8 score at its top, histogram bin 255, det_cut_kernel at s = 255, and quotas of 7 and 1 that cut
    inside the tie there (det_rows_kernel, det_emit_kernel keep the first in raster order). Threshold 0 adds the weaker corners."""
    imgs = vc.dots_batch(w, h)
    for threshold, max_kp in ((254, 10000), (254, 7), (0, 10000), (254, 1)):
        kps, rows = _batch().detect_images(ctx, imgs, threshold, max_kp)
        for i, img in enumerate(imgs):
            want_kp, want_rows = oracle.detect(img, threshold, max_kp)
            assert len(want_kp) > 0 and (threshold != 254 or (want_kp["response"] == 255).all())
            assert len(kps[i]) == len(want_kp), (threshold, max_kp, i)
            assert kps[i].tobytes() == want_kp.tobytes() and rows[i].tobytes() == want_rows.tobytes(), (threshold, max_kp, i)


# ---- FAST, pyramid, both descriptors ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_fast(threshold, max_kp, n_levels):
    return [grad_desc_ref.detect(_oracle(), img, threshold, max_kp, n_levels) for img in vc.mosaic_batch()]


@pytest.mark.parametrize("threshold,max_kp,n_levels", [(20, 10000, 8), (254, 10000, 8), (254, 37, 8), (0, 5, 16)])
def test_fast_pyramid_on_the_mosaic(ctx, threshold, max_kp, n_levels):
    """The kFromLevel form of both describe kernels on all 32 direction bins and on score 255; (254, 37, 8) cuts inside the tie at 255."""
    imgs = vc.mosaic_batch()
    kps, rows32, rows128, lc = _batch().detect_images_pyramid(ctx, imgs, threshold, max_kp, n_levels, descriptor="both")
    want = _want_fast(threshold, max_kp, n_levels)
    assert lc.shape == (len(imgs), n_levels)
    for i in range(len(imgs)):
        want_kp, want_rows32, want_lc, want_rows128 = want[i]
        assert len(want_kp) > 0 and lc[i].tolist() == want_lc.tolist(), i
        assert kps[i].tobytes() == want_kp.tobytes(), i
        assert rows32[i].tobytes() == want_rows32.tobytes(), i
        assert rows128[i].dtype == np.float32 and rows128[i].shape == (len(want_kp), 128)
        assert rows128[i].tobytes() == want_rows128.tobytes(), i
    if threshold == 254:
        assert all((k["response"] == 255).all() for k in kps)


# ---- compute() at the mosaic's centres -----------------------------------------------------------------------------------------------------
def test_describe_grad_at_the_centres_with_refused_records_between(ctx, pkg):
    """grad_describe_kernel<kAtRecords>: the LDS atomics past 2^23, both 64-bit wave reductions, isqrt64, the n / 5 clip, the
    min(255, ...) cut and the n' = 0 branch on the device; a refused record at every position of a four-wave workgroup beside active
    ones (inactive waves still reach both barriers), and a last workgroup of two."""
    batch = _batch()
    m = vc.mosaic()
    mixed, refused = vc.mixed_records(pkg.KEYPOINT_DTYPE)
    want_status, want_kp, want_rows = grad_desc_ref.describe(m, mixed)
    assert want_status == 1 and len(mixed) % 4 != 0 and np.array_equal(np.isnan(want_rows[:, 0]), refused)
    status, got_kp, got_rows = batch.describe_image(ctx, m, mixed, descriptor="grad", fill=-7.0)
    assert status == 1 and got_kp.tobytes() == want_kp.tobytes()
    assert (got_rows[refused] == -7.0).all()
    assert got_rows[~refused].tobytes() == want_rows[~refused].tobytes()
    assert (got_rows[~refused] == 255).any() and (~got_rows[~refused].any(axis=1)).sum() >= 2          # the cut at 255; n' = 0
    centres = vc.centre_records(pkg.KEYPOINT_DTYPE)
    want_status, want_kp, want_rows = grad_desc_ref.describe(m, centres)
    status, got_kp, got_rows = batch.describe_image(ctx, m, centres, descriptor="grad", fill=-7.0)
    assert want_status == 0 and status == 0 and got_kp.tobytes() == want_kp.tobytes() and got_rows.tobytes() == want_rows.tobytes()
    assert sorted(set(np.rint(got_kp["angle"] / np.float32(11.25)).astype(int).tolist())) == list(range(32))


def test_describe_brief_at_the_centres_with_refused_records_between(ctx, pkg, oracle):
    batch = _batch()
    m = vc.mosaic()
    mixed, refused = vc.mixed_records(pkg.KEYPOINT_DTYPE)
    centres = vc.centre_records(pkg.KEYPOINT_DTYPE)
    rc, want_kp, want_rows = oracle.describe(m, mixed[~refused])
    assert rc == len(mixed) - refused.sum() and oracle.describe(m, mixed)[0] == -1
    status, got_kp, got_rows = batch.describe_image(ctx, m, mixed, fill=0xA5)
    assert status == 1 and got_kp[refused].tobytes() == mixed[refused].tobytes() and (got_rows[refused] == 0xA5).all()
    assert got_kp[~refused].tobytes() == want_kp.tobytes() and got_rows[~refused].tobytes() == want_rows.tobytes()
    rc, want_kp, want_rows = oracle.describe(m, centres)
    status, got_kp, got_rows = batch.describe_image(ctx, m, centres, fill=0xA5)
    assert rc == 48 and status == 0 and got_kp.tobytes() == want_kp.tobytes() and got_rows.tobytes() == want_rows.tobytes()
    assert got_kp.tobytes() == batch.describe_image(ctx, m, centres, descriptor="grad")[1].tobytes()          # the same directions


# ---- DoG ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosaic", "discs"])
def test_dog_planes_with_the_contrast_on_a_candidates_own_value(ctx, name):
    """|c| > contrast decided at equality: contrasts c* and c* - 1 for the weakest and the strongest level-0 candidate of the image,
    beside 0 and 65535; candidate and code planes on every pixel of the image, of 255 - image and (the mosaic) of its upside-down copy."""
    batch = _batch()
    imgs = {"mosaic": vc.mosaic_batch, "discs": vc.discs_batch}[name]()
    for which, (c, x, y) in vc.own_contrasts(name).items():                     # the planes must differ where the equality is
        assert batch.dog_candidates(ctx, imgs[:1], c - 1)[0, y, x] > 0 and batch.dog_candidates(ctx, imgs[:1], c)[0, y, x] == 0, which
    for c in vc.contrast_set(name):
        want_cand = np.stack([dog_ref.candidates(img, c) for img in imgs])
        want_codes = np.stack([dog_refine_ref.offsets(img, c, cand) for img, cand in zip(imgs, want_cand)])
        for got, want, dtype in ((batch.dog_candidates(ctx, imgs, c), want_cand, np.uint8), (batch.dog_offsets(ctx, imgs, c), want_codes, np.uint16)):
            assert got.dtype == dtype and got.shape == want.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, f"contrast {c}: {len(bad)} wrong pixels, the first (image, y, x) = {bad[0].tolist()}: " \
                                  f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@functools.lru_cache(maxsize=None)
def _dog_planes():
    out = []
    for img in vc.mosaic_batch():
        cand = dog_ref.level_candidates(img, 128, 8)
        out.append((cand, dog_refine_ref.level_offsets(img, 128, 8, cand)))
    return out


@functools.lru_cache(maxsize=None)
def _want_dog(max_kp, refine):
    return [dog_refine_ref.detect(_oracle(), img, 128, max_kp, 8, cand, refine, codes) for img, (cand, codes) in zip(vc.mosaic_batch(), _dog_planes())]


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("max_kp", [10000, 37])
def test_dog_pyramid_on_the_mosaic(ctx, max_kp, refine):
    imgs = vc.mosaic_batch()
    kps, rows32, rows128, lc = _batch().detect_images_pyramid(ctx, imgs, 20, max_kp, 8, descriptor="both", detector="dog", contrast=128, refine=refine)
    want = _want_dog(max_kp, refine)
    for i in range(len(imgs)):
        want_kp, want_rows32, want_lc, want_rows128 = want[i]
        assert len(want_kp) > 0 and lc[i].tolist() == want_lc.tolist(), i
        assert kps[i].tobytes() == want_kp.tobytes(), i
        assert rows32[i].tobytes() == want_rows32.tobytes() and rows128[i].tobytes() == want_rows128.tobytes(), i
    if refine:
        plain = _want_dog(max_kp, False)
        assert any((k["x"] != p[0]["x"]).any() for k, p in zip(kps, plain))


def test_refined_dog_graph_replay_on_the_inverted_mosaic(ctx):
    import torch
    batch = _batch()
    first, second = vc.mosaic_batch()[:1], vc.mosaic_batch()[2:]
    want = {0: _want_dog(10000, True)[:1], 1: _want_dog(10000, True)[2:]}
    d_imgs = torch.from_numpy(np.ascontiguousarray(first)).cuda()
    run = batch.DetectPyramid(ctx, 1, vc.MOSAIC_W, vc.MOSAIC_H, 20, 10000, 8, descriptor="both", detector="dog", contrast=128, refine=True)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.stream(stream):
            run.run(d_imgs)                                   # warm-up
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            run.run(d_imgs)
        for which, imgs in ((1, second), (0, first)):
            d_imgs.copy_(torch.from_numpy(np.ascontiguousarray(imgs)))
            for t in (run.d_kp, run.d_desc, run.d_counts, run.d_level_counts, run.d_rows128):
                t.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            kps, rows32, rows128, lc = run.results()
            want_kp, want_rows32, want_lc, want_rows128 = want[which][0]
            assert kps[0].tobytes() == want_kp.tobytes() and rows32[0].tobytes() == want_rows32.tobytes()
            assert lc[0].tolist() == want_lc.tolist() and rows128[0].tobytes() == want_rows128.tobytes() and rows128[0].any()
    finally:
        ctx.set_stream(None)
        torch.cuda.synchronize()
        g.reset()
