"""CPU: the statements behind pipeline.run_images / structureFromMotion (tests/sfm_images_ref.py) on the committed SfM photographs
(tests/golden/image_sfm_pair_1008x756.npz: PikaBun1 / PikaBun4 of the reference's SourceImages, grey, halved; a stated camera) -- the
reference's structureFromMotion with algo 2 (SfMUtil.cpp:4-83) from real pixels, at 4000 keypoints; and the two definitions the new
device entry points are compared with, the grey formula and the pack rule. tests/test_gpu_sfm_images.py holds the GPU to all of it."""
import importlib
import os

import numpy as np
import pytest

import sfm_images_ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "image_sfm_pair_1008x756.npz")
MAX_KP = 4000


@pytest.fixture(scope="module")
def pair():
    z = np.load(GOLDEN)
    return {k: np.ascontiguousarray(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def chain(oracle, pair):
    return sfm_images_ref.chain(oracle, pair["left"], pair["right"], tuple(pair["camera"]), MAX_KP)


def test_fixture_is_what_its_maker_states(pair):
    assert pair["left"].shape == pair["right"].shape == (756, 1008) and pair["left"].dtype == np.uint8
    assert pair["bgr_crop"].shape == (64, 96, 3) and pair["bgr_crop"].dtype == np.uint8
    assert pair["camera"].tolist() == [800.0, 800.0, 504.0, 378.0]
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_photographs_to_a_pose_on_the_cpu(pair, chain):
    """The five assertions of sfm_images_ref.pose_checks on the CPU chain; measured here: 4000 / 4000 keypoints, 2659 survivors, 1656
    RANSAC inliers, 1641 after recoverPose, none behind a camera, 0.402 px."""
    tv = chain["two_view"]
    assert tv["E"] is not None
    n_pose = int((tv["mask"] != 0).sum())
    rms = sfm_images_ref.pose_checks(len(chain["keypoints"][0]), len(chain["keypoints"][1]), len(chain["survivors"]), n_pose, tv["behind"],
                                     tv["sum_sq_err1"], tv["sum_sq_err2"], pair["camera"])
    assert len(chain["matches"]) == len(chain["keypoints"][0]) and len(tv["points"]) == n_pose == tv["n_pose"]
    assert abs(np.linalg.norm(tv["t"]) - 1) < 1e-9 and abs(np.linalg.det(tv["R"]) - 1) < 1e-9
    print(f"survivors {len(chain['survivors'])}, ransac {tv['n_ransac']}, pose {n_pose}, rms {rms:.4f} px, t {tv['t']}")


def test_grey_formula_on_the_colour_crop(pair):
    """grey = (299 R + 587 G + 114 B + 500) // 1000 on B, G, R bytes: the maker's formula (which reads R, G, B) on the crop, the
    extremes, and never more than one level from the real-valued weights."""
    crop = pair["bgr_crop"]
    got = sfm_images_ref.grey(crop)
    rgb = crop[..., ::-1].astype(np.int64)
    assert np.array_equal(got, ((299 * rgb[..., 0] + 587 * rgb[..., 1] + 114 * rgb[..., 2] + 500) // 1000).astype(np.uint8))
    assert got.shape == (64, 96) and got.std() > 1        # (a piece with something on it)
    exact = 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]
    assert np.abs(got - exact).max() <= 0.5 + 1e-9
    assert sfm_images_ref.grey(np.full((2, 2, 3), 255, np.uint8)).tolist() == [[255, 255], [255, 255]]
    assert sfm_images_ref.grey(np.zeros((1, 1, 3), np.uint8)).tolist() == [[0]]
    assert sfm_images_ref.grey(np.array([[[255, 0, 0]]], np.uint8)).tolist() == [[29]]     # blue alone: 114 * 255 / 1000 = 29.07


def test_pack_rule_is_concat_frames():
    """frame_off[i + 1] = frame_off[i] + min(counts[i], max_keypoints), element j of image i at frame_off[i] + j: what types.concat_frames
    makes of the per-image lists -- with an empty image, a count above the cap and one image alone."""
    types = importlib.import_module("sfm-gms_amd.types")
    rng = np.random.default_rng(3)
    for counts, cap in (([5, 0, 9, 7], 7), ([0, 0], 4), ([3], 3), ([6], 2)):
        n = len(counts)
        kp = rng.integers(0, 2**31, (n, cap, 7)).astype(np.int32).view(types.KEYPOINT_DTYPE).reshape(n, cap)
        rows = rng.integers(0, 256, (n, cap, 32)).astype(np.uint8)
        got_kp, got_rows, off = sfm_images_ref.pack(kp, rows, counts, cap)
        lists = [kp[i, :min(c, cap)] for i, c in enumerate(counts)]
        want_kp, want_off = types.concat_frames(lists)
        assert got_kp.tobytes() == want_kp.tobytes() and np.array_equal(off, want_off) and off.dtype == np.int64
        assert got_rows.tobytes() == b"".join(rows[i, :min(c, cap)].tobytes() for i, c in enumerate(counts))


def test_argument_checks_need_no_device(pkg, pair):
    """structureFromMotion and run_images refuse a wrong channel count, mixed sizes, a bad method and images that are not 8-bit before
    they touch a device (there is none here, and run_images gets no context)."""
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    left, right, cam = pair["left"], pair["right"], tuple(pair["camera"])
    for a, b, kw in ((np.zeros((64, 64, 4), np.uint8),) * 2 + ({},), (left, right[:, :-1], {}), (left, np.stack([right] * 3, axis=2), {}),
                     (left, right, {"method": "sift"})):
        with pytest.raises(ValueError):
            pkg.structureFromMotion(a, b, cam, **kw)
    for images, kw in ((np.zeros((2, 64, 64, 2), np.uint8), {}), ([left, right[:-1]], {}), (np.stack([left, right]), {"method": "orb"}),
                       (np.stack([left, right]).astype(np.float32), {}), (np.stack([left, right]), {"descriptor": "sift"})):
        with pytest.raises(ValueError):
            pipeline.run_images(None, images, **kw)
