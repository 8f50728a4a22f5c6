"""-m gpu: pipeline.run_main_scenarios -- the three scenarios of the reference's main() (main.cpp:28-47) from two photographs, the
right image turned and resized on the device -- on tests/golden/image_sfm_pair_1008x756.npz at 4000 keypoints and a 500 x 500 resize:
the transformed images against tests/warp_ref.py, the equally sized scenarios against run_images on [left, transformed right], the
resized scenario against the host-list route (detect_images_pyramid per image -> FrameTable / DescriptorTable -> match_pairs ->
filter_pairs), and the rotation hypothesis the filter picks against that route's."""
import importlib
import os

import numpy as np
import pytest

import warp_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "image_sfm_pair_1008x756.npz")
MAX_KP, RESIZE_TO, ANGLE = 4000, (500, 500), 180


@pytest.fixture(scope="module")
def photos():
    z = np.load(GOLDEN)
    return np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])


@pytest.fixture(scope="module")
def scenarios(ctx, photos):
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    return pipeline.run_main_scenarios(ctx, photos[0], photos[1], resize_to=RESIZE_TO, angle=ANGLE, max_keypoints=MAX_KP)


@pytest.fixture(scope="module")
def transformed(photos):
    """the statement's images, once"""
    return {"normal": photos[1], "rotated": warp_ref.img_rotate(photos[1], ANGLE), "resized": warp_ref.resize(photos[1], RESIZE_TO)}


@pytest.fixture(scope="module")
def host_route(ctx, pkg, photos, transformed):
    """name -> (matches, out, results) of the GMS flow by the host-list route, once"""
    batch = importlib.import_module("sfm-gms_amd.batch")
    left = photos[0]
    det = {}
    for name, img in (("left", left),) + tuple(transformed.items()):
        kps, rows, _ = batch.detect_images_pyramid(ctx, img[None], 20, MAX_KP, 8, descriptor="grad")
        det[name] = (kps[0], rows[0], (img.shape[1], img.shape[0]))
    out = {}
    for name in transformed:
        (kp1, rows1, size1), (kp2, rows2, size2) = det["left"], det[name]
        table = batch.FrameTable(ctx, [kp1, kp2], [size1, size2])
        dt = batch.DescriptorTable(ctx, table, [rows1, rows2], pkg.GMS_DESC_L2_F32X128)
        pairs = np.zeros(1, dtype=pkg.PAIR_DTYPE)
        pairs[0] = (0, 1, len(kp1), 0, 0)
        matches = batch.match_pairs(ctx, dt, pairs)
        res_out, res, _ = batch.filter_pairs(ctx, table, pairs, matches, True, True, 6.0)
        out[name] = (matches, res_out, res)
    return out


def test_transformed_images_equal_the_statement(scenarios, transformed):
    assert np.array_equal(scenarios["images"]["rotated"], transformed["rotated"])
    assert np.array_equal(scenarios["images"]["resized"], transformed["resized"])
    assert scenarios["sizes"] == [(1008, 756)] * 3 + [RESIZE_TO]
    frames, _ = scenarios["tables"]
    assert frames.n_frames == 4 and frames.d_wh.cpu().numpy().reshape(4, 2).tolist() == [list(s) for s in scenarios["sizes"]]
    assert (np.diff(frames.frame_off_host) > 500).all()


def _same_record(got, want, keys):
    for k in keys:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert got["pairs"]["m"].tolist() == want["pairs"]["m"].tolist() and got["pairs"]["match_off"].tolist() == want["pairs"]["match_off"].tolist()


@pytest.mark.parametrize("name", ["normal", "rotated"])
def test_equally_sized_scenarios_equal_run_images(ctx, photos, scenarios, transformed, name):
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    images = np.stack([photos[0], transformed[name]])
    want = pipeline.run_images(ctx, images, method="gms", max_keypoints=MAX_KP, withRotation=True, withScale=True)
    _same_record(scenarios[name]["gms"], want, ("matches", "out", "results"))
    assert int(want["results"]["status"][0]) == 0 and int(want["results"]["n_inliers"][0]) > 0
    want = pipeline.run_images(ctx, images, method="bf", max_keypoints=MAX_KP)
    _same_record(scenarios[name]["bf"], want, ("out", "results", "bf_results"))


def test_resized_scenario_equals_the_host_list_route(scenarios, host_route):
    matches, out, res = host_route["resized"]
    got = scenarios["resized"]["gms"]
    assert got["matches"].tobytes() == matches.tobytes() and got["results"].tobytes() == res.tobytes()
    n = int(res["n_inliers"][0])
    assert int(res["status"][0]) == 0 and n > 0 and got["out"][:n].tobytes() == out[:n].tobytes()


def test_rotation_hypothesis_agrees_with_the_host_list_route(scenarios, host_route):
    for name in ("normal", "rotated", "resized"):
        got, want = scenarios[name]["gms"]["results"], host_route[name][2]
        assert (int(got["best_rot"][0]) == 5) == (int(want["best_rot"][0]) == 5), name
        assert (int(got["best_rot"][0]), int(got["best_scale"][0])) == (int(want["best_rot"][0]), int(want["best_scale"][0])), name
