"""CPU: the one-to-one rule and the registration on a keep plane (tests/match_unique_ref.py) -- the hand-made lists of
tests/match_unique_cases.py against the winners they state, the host build of match_unique_core.h (tests/cpp/match_unique_host.cpp,
plain and under the address / undefined-behaviour sanitizers) against the statement byte for byte, three scenes with redirected train
indices (n_multi > 0 without the plane, 0 with it, the views untouched), inputs that are one-to-one already, the five-view scene with
ground truth through the bundle adjustment's statement, and what of the C ABI is host arithmetic."""
import os

import numpy as np
import pytest

import match_unique_cases as ucases
import match_unique_ref as U
import sfm_ba_ref as B
import sfm_ref
import sfm_register_cases as rcases
import sfm_register_ref as R
import hostbuild as hb

HOST_SRC = "match_unique_host.cpp"
NAMES = sorted(ucases.CASES)
REGISTER_ARRAYS = ("plan", "views", "registration", "points_world", "track", "cloud", "cloud_id", "cloud_obs", "cloud_est", "cloud_spread", "summary")
UNTOUCHED = ("views", "registration", "points_world")


def redirected(name):
    """A registration case with 30 % of the train indices redirected and distances 0 .. 5, as a match_unique case."""
    c = U.redirect_trains(rcases.case(name), 0.3, 77)
    return dict(c, total_m=c.get("total_m", len(c["mask"])))


def statement(c):
    return U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"], c["total_m"])


def write_input(c, path):
    flags = (1 if c["mask"] is not None else 0) | (2 if c["tv"] is not None else 0)
    with open(path, "wb") as f:
        f.write(np.array([len(c["frame_off"]) - 1, len(c["pairs"]), c["total_m"], flags], np.int64).tobytes())
        f.write(np.ascontiguousarray(c["frame_off"], dtype=np.int64).tobytes())
        f.write(np.ascontiguousarray(c["pairs"]).tobytes())
        f.write(np.ascontiguousarray(c["matches"][:c["total_m"]]).tobytes())
        if flags & 1:
            f.write(np.ascontiguousarray(c["mask"][:c["total_m"]], dtype=np.uint8).tobytes())
        if flags & 2:
            f.write(np.ascontiguousarray(c["tv"]).tobytes())


def run_host(exe, c, tmp):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    write_input(c, src)
    res = hb.run(exe, src, dst)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(dst, np.uint8)
    m = c["total_m"]
    return raw[:m].copy(), raw[m:].view(np.int32).reshape(-1, 2).copy()


def all_cases():
    return [(n, ucases.case(n)) for n in NAMES] + [("chain_roles", dict(rcases.case("chain_roles"), total_m=len(rcases.case("chain_roles")["mask"]))),
                                                    ("misfit_records", dict(rcases.case("misfit_records")))] + \
           [(n + "_redirected", redirected(n)) for n in ("chain_roles", "tiles_past_256", "chain_300")]


@pytest.mark.parametrize("name", NAMES)
def test_hand_made_lists_keep_the_stated_matches(name):
    c = ucases.case(name)
    keep, counts = statement(c)
    assert keep.shape == (c["total_m"],) and counts.shape == (len(c["pairs"]), 2)
    owned = np.zeros(c["total_m"], bool)
    for i, ks in c["expect"].items():
        off, m = int(c["pairs"][i]["match_off"]), int(c["pairs"][i]["m"])
        assert np.nonzero(keep[off:off + m])[0].tolist() == ks, (name, i)
        assert counts[i][1] == len(ks) and counts[i][0] >= len(ks)
        owned[off:off + m] = True
    for i in range(len(c["pairs"])):
        if i not in c["expect"]:                               # the misfits
            assert counts[i].tolist() == [0, 0]
    assert not keep[~owned].any()


def test_the_rule_is_not_a_maximum_matching():
    c = ucases.case("not_a_matching")
    keep, counts = statement(c)
    assert counts.tolist() == [[3, 1]]                        # three live matches, of which (0, 0) and (1, 1) could both be kept


def test_the_shape_cases_reach_what_they_are_for():
    c = ucases.case("two_chunks")
    assert c["pairs"]["m"][0] == 600 > 2 * 256
    c = ucases.case("one_train_300")
    assert (c["matches"]["trainIdx"][2:302] == 11).all() and statement(c)[1].tolist() == [[300, 1]]
    for name in ("chain_roles", "tiles_past_256", "chain_300"):
        c = redirected(name)
        keep, counts = statement(c)
        assert (counts[:, 1] < counts[:, 0]).any(), name      # the redirection left rivals


@pytest.fixture(scope="module")
def host_exe():
    exe = hb.host_exe(HOST_SRC)
    return exe


@pytest.mark.parametrize("name,c", all_cases(), ids=[n for n, _ in all_cases()])
def test_host_build_of_the_core_equals_the_statement(host_exe, tmp_path, name, c):
    want_keep, want_counts = statement(c)
    keep, counts = run_host(host_exe, c, str(tmp_path))
    assert keep.tobytes() == want_keep.tobytes() and counts.tobytes() == want_counts.tobytes()


def test_stand_alone_host_program_under_sanitizers(tmp_path):
    exe = hb.host_exe_sanitized(HOST_SRC)
    for name, c in all_cases():
        if name.startswith("tiles_past_256"):
            continue                                            # (a million keypoints: the plain build covers it)
        want_keep, want_counts = statement(c)
        keep, counts = run_host(exe, c, str(tmp_path))
        assert keep.tobytes() == want_keep.tobytes() and counts.tobytes() == want_counts.tobytes(), name


# ---- the registration on a plane -------------------------------------------------------------------------------------------------
def scene_case(shape):
    """sfm_register_cases.Scene(5, 6, 300) as a chain, a star or two branches; 30 % of every pair's train indices redirected."""
    sc = rcases.Scene(5, 6, 300)
    fp = {"chain": [(f, f + 1) for f in range(5)], "star": [(0, f + 1) for f in range(5)],
          "two_branches": [(0, 1), (0, 2), (1, 3), (2, 4), (3, 5)]}[shape]
    c = rcases.assemble(sc, [dict(a=a, b=b, unit=1.0 + 0.5 * i, pts=np.arange(300)) for i, (a, b) in enumerate(fp)])
    return U.redirect_trains(c, 0.3, 5)


def both(c, **kw):
    args = (c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    kw = dict({k: c[k] for k in ("plan", "total_m") if k in c}, **kw)
    keep, counts = U.unique(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"], kw.get("total_m", len(c["mask"])))
    return R.register(*args, **kw), U.register_keep(*args, keep=keep, **kw), keep, counts


@pytest.mark.parametrize("shape", ["chain", "star", "two_branches"])
def test_no_track_holds_two_keypoints_of_a_frame(shape):
    c = scene_case(shape)
    without, with_, keep, counts = both(c)
    s0, s1 = without["summary"][0], with_["summary"][0]
    print(shape, "n_multi", s0["n_multi"], "->", s1["n_multi"], "tracks", s0["n_tracks"], "->", s1["n_tracks"], "kept", counts[:, 1].tolist())
    assert s0["n_multi"] > 0 and s1["n_multi"] == 0 and s1["n_tracks"] > s0["n_tracks"]
    for k in UNTOUCHED:
        assert without[k].tobytes() == with_[k].tobytes(), k
    assert s1["n_points"] == counts[:, 1].sum() == with_["cloud_est"].sum() == (with_["track"] >= 0).sum()
    assert (s1["n_registered"], s1["n_ok_pairs"]) == (s0["n_registered"], s0["n_ok_pairs"])


def test_one_to_one_input_changes_nothing():
    c = rcases.case("chain_roles")
    without, with_, keep, counts = both(c)
    live = np.zeros(len(c["mask"]), np.uint8)
    for i in range(len(c["pairs"])):
        off, m = int(c["pairs"][i]["match_off"]), int(c["pairs"][i]["m"])
        live[off:off + m] = U.live_of(i, c["frame_off"], c["pairs"], c["matches"], c["mask"], c["tv"])
    assert keep.tobytes() == live.tobytes() and (counts[:, 0] == counts[:, 1]).all() and counts[:, 0].sum() > 200
    for k in REGISTER_ARRAYS:
        assert without[k].tobytes() == with_[k].tobytes(), k
    none = U.register_keep(c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    for k in REGISTER_ARRAYS:
        assert without[k].tobytes() == none[k].tobytes(), k


def test_a_plane_of_zeros_leaves_the_views_and_no_track():
    c = rcases.case("chain_roles")
    args = (c["frame_off"], c["pairs"], c["matches"], c["mask"], c["points3d"], c["tv"], c["root"], c["min_links"])
    without, with_ = R.register(*args), U.register_keep(*args, keep=np.zeros(len(c["mask"]), np.uint8))
    for k in UNTOUCHED:
        assert without[k].tobytes() == with_[k].tobytes(), k
    assert (with_["track"] == -1).all() and len(with_["cloud_id"]) == 0 and with_["summary"]["n_points"][0] == 0


def five_views_with_plane(synth):
    """test_sfm_register_ref.truth_scene (five views, 20 % of the train indices redrawn, default_rng(1)) through the CPU two-view chain
    -> the scene, the arrays, the registration without and with the plane."""
    from test_sfm_register_ref import truth_scene
    sc, frame_pairs, pairs, matches, mask, points, tv = truth_scene(synth, None)
    for i, (a, b) in enumerate(frame_pairs):
        q, t = matches["queryIdx"][i * 400:(i + 1) * 400], matches["trainIdx"][i * 400:(i + 1) * 400]
        uv1 = np.stack([sc["frames"][a]["x"][q], sc["frames"][a]["y"][q]], 1)
        uv2 = np.stack([sc["frames"][b]["x"][t], sc["frames"][b]["y"][t]], 1)
        r = sfm_ref.two_view(uv1, uv2, sc["camera"], None, 0.7, 1.0, 1000)
        assert r["E"] is not None
        k = int((r["mask"] != 0).sum())
        tv[i]["R"], tv[i]["t"], tv[i]["n_points"], tv[i]["n_triangulated"] = r["R"], np.asarray(r["t"]).reshape(3), 400, k
        mask[i * 400:(i + 1) * 400] = r["mask"]
        points[i * 400:i * 400 + k] = r["points"]
    frame_off = np.arange(6, dtype=np.int64) * 400
    keep, counts = U.unique(frame_off, pairs, matches, mask, tv)
    without = R.register(frame_off, pairs, matches, mask, points, tv)
    with_ = U.register_keep(frame_off, pairs, matches, mask, points, tv, keep=keep)
    return sc, (frame_off, pairs, matches, mask, points, tv), without, with_, keep, counts


def test_five_views_with_the_plane_against_truth_and_through_the_bundle_adjustment(synth):
    """The scene and seed of test_sfm_register_ref.truth_scene as they stand (default_rng(1)): both assertions hold for it."""
    from test_sfm_register_ref import check_against_truth
    sc, (frame_off, pairs, matches, mask, points, tv), without, with_, keep, counts = five_views_with_plane(synth)
    check_against_truth(sc, with_)
    for k in UNTOUCHED:
        assert without[k].tobytes() == with_[k].tobytes(), k
    xy = np.concatenate([np.stack([fr["x"], fr["y"]], 1) for fr in sc["frames"]]).astype(np.float32)
    cam = tuple(sc["camera"]) + (0.0,) * 5
    s = []
    for reg in (without, with_):
        out = B.bundle_adjust(xy, frame_off, pairs, matches, mask, reg["views"], reg["registration"], reg["track"], reg["cloud"], reg["cloud_id"],
                              cam, n_iters=0)
        s.append(out["ba_summary"][0])
    print("n_multi", without["summary"]["n_multi"][0], "->", with_["summary"]["n_multi"][0], "tracks used", s[0]["n_tracks_used"], "->",
          s[1]["n_tracks_used"], "multi", s[0]["n_tracks_multi"], "->", s[1]["n_tracks_multi"])
    assert with_["summary"]["n_multi"][0] == 0 and s[1]["n_tracks_multi"] == 0
    assert s[1]["n_tracks_used"] >= s[0]["n_tracks_used"]


# ---- what of the C ABI is host arithmetic ------------------------------------------------------------------------------------------
def test_workspace_size_and_the_one_shots_refusals_need_no_device(pkg):
    lib = pkg.load_library()
    up = lambda b: (b + 255) & ~255
    assert lib.gms_match_unique_workspace_bytes(7, 16000, 21000) == 2 * up(16 * 21000)
    assert lib.gms_match_unique_workspace_bytes(999, 10 ** 7, 10 ** 7) == 32 * 10 ** 7      # neither the pairs nor the keypoints count
    assert lib.gms_match_unique_workspace_bytes(0, 0, 0) == 256
    assert lib.gms_match_unique_workspace_bytes(-1, 10, 10) == 0 and lib.gms_match_unique_workspace_bytes(1, 2 ** 31 - 1, 10) == 0
    assert lib.gms_match_unique_workspace_bytes(1, 10, -1) == 0 and lib.gms_match_unique_workspace_bytes(1, 10, 2 ** 40) == 0
    c = ucases.case("misfits")
    good = ucases.case("equal_distances")
    keep, counts = np.zeros(c["total_m"], np.uint8), np.zeros((len(c["pairs"]), 2), np.int32)

    def call(frame_off, pairs, matches=c["matches"], keep_ptr=keep.ctypes.data, counts_ptr=counts.ctypes.data, n_frames=None):
        return lib.gms_match_unique(frame_off.ctypes.data if frame_off is not None else None, len(c["frame_off"]) - 1 if n_frames is None else n_frames,
                                    pairs.ctypes.data, len(pairs), matches.ctypes.data if matches is not None else None, None, None, keep_ptr, counts_ptr)
    for i in (1, 2, 3, 4, 6):   # every misfit record the host can tell (the arrays' length is not the one-shot's to know), beside one that fits
        assert call(c["frame_off"], np.ascontiguousarray(c["pairs"][[0, i]])) == -1, i
    assert call(None, good["pairs"]) == -1 and call(good["frame_off"], good["pairs"], n_frames=0) == -1
    assert call(good["frame_off"], good["pairs"], matches=None) == -1 and call(good["frame_off"], good["pairs"], keep_ptr=None) == -1
    assert call(good["frame_off"], good["pairs"], counts_ptr=None) == -1
    assert call(np.array([0, 9, 8], np.int64), good["pairs"]) == -1                          # decreasing offsets
    with pytest.raises(ValueError):
        pkg.uniqueMatches(good["matches"][2:9], 8, 9, mask=np.ones(3, np.uint8))             # a mask of another length
