"""-m gpu: the two-view kernels away from the one scene of test_gpu_twoview.py -- the five-point solver as the kernel runs it
(gms_selftest_five_point) on well-posed and degenerate minimal samples; gms_find_essential_batch_device on other motions, sizes around
the workgroup widths, iteration bounds around the round sizes, other thresholds and cameras, in both template shapes (the default and
GMS_TV_GEOM=0, which is read once per process: a fresh child); recoverPose with each of the four hypotheses the true pose, batched and
single-pair; pairs beyond the 16384-point vote cache of recover_pose_batch_kernel; the whole chain on a forward and a rolled motion.
References: oracle/sfm_ref.py (numpy) -- for the solver and for findEssentialMat what it returned as recorded in
tests/golden/twoview/restatement.npz, which tests/test_twoview_core.py holds to a fresh run; the scenes and the shared checks are
tests/twoview_scenes.py.

Run as a script (`python test_gpu_twoview_geometry.py out.npz`) this file only runs gms_find_essential_batch_device on every
configuration and saves what it returned: the child of test_find_essential_wide_shape_in_a_fresh_process."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import sfm_ref
import twoview_scenes as scenes

pytestmark = pytest.mark.gpu
SENTINEL = 77
REFUSED = "refused"      # what a batch with max_iters < 1 gives: GMS_ERR_BAD_ARG, nothing written


def _upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def _coords_batch(pkg, pairs_uv):
    """[(uv1, uv2)] -> pair table (pair i owns n_i + slack entries), TWO_VIEW records with n_points = n_i, both coordinate arrays"""
    types = importlib.import_module("sfm-gms_amd.types")
    pairs, tv = np.zeros(len(pairs_uv), dtype=pkg.PAIR_DTYPE), np.zeros(len(pairs_uv), dtype=types.TWO_VIEW_DTYPE)
    off, c1, c2 = 0, [], []
    for i, (u1, u2) in enumerate(pairs_uv):
        n, slack = len(u1), 3 + (i % 4)
        pairs[i] = (0, 1, n + slack, 0, off)
        tv["n_points"][i] = n
        pad = np.full((slack, 2), 12345.0, dtype=np.float32)
        c1 += [u1, pad]
        c2 += [u2, pad]
        off += n + slack
    return pairs, tv, np.concatenate(c1), np.concatenate(c2)


# ---- the solver as the kernel runs it --------------------------------------------------------------------------------------------------
def test_solver_in_lds_lanes_on_every_family(ctx):
    """gms_selftest_five_point -- sixteen lanes of a wave, matrices in LDS, as find_essential_kernel runs the solver -- on 300 seeded
    samples of each of nine families: every model is a valid essential matrix (constraints within the gate, singular values (s, s, 0)),
    on the degenerate families too; on the four well-posed ones the models equal sfm_ref.five_point's within 1e-9 on all but 0.3 % of
    the samples. With 1, 15, 16 and 17 samples (a partial wave, a full one, a second workgroup) each sample's models are bit for bit
    those of the 300-sample launch."""
    full = {fam: ctx.selftest_five_point(*scenes.minimal_samples(fam)) for fam in scenes.FAMILIES}
    seen = scenes.compare_solver_on_families(lambda fam: full[fam])
    assert seen["planar"] > 1000
    for fam in scenes.FAMILIES:
        x1, x2 = scenes.minimal_samples(fam)
        for count in (1, 15, 16, 17):
            part = ctx.selftest_five_point(x1[:count], x2[:count])
            assert len(part) == count and all(np.array_equal(a, b) for a, b in zip(part, full[fam])), (fam, count)


# ---- findEssentialMat ----------------------------------------------------------------------------------------------------------------
def _groups():
    """{(camera, prob, threshold, max_iters): [case names]}: one ragged batch each; the degenerate scenes sit among the healthy pairs"""
    groups = {}
    for name, (_, camera, prob, threshold, max_iters) in list(scenes.RANSAC_CASES.items()) + list(scenes.DEGENERATE_CASES.items()):
        groups.setdefault((camera, prob, threshold, max_iters), []).append(name)
    for key, names in groups.items():           # degenerate pairs in the middle of their batch, not at its end
        sick = [n for n in names if n in scenes.DEGENERATE_CASES]
        well = [n for n in names if n not in scenes.DEGENERATE_CASES]
        assert well
        groups[key] = well[:1] + sick + well[1:]
    return groups


def _run_find_essential(ctx, pkg, names, key):
    """one batch -> {name: (E, mask, n_ransac, iters, status, slack untouched)}"""
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    camera, prob, threshold, max_iters = key
    pairs, tv, c1, c2 = _coords_batch(pkg, [scenes.case_scene(n) for n in names])
    d_pairs, d_c1, d_c2, d_tv = _upload(pairs), _upload(c1), _upload(c2), _upload(tv)
    d_mask = torch.full((len(c1),), SENTINEL, dtype=torch.uint8, device=d_c1.device)
    torch.cuda.synchronize()
    call = lambda: ctx.find_essential_batch_device(types.make_camera(camera), d_pairs.data_ptr(), len(pairs), d_c1.data_ptr(), d_c2.data_ptr(),
                                                   d_mask.data_ptr(), d_tv.data_ptr(), prob, threshold, max_iters)
    if max_iters < 1:
        # include/gms.h's entry point takes max_iters >= 1 (the host core and the restatement run 0 as 1): the call is refused as a bad
        # argument and nothing is launched -- no record, no mask byte changes
        with pytest.raises(types.GmsError) as err:
            call()
        ctx.synchronize()
        assert err.value.code == types.GMS_ERR_BAD_ARG
        assert d_tv.cpu().numpy().tobytes() == tv.tobytes() and (d_mask.cpu().numpy() == SENTINEL).all()
        return {name: REFUSED for name in names}
    call()
    ctx.synchronize()
    got, mask = d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE), d_mask.cpu().numpy()
    out = {}
    for i, name in enumerate(names):
        o, n, m = int(pairs["match_off"][i]), int(tv["n_points"][i]), int(pairs["m"][i])
        out[name] = (got["E"][i].copy(), mask[o:o + n].copy(), int(got["n_ransac"][i]), int(got["ransac_iters"][i]), int(got["status"][i]),
                     bool((mask[o + n:o + m] == SENTINEL).all()))
    return out


def _run_every_group(ctx, pkg):
    out = {}
    for key, names in _groups().items():
        out.update(_run_find_essential(ctx, pkg, names, key))
    return out


def _check_find_essential(results):
    """equality with the restatement exactly as test_find_essential_batch_against_the_restatement demands it; the degenerate pairs
    are held to the properties any answer must have"""
    assert set(results) == set(scenes.RANSAC_CASES) | set(scenes.DEGENERATE_CASES)
    for name, result in results.items():
        if result == REFUSED:
            assert (scenes.RANSAC_CASES.get(name) or scenes.DEGENERATE_CASES[name])[4] < 1, name
            continue
        E, mask, n_ransac, iters, status, slack_ok = result
        assert slack_ok, name
        if name in scenes.DEGENERATE_CASES:
            assert status == (0 if n_ransac > 0 else -8), name
            scenes.assert_ransac_properties(name, E, mask, n_ransac, iters)
            continue
        wE, wmask, witers = scenes.recorded_ransac(name)
        assert np.array_equal(mask, wmask) and n_ransac == int(wmask.sum()) and iters == witers, (name, n_ransac, int(wmask.sum()), iters, witers)
        if wE is None:
            assert status == -8 and not E.any(), name
        else:
            assert status == 0 and np.abs(E - wE).max() < 1e-9, (name, np.abs(E - wE).max())


def test_find_essential_on_other_motions_sizes_and_parameters(ctx, pkg):
    """find_essential_kernel<128, 12> (the default shape) on every configuration of twoview_scenes.RANSAC_CASES, one ragged batch per
    (camera, confidence, threshold, max_iters): iteration count, inlier mask and count equal to sfm_ref.find_essential_mat, E within
    1e-9, bytes beyond a pair's points untouched. The degenerate scenes (an image's points on a line) ride in the same batches: they
    end with no model (-8, zero E, zero mask) or a VALID essential matrix whose Sampson test is the mask, and the healthy pairs'
    records and masks are byte for byte what the batch without them gives."""
    results = _run_every_group(ctx, pkg)
    _check_find_essential(results)
    for key, names in _groups().items():
        if not any(n in scenes.DEGENERATE_CASES for n in names):
            continue
        well = [n for n in names if n not in scenes.DEGENERATE_CASES]
        alone = _run_find_essential(ctx, pkg, well, key)
        for n in well:
            assert alone[n] != REFUSED and alone[n][0].tobytes() == results[n][0].tobytes() and np.array_equal(alone[n][1], results[n][1]) and alone[n][2:] == results[n][2:], n


def test_find_essential_wide_shape_in_a_fresh_process(pkg, tmp_path):
    """The same configurations through find_essential_kernel<256, 16> (GMS_TV_GEOM=0, read once per process: a fresh child runs the
    batches and saves what came back), held to the same equalities."""
    out = str(tmp_path / "wide.npz")
    env = dict(os.environ, GMS_TV_GEOM="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    names = [str(n) for n in z["names"]]
    results = {n: REFUSED if z["refused"][i] else (z[f"E_{i}"], z[f"mask_{i}"], int(z["n_ransac"][i]), int(z["iters"][i]), int(z["status"][i]),
                                                    bool(z["slack_ok"][i])) for i, n in enumerate(names)}
    assert str(z["geom"]) == "0"
    _check_find_essential(results)


# ---- recoverPose: each of the four hypotheses the true one -----------------------------------------------------------------------------
def _pose_cases(seed):
    """one E: for each of its four hypotheses a scene in which that one is the true pose, for E and -E: 8 (E, uv1, uv2, R, t)"""
    rng = np.random.default_rng(seed)
    E = scenes.random_essential(rng)
    cases = []
    for h in range(4):
        uv1, uv2, R, t = scenes.hypothesis_scene(rng, E, h)
        wrong = rng.uniform(size=len(uv1)) < 0.2
        uv2[wrong] = np.stack([rng.uniform(0, 1920, int(wrong.sum())), rng.uniform(0, 1080, int(wrong.sum()))], axis=1).astype(np.float32)
        cases += [(E, uv1, uv2, R, t), (-E, uv1, uv2, R, t)]
    return cases


@pytest.mark.parametrize("seed", [41, 42])
def test_recover_pose_every_hypothesis_batched_and_single(ctx, pkg, seed):
    """recover_pose_batch_kernel (E preset in the records) and the single-pair gms_recover_pose_device on four scenes per E, each with
    another of (R1, t), (R2, t), (R1, -t), (R2, -t) the true pose (a fifth of the correspondences wrong), for E and -E, with and without
    an input mask: R and t within 1e-9 of sfm_ref.recover_pose and equal to the scene's pose, the count and the mask exact, and over
    the four scenes of one E the winner's index takes four distinct values in 0..3."""
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    cases = _pose_cases(seed)
    cam = types.make_camera(scenes.BASE_CAMERA)
    pairs, tv, c1, c2 = _coords_batch(pkg, [(u1, u2) for _, u1, u2, _, _ in cases])
    tv["E"] = [E for E, *_ in cases]
    rng = np.random.default_rng(seed + 100)
    in_bytes = rng.choice(np.array([0, 1, 200, 255], dtype=np.uint8), size=len(c1), p=[0.15, 0.4, 0.25, 0.2])
    d_pairs, d_c1, d_c2 = _upload(pairs), _upload(c1), _upload(c2)
    for use_mask in (False, True):
        d_tv = _upload(tv)
        d_mask = _upload(in_bytes) if use_mask else torch.full((len(c1),), SENTINEL, dtype=torch.uint8, device=d_c1.device)
        torch.cuda.synchronize()
        ctx.recover_pose_batch_device(cam, d_pairs.data_ptr(), len(pairs), d_c1.data_ptr(), d_c2.data_ptr(), d_mask.data_ptr(), d_tv.data_ptr(),
                                      use_in_mask=use_mask)
        ctx.synchronize()
        got, mask = d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE), d_mask.cpu().numpy()
        which = {1.0: [], -1.0: []}
        for i, (E, uv1, uv2, R, t) in enumerate(cases):
            o, n, m = int(pairs["match_off"][i]), len(uv1), int(pairs["m"][i])
            im = in_bytes[o:o + n] if use_mask else None
            Rr, tr, good, wmask = sfm_ref.recover_pose(E, uv1, uv2, scenes.BASE_CAMERA, im)
            assert np.abs(Rr - R).max() < 1e-12 and np.abs(tr - t).max() < 1e-12 and good > 0.7 * (n if im is None else (im != 0).sum())
            assert int(got["status"][i]) == 0 and np.abs(got["R"][i] - Rr).max() < 1e-9 and np.abs(got["t"][i] - tr).max() < 1e-9, (i, use_mask)
            assert int(got["n_pose"][i]) == good and np.array_equal(mask[o:o + n], wmask), (i, use_mask)
            assert np.array_equal(mask[o + n:o + m], in_bytes[o + n:o + m] if use_mask else np.full(m - n, SENTINEL, dtype=np.uint8))
            which[1.0 if i % 2 == 0 else -1.0].append(int(got["pose_which"][i]))      # (cases alternate E, -E)
            # the single-pair entry point on the same pair
            d_n = torch.tensor([n], dtype=torch.int32, device=d_c1.device)
            d_pose = torch.zeros(types.POSE_DTYPE.itemsize, dtype=torch.uint8, device=d_c1.device)
            d_out = torch.full((m,), SENTINEL, dtype=torch.uint8, device=d_c1.device)
            d_in = _upload(in_bytes[o:o + m]) if use_mask else None
            torch.cuda.synchronize()
            ctx.recover_pose_device(E, scenes.BASE_CAMERA, d_c1.data_ptr() + 8 * o, d_c2.data_ptr() + 8 * o, d_n.data_ptr(), m,
                                    d_in.data_ptr() if use_mask else None, d_pose.data_ptr(), d_out.data_ptr())
            ctx.synchronize()
            pose, sm = d_pose.cpu().numpy().view(types.POSE_DTYPE)[0], d_out.cpu().numpy()
            assert np.abs(pose["R"] - Rr).max() < 1e-9 and np.abs(pose["t"] - tr).max() < 1e-9 and int(pose["n_good"]) == good, (i, use_mask)
            assert np.array_equal(sm[:n], wmask) and (sm[n:] == SENTINEL).all() and int(pose["which"]) == int(got["pose_which"][i]), (i, use_mask)
        assert sorted(which[1.0]) == [0, 1, 2, 3] and sorted(which[-1.0]) == [0, 1, 2, 3], which


# ---- beyond the vote cache -------------------------------------------------------------------------------------------------------------
def test_recover_pose_beyond_the_vote_cache(ctx, pkg):
    """recover_pose_batch_kernel keeps the four votes of a pair's first 16384 correspondences in LDS and works the winner's vote out again
    (tv::pose_vote_one) for the ones beyond: pairs of 16384 + 300 points (two of them, true pose (R1, t) and (R1, -t) of the
    restatement's labelling, so that whichever way the core labels t one of them is won by a -t hypothesis), of exactly 16384 and of
    16385, a fifth of the correspondences wrong, with and without an input mask. The mask equals the restatement's over the whole
    range, its nonzero bytes number n_pose, bytes beyond n are untouched. (The restatement's per-point SVD loop is batched here --
    twoview_scenes.recover_pose_batched -- after that form is shown equal to sfm_ref.recover_pose on 600 points.)"""
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    rng = np.random.default_rng(61)
    E = scenes.random_essential(rng)
    small = scenes.hypothesis_scene(rng, E, 3)
    in600 = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=600)
    for im in (None, in600):
        a, b = sfm_ref.recover_pose(E, small[0], small[1], scenes.BASE_CAMERA, im), scenes.recover_pose_batched(E, small[0], small[1], in_mask=im)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    cases = []
    for n, h in ((16384 + 300, 0), (16384 + 300, 2), (16384, 3), (16385, 1)):
        uv1, uv2, R, t = scenes.hypothesis_scene(rng, E, h, n=n)
        wrong = rng.uniform(size=n) < 0.2
        uv2[wrong] = np.stack([rng.uniform(0, 1920, int(wrong.sum())), rng.uniform(0, 1080, int(wrong.sum()))], axis=1).astype(np.float32)
        cases.append((uv1, uv2, R, t))
    pairs, tv, c1, c2 = _coords_batch(pkg, [c[:2] for c in cases])
    tv["E"] = E
    in_bytes = rng.choice(np.array([0, 1, 200, 255], dtype=np.uint8), size=len(c1), p=[0.15, 0.4, 0.25, 0.2])
    d_pairs, d_c1, d_c2 = _upload(pairs), _upload(c1), _upload(c2)
    cam = types.make_camera(scenes.BASE_CAMERA)
    for use_mask in (False, True):
        d_tv = _upload(tv)
        d_mask = _upload(in_bytes) if use_mask else torch.full((len(c1),), SENTINEL, dtype=torch.uint8, device=d_c1.device)
        torch.cuda.synchronize()
        ctx.recover_pose_batch_device(cam, d_pairs.data_ptr(), len(pairs), d_c1.data_ptr(), d_c2.data_ptr(), d_mask.data_ptr(), d_tv.data_ptr(),
                                      use_in_mask=use_mask)
        ctx.synchronize()
        got, mask = d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE), d_mask.cpu().numpy()
        for i, (uv1, uv2, R, t) in enumerate(cases):
            o, n, m = int(pairs["match_off"][i]), len(uv1), int(pairs["m"][i])
            Rr, tr, good, wmask, _ = scenes.recover_pose_batched(E, uv1, uv2, in_mask=in_bytes[o:o + n] if use_mask else None)
            assert np.abs(Rr - R).max() < 1e-12 and np.abs(tr - t).max() < 1e-12
            assert np.abs(got["R"][i] - Rr).max() < 1e-9 and np.abs(got["t"][i] - tr).max() < 1e-9, (i, use_mask)
            assert np.array_equal(mask[o:o + n], wmask), (i, use_mask, np.nonzero(mask[o:o + n] != wmask)[0][:10])
            assert int(got["n_pose"][i]) == good == int(np.count_nonzero(mask[o:o + n])) and good > 0.5 * n * (0.85 if use_mask else 1.0)
            assert wmask[16384:].any() or n == 16384
            assert np.array_equal(mask[o + n:o + m], in_bytes[o + n:o + m] if use_mask else np.full(m - n, SENTINEL, dtype=np.uint8))
        assert int(got["pose_which"][0]) >= 2 or int(got["pose_which"][1]) >= 2, got["pose_which"]
        assert len({int(w) for w in got["pose_which"]}) == 4


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
def test_two_view_chain_on_forward_and_rolled_motion(ctx, pkg, synth):
    """gms_two_view_batch_device (gather -> findEssentialMat(0.7, 1.0) -> recoverPose -> compaction -> undistort -> triangulate) on a
    forward-motion pair and a pair rolled by 90 degrees, with lens distortion, against sfm_ref.two_view at the tolerances of
    test_two_view_batch_after_the_filter: RANSAC decisions, masks and counts exact; E, R, t within 1e-9; the 3-D points of true
    correspondences within 1e-6 relative; the error sums within 1e-8 relative."""
    import torch
    types = importlib.import_module("sfm-gms_amd.types")
    dist = (-0.12, 0.05, 0.001, -0.0007, 0.01)
    frames, pair_uv = [], []
    for seed, name in ((71, "forward"), (72, "roll_90")):
        uv1, uv2 = scenes.scene(seed, 1500, 0.3, **scenes.MOTIONS[name])
        frames += [synth.make_keypoints(uv1), synth.make_keypoints(uv2)]
        pair_uv.append((uv1, uv2))
    kp, frame_off = types.concat_frames(frames)
    n = 1500
    pairs = np.zeros(2, dtype=pkg.PAIR_DTYPE)
    pairs[0], pairs[1] = (0, 1, n, 0, 0), (2, 3, n, 0, n)
    matches = np.concatenate([synth.make_matches(np.arange(n), np.arange(n)), synth.make_matches(np.arange(n), np.arange(n))])
    res = np.zeros(2, dtype=pkg.RESULT_DTYPE)
    res["n_inliers"] = n
    dev = torch.device("cuda", 0)
    d_kp, d_off, d_pairs, d_matches, d_res = _upload(kp), torch.from_numpy(frame_off).to(dev), _upload(pairs), _upload(matches), _upload(res)
    d_c1, d_c2 = torch.zeros(4 * n, dtype=torch.float32, device=dev), torch.zeros(4 * n, dtype=torch.float32, device=dev)
    d_mask, d_p3 = torch.zeros(2 * n, dtype=torch.uint8, device=dev), torch.zeros(6 * n, dtype=torch.float64, device=dev)
    d_tv = torch.zeros(2 * types.TWO_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.two_view_batch_device(types.make_camera(scenes.BASE_CAMERA, dist), d_kp.data_ptr(), d_off.data_ptr(), 4, d_pairs.data_ptr(), 2, n,
                              d_matches.data_ptr(), d_res.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), d_mask.data_ptr(), d_p3.data_ptr(),
                              d_tv.data_ptr(), 0.7, 1.0, 1000)
    ctx.synchronize()
    tv, mask, p3 = d_tv.cpu().numpy().view(types.TWO_VIEW_DTYPE), d_mask.cpu().numpy(), d_p3.cpu().numpy().reshape(-1, 3)
    c1, c2 = d_c1.cpu().numpy().reshape(-1, 2), d_c2.cpu().numpy().reshape(-1, 2)
    for i, (uv1, uv2) in enumerate(pair_uv):
        o, t = i * n, tv[i]
        assert c1[o:o + n].tobytes() == uv1.tobytes() and c2[o:o + n].tobytes() == uv2.tobytes() and int(t["n_points"]) == n
        ref = sfm_ref.two_view(uv1, uv2, scenes.BASE_CAMERA, dist, 0.7, 1.0)
        assert ref["E"] is not None and int(t["status"]) == 0 and int(t["n_ransac"]) == ref["n_ransac"] and int(t["ransac_iters"]) == ref["iters"]
        assert np.abs(t["E"] - ref["E"]).max() < 1e-9 and np.abs(t["R"] - ref["R"]).max() < 1e-9 and np.abs(t["t"] - ref["t"]).max() < 1e-9
        assert int(t["n_pose"]) == ref["n_pose"] and np.array_equal(mask[o:o + n], ref["mask"])
        kept = int((ref["mask"] != 0).sum())
        assert kept > 0.5 * n and int(t["n_triangulated"]) == kept and int(t["n_finite"]) == kept and int(t["n_behind"]) == ref["behind"]
        assert np.allclose(p3[o:o + kept], ref["points"], rtol=1e-6, atol=1e-9)    # (RANSAC inliers in front of both cameras: well conditioned)
        assert abs(t["sum_sq_err1"] - ref["sum_sq_err1"]) <= 1e-8 * ref["sum_sq_err1"] + 1e-14
        assert abs(t["sum_sq_err2"] - ref["sum_sq_err2"]) <= 1e-8 * ref["sum_sq_err2"] + 1e-14
        # and the estimate is the scene's motion
        Rs, ts = scenes.MOTIONS["forward" if i == 0 else "roll_90"]["R"], scenes.MOTIONS["forward" if i == 0 else "roll_90"]["t"]
        assert np.degrees(np.arccos(min(1.0, (np.trace(t["R"] @ Rs.T) - 1) / 2))) < 1.5
        assert np.degrees(np.arccos(min(1.0, float(t["t"] @ ts / np.linalg.norm(ts))))) < 12.0


if __name__ == "__main__":
    _pkg = importlib.import_module("sfm-gms_amd")
    _ctx = _pkg.GmsContext(0)
    _res = _run_every_group(_ctx, _pkg)
    _ctx.close()
    _names = list(_res)
    _rows = [(np.zeros((3, 3)), np.zeros(0, dtype=np.uint8), 0, 0, 0, False) if _res[n] == REFUSED else _res[n] for n in _names]
    _save = dict(names=np.array(_names), geom=np.array(os.environ.get("GMS_TV_GEOM", "")), refused=np.array([_res[n] == REFUSED for n in _names]),
                 n_ransac=np.array([r[2] for r in _rows]), iters=np.array([r[3] for r in _rows]), status=np.array([r[4] for r in _rows]),
                 slack_ok=np.array([r[5] for r in _rows]))
    for _i, _r in enumerate(_rows):
        _save[f"E_{_i}"], _save[f"mask_{_i}"] = _r[0], _r[1]
    np.savez(sys.argv[1], **_save)
