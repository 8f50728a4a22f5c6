"""A dataset file in, filtered matches (and two-view geometry) out: the reference's SIFT_matchGMS + structureFromMotion flow
(FeatureMatchUtil.cpp:52-84 -> SfMUtil.cpp:17-82) for every pair of a GMSFRM01 file, on the GPU end to end:

    descriptors --gms_bfmatch_device--> putative matches --gms_filter_device--> survivors
        --gms_two_view_batch_device--> essential matrix, pose, triangulated points, reprojection error   (with a camera)

method="logos" runs the reference's SIFT_matchLOGOS flow instead (FeatureMatchUtil.cpp:86-131):

    descriptors --gms_logos_words_device--> visual words --gms_logos_prepare_device / gms_logos_filter_device--> survivors
        --gms_two_view_batch_device--> ...                                                                  (with a camera)

method="bf" runs the reference's DEFAULT_SIFT flow (bruteForceMatch, FeatureMatchUtil.cpp:20-31; its SIFT_matchBF baseline):

    descriptors --gms_bf_select_device (matcher, cross-check, sort, ratio prune)--> survivors
        --gms_two_view_batch_device--> ...                                                                  (with a camera)

run_images is the same three flows from pixels: grey or BGR images --gms_bgr_to_gray_device--> grey planes
    --gms_detect_pyramid_(grad_)batch_device--> keypoints and rows --gms_detect_pack_device--> the resident tables --> the stages above.

torch here is device memory only; every stage is a call into csrc/libgms_hip.so. Used by tools/gms_filter_file.py, tools/gms_sfm_pair.py
and the tests."""
from types import SimpleNamespace

import numpy as np
import torch

from .batch import (BfSelect, DescriptorTable, DetectPyramid, FrameTable, LogosDictionary, LogosFilter, LogosTable, DensePairs, dense_fuse_sources, fuse_dense, MatchUnique, SfmBundle, SfmRegister, Warp, _device, _to_dev,
                    bf_select_table, bgr_to_gray, frame_counts, frame_pairs_of, logos_dictionary, pair_table, tables_from_detector)
from .api import getRotationMatrix2D, logos_dict_args
from .types import (DMATCH_DTYPE, GMS_DESC_HAMMING256, GMS_DESC_L2_F32X128, GMS_ERR_CAPACITY, GMS_OK, PAIR_DTYPE, RESULT_DTYPE, TWO_VIEW_DTYPE,
                    desc_layout, make_camera, sfm_ba_params)

METHODS = ("gms", "bf", "logos")


def _two_view(ctx, frames, d_pairs, n_pairs, max_m, total_m, d_out, d_res, camera, dist, prob, ransac_threshold, max_iters, pairs=None,
              reg=None):
    """gms_two_view_batch_device on the survivors d_out and their gms_pair_result records d_res, laid out by the pair table d_pairs ->
    the two-view part of run_dataset's result: two_view, coords1, coords2, mask, points3d as host arrays. reg = (root, min_links)
    (with `pairs`, the host copy of the pair table): gms_sfm_register_device then joins the pairs on the tensors the stage left, in
    stream order behind it -> also SfmRegister.results()'s arrays (the plan as `register_plan`). reg[3] (unique): gms_match_unique_device
    in between, the registration on its keep plane -> also `keep` and `unique_counts`."""
    dev = frames.device
    cam = make_camera(camera, dist)
    d_c1 = torch.zeros(max(total_m, 1) * 2, dtype=torch.float32, device=dev)
    d_c2 = torch.zeros(max(total_m, 1) * 2, dtype=torch.float32, device=dev)
    d_mask = torch.zeros(max(total_m, 1), dtype=torch.uint8, device=dev)
    d_p3 = torch.zeros(max(total_m, 1) * 3, dtype=torch.float64, device=dev)
    d_tv = torch.zeros(max(n_pairs, 1) * TWO_VIEW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.two_view_batch_device(cam, frames.d_kp.data_ptr(), frames.d_frame_off.data_ptr(), frames.n_frames, d_pairs.data_ptr(), n_pairs,
                              max_m, d_out.data_ptr(), d_res.data_ptr(), d_c1.data_ptr(), d_c2.data_ptr(), d_mask.data_ptr(),
                              d_p3.data_ptr(), d_tv.data_ptr(), prob, ransac_threshold, max_iters)
    joined = {}
    if reg is not None:
        uq = None
        if reg[3]:   # one-to-one matches per pair in front, in stream order, on the tensors the two-view stage left
            uq = MatchUnique(ctx, frames.frame_off_host, pairs, device=dev, d_frame_off=frames.d_frame_off, d_pairs=d_pairs)
        job = SfmRegister(ctx, frames.frame_off_host, pairs, reg[0], reg[1], device=dev, d_frame_off=frames.d_frame_off, d_pairs=d_pairs,
                          keep=None if uq is None else uq.d_keep)
        refine = None
        if reg[2] is not None:   # bundle adjustment behind it, in stream order, on the registration's own tensors
            refine = SfmBundle(ctx, frames.frame_off_host, pairs, job.cloud_cap, camera, dist, device=dev, d_frame_off=frames.d_frame_off,
                               d_pairs=d_pairs, **reg[2])
        if uq is not None:
            uq.run(d_out, d_mask, d_tv)
        job.run(d_out, d_mask, d_p3, d_tv)
        if refine is not None:
            refine.run(job, frames.d_kp, d_out, d_mask)
        joined = job.results()
        joined["register_plan"] = joined.pop("plan")
        if uq is not None:
            joined["keep"], joined["unique_counts"] = uq.results()
        if refine is not None:
            joined.update(refine.results(len(joined["cloud_id"])))
    ctx.synchronize()
    return dict(joined, two_view=d_tv.cpu().numpy().view(TWO_VIEW_DTYPE)[:n_pairs], coords1=d_c1.cpu().numpy().reshape(-1, 2)[:total_m],
                coords2=d_c2.cpu().numpy().reshape(-1, 2)[:total_m], mask=d_mask.cpu().numpy()[:total_m],
                points3d=d_p3.cpu().numpy().reshape(-1, 3)[:total_m])


def run_dataset(ctx, ds, withRotation=False, withScale=False, thresholdFactor=6.0, match=None, camera=None, dist=None, prob=0.7,
                ransac_threshold=1.0, max_iters=1000, device="cuda:0", method="gms", dictionary=None, logos_capacity=None,
                cross_check=True, distance_coef=4.0, max_size=500, train_dictionary=None, register=False, root=0, min_links=8, bundle=False,
                unique=False, **ba):
    """(prob, ransac_threshold: findEssentialMat's confidence and threshold as the flow this function restates passes them -- SfMUtil.cpp:39:
    RANSAC, 0.7, 1.0 -- not OpenCV's own default of 0.999, which gms_find_essential_batch_device's Python mirror keeps.)
    ds: io.Dataset. match=None: brute-force match when the file carries descriptors and no matches. camera = (fx, fy, cx, cy)
    switches the two-view stage on. Returns a dict of host arrays: pairs, matches (the putative ones), out, results, and with a camera
    two_view (TWO_VIEW_DTYPE per pair), coords1, coords2, mask, points3d -- all per-match arrays laid out by match_off.
    method="logos": the LOGOS flow on the file's descriptors and pairs (frame_a, frame_b; their m / match_off are not used) with the
    caller's `dictionary` (rows like the descriptors); see _run_logos. Without one, train_dictionary=True or a dict of
    dictionary_training_options trains it first on the file's descriptors (gms_logos_dict_train_device) -- by default on frame 0's,
    as the reference clusters desc1 (FeatureMatchUtil.cpp:100-104); the result then also carries `dictionary` and
    `dictionary_result`. A `dictionary` that is passed is used as it is and train_dictionary is then not read. With neither,
    method="logos" raises.
    method="bf": bruteForceMatch on the file's descriptors and pairs (cross_check, distance_coef, max_size as the reference's
    4.0 / 500 by default); see _run_bf.
    register=True (needs a camera): the pairs are then joined into the frame of `root` behind the two-view stage, on the device
    (gms_sfm_register_device): the pairs are walked in order, a pair registers frame_b when frame_a is registered, and a
    pair with fewer than min_links scene points shared with the pair it hangs on fails. Adds views, registration, points_world, track,
    cloud, cloud_id, cloud_obs, cloud_est, cloud_spread, summary and register_plan. register=False returns the dict without them.
    bundle=True (needs register=True; ba: n_iters, n_cg, lambda0, cg_tol, ftol, huber_px, retriangulate): gms_sfm_ba_device then refines
    views and cloud over all the keypoints of a track, in stream order behind the registration. Adds views_ba, cloud_ba,
    track_status and ba_summary; the registration's own arrays stay as they are. bundle=False returns the dict without them.
    unique=True (needs register=True; ValueError otherwise): gms_match_unique_device in front of the registration, which then builds
    its tracks from the one-to-one matches only: with the plan the library makes no track holds two keypoints of a
    frame, and the bundle adjustment reads the tracks as they are. Adds keep (uint8 per match slot) and unique_counts (int32 live, kept
    per pair); views, registration and points_world are the bytes of unique=False, which returns the dict without the two.
    The stages themselves work on resident tables (_run_gms, _run_bf, _run_logos): run_images feeds them from pixels."""
    tail = (camera, dist, prob, ransac_threshold, max_iters, _register_args(register, root, min_links, camera, bundle, ba, unique))
    if method == "bf":
        if ds.descriptors is None:
            raise ValueError("method='bf' needs the dataset's descriptors")
        frames = FrameTable(ctx, ds.frames, ds.sizes, device=device)
        descs = DescriptorTable(ctx, frames, ds.descriptors, ds.desc_kind)
        return _run_bf(ctx, descs, ds.pairs, cross_check, distance_coef, max_size, *tail)
    if method == "logos":
        trained = None
        if dictionary is None and train_dictionary not in (None, False):
            dictionary, trained = _train_dictionary(ctx, ds, dictionary_training_options(train_dictionary), device)
        if ds.descriptors is None or dictionary is None:
            raise ValueError("method='logos' needs the dataset's descriptors and a dictionary")
        frames = FrameTable(ctx, ds.frames, ds.sizes, device=device)
        kind = int(ds.desc_kind)
        dt, width = desc_layout(kind)
        d_desc = None
        if frames.total:
            desc = np.concatenate([np.ascontiguousarray(d, dtype=dt).reshape(-1, width) for d in ds.descriptors])
            if len(desc) != frames.total:
                raise ValueError("one descriptor per keypoint")
            d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(frames.device)
        r = _run_logos(ctx, frames, d_desc, kind, ds.pairs, dictionary, logos_capacity, *tail)
        if trained is not None:
            r.update(dictionary=dictionary, dictionary_result=trained)
        return r
    if method != "gms":
        raise ValueError(f"unknown method {method!r}")
    frames = FrameTable(ctx, ds.frames, ds.sizes, device=device)
    do_match = (ds.descriptors is not None and len(ds.matches) == 0) if match is None else bool(match)
    if do_match and ds.descriptors is None:
        raise ValueError("the dataset carries no descriptors to match")
    descs = DescriptorTable(ctx, frames, ds.descriptors, ds.desc_kind) if do_match else None
    return _run_gms(ctx, frames, descs, ds.pairs, ds.matches, withRotation, withScale, thresholdFactor, *tail)


def _run_gms(ctx, frames, descs, src_pairs, matches, withRotation, withScale, thresholdFactor, camera, dist, prob, ransac_threshold, max_iters,
             reg=None):
    """The GMS flow on resident tables: putative matches (descs: a DescriptorTable, whose matcher gives every keypoint of frame_a one
    match -- BFMatcher::match without cross-check, FeatureMatchUtil.cpp:66-68; descs None: the host array `matches`, laid out by the
    pairs' match_off) -> gms_filter_device -> two-view with a camera. Returns run_dataset's record."""
    dev = frames.device
    pairs = np.ascontiguousarray(src_pairs, dtype=PAIR_DTYPE).copy()
    n_pairs = len(pairs)
    counts = np.diff(frames.frame_off_host)
    if descs is not None:
        table = pair_table(frame_pairs_of(pairs), counts[pairs["frame_a"]] if n_pairs else 0)
        pairs["m"], pairs["match_off"] = table["m"], table["match_off"]
    total_m = int((pairs["match_off"] + pairs["m"]).max()) if n_pairs else 0
    max_m = int(pairs["m"].max()) if n_pairs else 0
    d_pairs = _to_dev(pairs, dev) if n_pairs else torch.zeros(24, dtype=torch.uint8, device=dev)
    if descs is not None:
        d_matches = torch.zeros(max(total_m, 1) * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        descs.match_device(d_pairs.data_ptr(), n_pairs, max_m, d_matches.data_ptr())
    else:
        m_host = np.ascontiguousarray(matches, dtype=DMATCH_DTYPE)
        if total_m > len(m_host):
            raise ValueError("a pair's match range lies outside the dataset's match array")
        d_matches = _to_dev(m_host, dev) if len(m_host) else torch.zeros(16, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(max(total_m, 1) * 16, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(max(n_pairs, 1) * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.filter_device(frames.d_pts.data_ptr(), frames.d_frame_off.data_ptr(), frames.n_frames, d_pairs.data_ptr(), n_pairs, max_m,
                      d_matches.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), None, withRotation, withScale, thresholdFactor)
    out = dict(pairs=pairs)
    if camera is not None:
        out.update(_two_view(ctx, frames, d_pairs, n_pairs, max_m, total_m, d_out, d_res, camera, dist, prob, ransac_threshold, max_iters,
                             pairs, reg))
    ctx.synchronize()
    out.update(matches=d_matches.cpu().numpy().view(DMATCH_DTYPE)[:total_m], out=d_out.cpu().numpy().view(DMATCH_DTYPE)[:total_m],
               results=d_res.cpu().numpy().view(RESULT_DTYPE)[:n_pairs])
    return out


def _register_args(register, root, min_links, camera, bundle=False, ba=None, unique=False):
    """run_dataset's register / root / min_links / bundle / unique and the bundle adjustment's keywords -> None or (root, min_links,
    None or those keywords, unique), checked before anything is launched."""
    if bundle and not register:
        raise ValueError("bundle=True needs register=True: it refines the registration")
    if unique and not register:
        raise ValueError("unique=True needs register=True: it chooses the matches the registration builds its tracks from")
    if ba and not bundle:
        raise TypeError(f"unknown arguments {sorted(ba)} (the bundle adjustment's, without bundle=True)")
    if not register:
        return None
    if camera is None:
        raise ValueError("register=True needs a camera: it joins the two-view results")
    if int(min_links) < 1 or int(root) < 0:
        raise ValueError("root: a frame index; min_links: at least 1")
    if bundle:
        sfm_ba_params(**ba)   # (refuses an unknown keyword)
    return int(root), int(min_links), (dict(ba) if bundle else None), bool(unique)


def image_stack(images):
    """The argument checks of run_images, before anything is launched: `images` a host array or device tensor [n, H, W] (grey) or
    [n, H, W, 3] (B, G, R), or a list of equally sized [H, W] / [H, W, 3] images -> (uint8 array or tensor, is_bgr). Raises ValueError."""
    if isinstance(images, (list, tuple)):
        if len(images) == 0 or len({tuple(im.shape) for im in images}) != 1:
            raise ValueError("images: at least one image, all of one size and one channel count")
        images = torch.stack(list(images)) if torch.is_tensor(images[0]) else np.stack([np.asarray(im) for im in images])
    elif not torch.is_tensor(images):
        images = np.asarray(images)
    if images.ndim not in (3, 4) or (images.ndim == 4 and images.shape[3] != 3) or 0 in tuple(images.shape):
        raise ValueError("images: [n, H, W] grey or [n, H, W, 3] BGR")
    if images.dtype != (torch.uint8 if torch.is_tensor(images) else np.uint8):
        raise ValueError("images: 8-bit")
    return images, images.ndim == 4


def _train_dictionary_device(ctx, descs, opts):
    """_train_dictionary on a resident DescriptorTable: the rows go from tensor to tensor, the dictionary stays on the device for the
    word lookup -> (dictionary as a device tensor, as a host array for the record, its LOGOS_DICT_RESULT_DTYPE record)."""
    frames, kind = descs.frames, descs.kind
    dt, width = logos_dict_args(kind, opts["n_words"], opts["attempts"], opts["max_iters"])
    n_rows = int(frames.frame_off_host[1]) if opts["rows"] == "first" else frames.total
    if n_rows == 0:
        raise ValueError("method='logos' needs descriptors to train a dictionary on")
    job = LogosDictionary(ctx, kind, 1, n_rows, opts["n_words"], opts["attempts"], opts["max_iters"], opts["seed"], frames.device)
    nbytes = n_rows * width * np.dtype(dt).itemsize
    job.d_desc[:nbytes].copy_(descs.d_desc[:nbytes])
    job.d_set_off.copy_(torch.tensor([0, n_rows], dtype=torch.int64))
    torch.cuda.synchronize(frames.device)
    job.run()
    ctx.synchronize()
    dic, rec, _ = job.results()
    if rec[0]["status"] != 0:
        raise ValueError(f"train_dictionary: the training rows were refused (status {int(rec[0]['status'])}): at least n_words and at "
                         "most 2^20 rows, L2 elements finite and within [-4096, 4096]")
    return job.d_dict, dic[0], rec[0]


def run_images(ctx, images, camera=None, dist=None, method="gms", pairs=None, threshold=20, max_keypoints=10000, n_levels=8,
               descriptor="grad", withRotation=False, withScale=False, thresholdFactor=6.0, prob=0.7, ransac_threshold=1.0, max_iters=1000,
               device=None, dictionary=None, logos_capacity=None, cross_check=True, distance_coef=4.0, max_size=500, train_dictionary=None,
               keep_tables=False, detector="fast", contrast=128, refine=False, register=False, root=0, min_links=8, bundle=False, dense=False,
               min_disp16=16, dense_cap=None, dense_sgm=None, fuse=False, fuse_tol16=16, fuse_min_support=1, fuse_cap=None, dense_speckle=None,
               dense_poses="pair", dense_pairs=None, unique=False, **ba):
    """run_dataset from pixels. images: [n, H, W] grey or [n, H, W, 3] BGR, 8-bit, a host array or a device tensor (or a list of equally
    sized images). BGR goes through gms_bgr_to_gray_device; the pyramid keypoint source (threshold, max_keypoints, n_levels; detector
    "fast", or "dog" with `contrast` in the place of `threshold`: gms_detect_dog_batch_device, with refine=True
    gms_detect_dog_refined_batch_device; descriptor "grad" / "both": the 128-float rows under NORM_L2, "brief": the 32-byte rows under NORM_HAMMING) leaves its blocks on the
    device, gms_detect_pack_device puts them back to back, and the tables are built there: between the pixels and the results only the
    n + 1 frame offsets (and the status records the stages already read) come back. pairs: (frame_a, frame_b) rows or PAIR_DTYPE
    records; default every a < b. The other arguments and the returned records are run_dataset's (the matcher always runs: there are
    no matches to bring); keep_tables=True adds `tables` = (FrameTable, DescriptorTable), the resident keypoints and rows.
    register, root, min_links, bundle, unique and the bundle adjustment's keywords: run_dataset's.
    dense=True (needs a camera): adds `dense`, one entry per pair -- None for a pair without a pose or one that is not
    rectifiable, else a dict of points float32 [k, 3], colors uint8 [k] or [k, 3], pixel int32 [k], count and plan
    (gms_dense_pairs_device on the photographs themselves; min_disp16, dense_cap = the most points per pair, dense_sgm = the
    matcher's keywords). The points are in frame_a's frame and the pair's unit, as points3d; with register=True in the world frame,
    as points_world, and a pair the registration does not use has none. dense=False returns the dict without.
    dense_speckle = (max_speckle_size, max_diff16): the speckle filter on every pair's disparity map between the matcher and the
    cloud (gms_dense_pairs_filtered_device; max_diff16 in sixteenths of a pixel); each `dense` entry then also holds `removed`, and
    the fusion reads the filtered maps. None: no filter.
    fuse=True (needs dense=True and register=True: without a registration the clouds share no frame) adds
    `dense_fused`, the pairs' clouds fused into one by depth consistency (gms_dense_fuse_device on the maps, plans, views and scales
    still resident on the device): a dict of points float32 [k, 3], colors, source int32 [k] (an index into `pairs`), index int32 [k]
    (the point's index in that pair's `dense` entry), support and conflict uint8 [k] (the other pairs whose own disparity map agrees /
    disagrees with the point within fuse_tol16 sixteenths of a pixel, support counting the point's own pair) and counts int32
    [n_pairs + 1] (kept per pair, then the total). A point is kept once, by the lowest pair that sees it consistently, and only with
    support >= fuse_min_support; fuse_cap: the most points returned (default: room for all). `dense` itself is what it is without
    fuse; fuse=False returns the dict without `dense_fused`.
    dense_poses: where the dense stage and the fusion take a pair's pose and scale from. "pair", the default: the
    pair's own two-view record and the registration's scale, as ever. "registration" (needs register=True) / "bundle" (needs
    bundle=True): gms_sfm_pair_poses_device derives every pair's records from `views` / `views_ba`, the dense stage rectifies by them
    and its clouds and the fusion are in the frame of those views; the dict then also holds `dense_pose_records` = (two-view records,
    registration records) of the dense pairs, TWO_VIEW_DTYPE and SFM_PAIR_REG_DTYPE. dense_pairs = [(a, b), ...] (needs dense_poses
    other than "pair"): the frame pairs to match densely, in place of `pairs` -- any two registered frames, matched sparsely or not;
    `dense`, `dense_pose_records`, `dense_fused["source"]`, its counts and the fusion's neighbour table then index into dense_pairs,
    not into `pairs`. None: the sparse pair list."""
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}")
    if dense and camera is None:
        raise ValueError("dense=True needs a camera: it rectifies by the recovered poses")
    if fuse and not (dense and register):
        raise ValueError("fuse=True needs dense=True and register=True: without a registration the clouds share no frame")
    dense_pairs = check_dense_poses(dense_poses, dense_pairs, dense, register, bundle)
    if descriptor not in ("brief", "grad", "both"):
        raise ValueError('descriptor: "brief", "grad" or "both"')
    images, is_bgr = image_stack(images)
    n, h, w = images.shape[:3]
    reg = _register_args(register, root, min_links, camera, bundle, ba, unique)
    if reg is not None and not 0 <= reg[0] < n:
        raise ValueError("root: a frame index")
    if pairs is None:
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    src = np.asarray(pairs)
    src = src if src.dtype == PAIR_DTYPE else pair_table(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), 0)
    dev = _device(ctx, device)
    d_images = (images if torch.is_tensor(images) else torch.from_numpy(np.ascontiguousarray(images))).to(dev).contiguous()
    source = DetectPyramid(ctx, n, w, h, threshold, max_keypoints, n_levels, dev, descriptor, detector, contrast, refine)   # (refuses a bad size before any launch)
    d_photos = d_images
    if is_bgr:
        d_images = bgr_to_gray(ctx, d_images)
    torch.cuda.synchronize(dev)
    source.run(d_images)
    kind = GMS_DESC_HAMMING256 if descriptor == "brief" else GMS_DESC_L2_F32X128
    frames, descs = tables_from_detector(source, [(w, h)] * n, kind)
    tail = (camera, dist, prob, ransac_threshold, max_iters, reg)
    if method == "bf":
        r = _run_bf(ctx, descs, src, cross_check, distance_coef, max_size, *tail)
    elif method == "logos":
        trained = None
        if dictionary is None and train_dictionary not in (None, False):
            dictionary, dic_host, trained = _train_dictionary_device(ctx, descs, dictionary_training_options(train_dictionary))
        if dictionary is None:
            raise ValueError("method='logos' needs a dictionary, or train_dictionary")
        r = _run_logos(ctx, frames, descs.d_desc, kind, src, dictionary, logos_capacity, *tail)
        if trained is not None:
            r.update(dictionary=dic_host, dictionary_result=trained)
    else:
        r = _run_gms(ctx, frames, descs, src, None, withRotation, withScale, thresholdFactor, *tail)
    if dense:
        runs = [] if fuse else None       # (the runs' device buffers stay alive until the fusion has read them)
        rd = r
        if dense_poses != "pair":         # the dense stages' inputs from the chosen views instead of the pairs' own records
            rd = _dense_pose_records(ctx, r, dense_poses, dense_pairs, dev)
            r.update(dense_pose_records=(rd["two_view"], rd["registration"]))
        r.update(dense=_dense_pairs(ctx, d_photos, rd, camera, dist, min_disp16, dense_cap, dense_sgm, reg is not None, runs, dense_speckle))
        if fuse:
            r.update(dense_fused=_dense_fuse(ctx, runs, len(rd["pairs"]), 3 if d_photos.dim() == 4 else 1, fuse_tol16, fuse_min_support, fuse_cap))
    if keep_tables:
        r.update(tables=(frames, descs))
    return r


DENSE_POSES = ("pair", "registration", "bundle")


def check_dense_poses(dense_poses, dense_pairs, dense, register, bundle):
    """run_images' dense_poses / dense_pairs, refused before any device work -> dense_pairs as an int64 [n, 2] array, or None."""
    if dense_poses not in DENSE_POSES:
        raise ValueError(f"dense_poses: one of {DENSE_POSES}, not {dense_poses!r}")
    if dense_poses == "pair":
        if dense_pairs is not None:
            raise ValueError('dense_pairs needs dense_poses="registration" or "bundle": a pair the sparse stage did not match has no pose of its own')
        return None
    if not dense:
        raise ValueError(f"dense_poses={dense_poses!r} needs dense=True: it says where the dense stage takes its poses from")
    if dense_poses == "bundle" and not bundle:
        raise ValueError('dense_poses="bundle" needs bundle=True: it reads the bundle-adjusted views')
    if not register:
        raise ValueError(f"dense_poses={dense_poses!r} needs register=True: it reads the registration's views")
    if dense_pairs is None:
        return None
    fp = np.asarray(dense_pairs, dtype=np.int64)
    if fp.ndim != 2 or fp.shape[1] != 2 or len(fp) < 1 or (np.abs(fp) > 2 ** 31 - 1).any():
        raise ValueError("dense_pairs: (frame_a, frame_b) rows")
    return fp


def _dense_pose_records(ctx, r, dense_poses, dense_pairs, dev):
    """run_images' dense_poses other than "pair": gms_sfm_pair_poses_device on `views` or `views_ba` for the dense pairs (default: the
    sparse pair list's frames) -> what _dense_pairs and _dense_fuse read of `r`, with those records in the place of the pairs' own."""
    from .batch import pair_poses
    views = r["views_ba" if dense_poses == "bundle" else "views"]
    fp = np.stack([r["pairs"]["frame_a"], r["pairs"]["frame_b"]], 1).astype(np.int64) if dense_pairs is None else dense_pairs
    job = pair_poses(ctx, views, fp, dev)
    tv, reg = job.results()
    return dict(pairs=job.recs, two_view=tv, registration=reg, views=views)


def _dense_pairs(ctx, d_photos, r, camera, dist, min_disp16, cap, sgm, registered, keep=None, speckle=None):
    """run_images' dense=True: gms_dense_pairs_device for the pairs with a pose, one run per output size (the source's size, and its
    transpose for the pairs whose baseline is nearer the vertical), on the two-view records and the registration that `r` holds.
    keep: a list that gets (run, pair indices) of every run, for the fusion."""
    from .api import stereoRectify
    n, h, w = d_photos.shape[:3]
    channels = 3 if d_photos.dim() == 4 else 1
    pairs, tv = r["pairs"], r["two_view"]
    out = [None] * len(pairs)
    groups = {}
    for i in range(len(pairs)):
        if int(tv["status"][i]) != GMS_OK:
            continue
        plan = stereoRectify(camera, dist, tv["R"][i], tv["t"][i], (w, h))
        if plan.ok:
            groups.setdefault(plan.out_size, []).append(i)
    for size, idx in groups.items():
        run = DensePairs(ctx, len(idx), (w, h), size, camera, dist, channels, cap=cap, min_disp16=min_disp16, params=sgm, device=d_photos.device,
                         speckle=speckle)
        run.set_two_view(tv[idx])
        if registered:
            sub = pairs[idx].copy()
            run.set_registration(_to_dev(sub, d_photos.device), _to_dev(r["registration"][idx], d_photos.device),
                                 _to_dev(r["views"], d_photos.device), len(r["views"]))
        a = d_photos[torch.as_tensor(pairs["frame_a"][idx].astype(np.int64), device=d_photos.device)].contiguous()
        b = d_photos[torch.as_tensor(pairs["frame_b"][idx].astype(np.int64), device=d_photos.device)].contiguous()
        torch.cuda.synchronize(d_photos.device)
        run.run(a, b)
        ctx.synchronize()
        if keep is not None:
            keep.append((run, idx))
        counts, plans = run.d_count.cpu().numpy(), run.plans()
        removed = None if speckle is None else run.d_removed.cpu().numpy()
        for j, i in enumerate(idx):
            k = min(int(counts[j]), run.cap)
            colors = run.d_cloud_color[j, :k].cpu().numpy()
            out[i] = dict(points=run.d_xyz[j, :k].cpu().numpy(), colors=colors if channels == 3 else colors[:, 0],
                          pixel=run.d_pixel[j, :k].cpu().numpy(), count=int(counts[j]), plan=plans[j:j + 1])
            if removed is not None:
                out[i].update(removed=int(removed[j]))
    return out


def _dense_fuse(ctx, runs, n_pairs, channels, tol16, min_support, cap):
    """run_images' fuse=True: one gms_dense_fuse_device over the sources of every dense run, in the order of `pairs` (the pointer table
    joins the two size groups without a copy); `source` comes back as an index into `pairs`. No source: an empty cloud."""
    srcs = sorted(((i, s) for run, idx in runs for i, s in zip(idx, dense_fuse_sources(run))), key=lambda e: e[0])
    counts = np.zeros(n_pairs + 1, np.int32)
    if not srcs:
        return dict(points=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3) if channels == 3 else (0,), np.uint8), source=np.zeros(0, np.int32),
                    index=np.zeros(0, np.int32), support=np.zeros(0, np.uint8), conflict=np.zeros(0, np.uint8), counts=counts)
    pair_of = np.array([i for i, _ in srcs], np.int32)
    out = fuse_dense(ctx, [s for _, s in srcs], None, channels, tol16, min_support, cap)
    counts[pair_of], counts[-1] = out["counts"][:-1], out["counts"][-1]
    out.update(source=pair_of[out["source"]], counts=counts)
    return out


MAIN_SCENARIOS = ("normal", "rotated", "resized")   # frame 0 = the left image; frames 1, 2, 3 = the right image of each scenario


def run_main_scenarios(ctx, img1, img2, resize_to=(1000, 1000), angle=180, threshold=20, max_keypoints=10000, n_levels=8,
                       descriptor="grad", thresholdFactor=6.0, cross_check=True, distance_coef=4.0, max_size=500, camera=None, dist=None,
                       prob=0.7, ransac_threshold=1.0, max_iters=1000, device=None, detector="fast", contrast=128, refine=False):
    """The three feature-match scenarios of the reference's main() (main.cpp:28-47) from its two photographs: the pair as it is, the
    right image turned by `angle` degrees (img_rotate: getRotationMatrix2D + warpAffine) and the right image resized to `resize_to` =
    (width, height) (cv::resize). img1, img2: equally sized [H, W] grey or [H, W, 3] BGR images, host arrays or device tensors.
    The right image is transformed on the device (gms_warp_affine_device, gms_resize_device; BGR is transformed as BGR and then goes
    through gms_bgr_to_gray_device, as the reference transforms what imread gave it); one detector runs over left, right and the
    turned image, a second over the resized one; gms_detect_pack_device puts all four frames back to back, and ONE FrameTable /
    DescriptorTable with each frame's own size is built there -- between the pixels and the results only the 5 frame offsets (and the
    status records the stages read) come back. Each scenario then runs its pair (0, k) with method="bf" (bruteForceMatch) and with
    method="gms" at withRotation = withScale = True (FeatureMatchUtil.cpp:69). detector, refine and stage arguments: run_images'.
    Returns {"images": {"rotated", "resized"} (the transformed right images, of the kind that came in), "tables": (FrameTable,
    DescriptorTable), "sizes": the four (width, height), and per scenario name {"bf": record, "gms": record}, run_dataset's records}."""
    if descriptor not in ("brief", "grad", "both"):
        raise ValueError('descriptor: "brief", "grad" or "both"')
    pair, is_bgr = image_stack([img1, img2])
    on_dev = torch.is_tensor(pair)
    h, w = pair.shape[1:3]
    rw, rh = int(resize_to[0]), int(resize_to[1])
    dev = _device(ctx, device)
    d_pair = (pair if on_dev else torch.from_numpy(np.ascontiguousarray(pair))).to(dev).contiguous()
    ch = 3 if is_bgr else 1
    # (both detectors refuse a bad size before anything is launched)
    det3 = DetectPyramid(ctx, 3, w, h, threshold, max_keypoints, n_levels, dev, descriptor, detector, contrast, refine)
    det1 = DetectPyramid(ctx, 1, rw, rh, threshold, max_keypoints, n_levels, dev, descriptor, detector, contrast, refine)
    turn = Warp(ctx, 1, (w, h), (w, h), ch, 1, dev)
    shrink = Warp(ctx, 1, (w, h), (rw, rh), ch, 1, dev)
    turn.set_matrices(getRotationMatrix2D((w / 2., h / 2.), angle, 1.0))
    torch.cuda.synchronize(dev)
    d_right = d_pair[1:2]
    turn.warp_affine(d_right)
    shrink.resize(d_right)
    ctx.synchronize()
    d_three = torch.cat([d_pair, turn.d_dst])
    d_small = shrink.d_dst
    if is_bgr:
        d_three, d_small = bgr_to_gray(ctx, d_three), bgr_to_gray(ctx, d_small)
    # the two detectors write their blocks into one [4][max_keypoints] set, so that one pack run lays the four frames back to back
    slots = max(4 * det3.max_keypoints, 1)
    joint = SimpleNamespace(ctx=ctx, n=4, max_keypoints=det3.max_keypoints, w=w, h=h,
                            d_kp=torch.zeros(slots * 28, dtype=torch.uint8, device=dev),
                            d_desc=torch.zeros(slots * 32, dtype=torch.uint8, device=dev),
                            d_counts=torch.zeros(4, dtype=torch.int32, device=dev),
                            d_rows128=None if descriptor == "brief" else torch.zeros(slots * 128, dtype=torch.float32, device=dev))
    cut = 3 * det3.max_keypoints
    for det, lo, hi, c0, c1 in ((det3, 0, cut, 0, 3), (det1, cut, slots, 3, 4)):
        det.d_kp, det.d_desc, det.d_counts = joint.d_kp[lo * 28:hi * 28], joint.d_desc[lo * 32:hi * 32], joint.d_counts[c0:c1]
        if joint.d_rows128 is not None:
            det.d_rows128 = joint.d_rows128[lo * 128:hi * 128]
    torch.cuda.synchronize(dev)
    det3.run(d_three.contiguous())
    det1.run(d_small.contiguous())
    sizes = [(w, h)] * 3 + [(rw, rh)]
    kind = GMS_DESC_HAMMING256 if descriptor == "brief" else GMS_DESC_L2_F32X128
    frames, descs = tables_from_detector(joint, sizes, kind)
    tail = (camera, dist, prob, ransac_threshold, max_iters)
    images = {"rotated": turn.d_dst[0], "resized": shrink.d_dst[0]}
    out = {"images": images if on_dev else {k: v.cpu().numpy() for k, v in images.items()}, "tables": (frames, descs), "sizes": sizes}
    for k, name in enumerate(MAIN_SCENARIOS, start=1):
        src = pair_table(np.array([[0, k]], dtype=np.int64), 0)
        out[name] = {"bf": _run_bf(ctx, descs, src, cross_check, distance_coef, max_size, *tail),
                     "gms": _run_gms(ctx, frames, descs, src, None, True, True, thresholdFactor, *tail)}
    return out


def calibrate_images(ctx, images, board_size=(6, 9), max_candidates=256, device=None):
    """The reference's calibration (main.cpp:53-68): addChessboardPoints over the images, then calibrateCamera. images: [n, H, W] grey
    or [n, H, W, 3] BGR (through gms_bgr_to_gray_device), 8-bit, a host array, a device tensor or a list of equally sized images.
    ONE gms_chess_candidates_device launch covers all images and only the candidate records are read back; the boards are ordered on
    the host (gms_order_chessboard, the rule gms_find_chessboard_corners applies, here on the records); ONE
    gms_corner_subpix_device launch refines every found board's corners on the resident images; gms_calibrate_camera runs on the
    host. Images without a board are skipped, as the reference skips them.
    Returns {"found": bool [n], "successes", "image_points": [successes, nx * ny, 2], "object_points", "K", "dist", "rvecs", "tvecs",
    "rms", "camera": (fx, fy, cx, cy), "candidates": per image}; K and the rest are None when no board was found."""
    from .api import calibrateCamera, chessboardObjectPoints
    from .batch import ChessCorners, corner_subpix_images
    from .capi import load_library
    import ctypes as C
    stack, is_bgr = image_stack(images)
    dev = _device(ctx, device)
    d = (stack if torch.is_tensor(stack) else torch.from_numpy(np.ascontiguousarray(stack))).to(dev).contiguous()
    if is_bgr:
        d = bgr_to_gray(ctx, d)
    n, h, w = d.shape
    nx, ny = int(board_size[0]), int(board_size[1])
    if nx == ny or nx < 2 or ny < 2 or nx * ny > max_candidates:
        raise ValueError("board_size: (nx, ny) with nx != ny, both at least 2, nx * ny <= max_candidates")
    run = ChessCorners(ctx, n, w, h, max_candidates, dev)
    run.run(d)
    cands = run.candidates()
    lib = load_library()
    found, starts = np.zeros(n, bool), []
    for i, c in enumerate(cands):
        if len(c) < nx * ny:
            continue
        pts = np.ascontiguousarray(np.stack([c["x"][:nx * ny], c["y"][:nx * ny]], 1), dtype=np.float64)
        out = np.zeros_like(pts)
        ok = C.c_int(0)
        if lib.gms_order_chessboard(pts.ctypes.data, nx, ny, C.byref(ok), out.ctypes.data) != 0:
            raise ValueError("gms_order_chessboard: bad argument")
        if ok.value:
            found[i] = True
            starts.append(out)
    r = {"found": found, "successes": int(found.sum()), "candidates": cands, "image_points": np.zeros((0, nx * ny, 2)), "object_points": [],
         "K": None, "dist": None, "rvecs": None, "tvecs": None, "rms": None, "camera": None}
    if not starts:
        return r
    image_of = np.repeat(np.nonzero(found)[0], nx * ny)
    refined, status = corner_subpix_images(ctx, d, image_of, np.concatenate(starts))
    r["image_points"], r["subpix_status"] = refined.reshape(-1, nx * ny, 2), status.reshape(-1, nx * ny)
    r["object_points"] = [chessboardObjectPoints((nx, ny))] * len(starts)
    r["rms"], r["K"], r["dist"], r["rvecs"], r["tvecs"] = calibrateCamera(r["object_points"], list(r["image_points"]), (w, h))
    r["camera"] = (float(r["K"][0, 0]), float(r["K"][1, 1]), float(r["K"][0, 2]), float(r["K"][1, 2]))
    return r


def dictionary_training_options(train_dictionary):
    """run_dataset's train_dictionary= as a full dict: True, or a dict with any of rows ("first": frame 0's descriptors, as the
    reference trains on desc1; "all": every frame's, as one set), n_words, attempts, max_iters, seed."""
    opts = {"rows": "first", "n_words": 50, "attempts": 3, "max_iters": 100, "seed": 0}
    if train_dictionary is not True:
        given = dict(train_dictionary)
        unknown = set(given) - set(opts)
        if unknown:
            raise ValueError(f"train_dictionary: unknown keys {sorted(unknown)}")
        opts.update(given)
    if opts["rows"] not in ("first", "all"):
        raise ValueError("train_dictionary: rows is 'first' or 'all'")
    return opts


def _train_dictionary(ctx, ds, opts, device):
    """-> (dictionary, its LOGOS_DICT_RESULT_DTYPE record), trained on the dataset's descriptors; a set outside the domain raises."""
    if ds.descriptors is None or len(ds.descriptors) == 0:
        raise ValueError("method='logos' needs the dataset's descriptors and a dictionary")
    kind = int(ds.desc_kind)
    dt, width = logos_dict_args(kind, opts["n_words"], opts["attempts"], opts["max_iters"])
    rows = [np.ascontiguousarray(d, dtype=dt).reshape(-1, width) for d in ds.descriptors]
    train = rows[0] if opts["rows"] == "first" else np.concatenate(rows)
    dic, rec, _ = logos_dictionary(ctx, [train], kind, opts["n_words"], opts["attempts"], opts["max_iters"], opts["seed"], device)
    if rec[0]["status"] != 0:
        raise ValueError(f"train_dictionary: the training rows were refused (status {int(rec[0]['status'])}): at least n_words and at "
                         "most 2^20 rows, L2 elements finite and within [-4096, 4096]")
    return dic[0], rec[0]


def _run_logos(ctx, frames, d_desc, kind, src_pairs, dictionary, capacity, camera, dist, prob, ransac_threshold, max_iters, reg=None):
    """The LOGOS flow on resident tables: the rows d_desc (a device tensor, row i of keypoint i of `frames`; None without keypoints)
    -> words (the exact nearest row of `dictionary`, a host array or a device tensor of rows like the descriptors) -> one LOGOS table
    for all frames -> every pair in one filter run -> two-view with a camera. Pair p gets room for `capacity` survivors (default: the
    larger of its two frames); pairs that overflow are reported with the count they need, and the batch is run once more with that
    room. Returns what run_dataset returns (`matches` empty: LOGOS has no putative matches), plus words (per keypoint) and
    logos_results (LOGOS_RESULT_DTYPE per pair); `results` are gms_pair_result records, `pairs` the table the survivors are laid out
    by."""
    dev = frames.device
    dt, width = desc_layout(kind)
    if torch.is_tensor(dictionary):
        d_dict = dictionary.contiguous().view(torch.uint8).reshape(-1)
        n_words = d_dict.numel() // (width * np.dtype(dt).itemsize)
    else:
        dic = np.ascontiguousarray(dictionary, dtype=dt).reshape(-1, width)
        d_dict, n_words = torch.from_numpy(dic.view(np.uint8).reshape(-1).copy()).to(dev), len(dic)
    total_kp = frames.total
    if total_kp:
        if d_desc is None or d_desc.numel() * d_desc.element_size() < total_kp * width * np.dtype(dt).itemsize:
            raise ValueError("one descriptor per keypoint")
        d_words = torch.zeros(total_kp, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.logos_words_device(kind, d_desc.data_ptr(), total_kp, d_dict.data_ptr(), n_words, d_words.data_ptr())
    else:
        d_words = torch.zeros(1, dtype=torch.int32, device=dev)
    table = LogosTable(ctx, frames, d_words, n_words)
    src = frame_pairs_of(np.ascontiguousarray(src_pairs, dtype=PAIR_DTYPE))
    n_pairs = len(src)
    counts = np.diff(frames.frame_off_host)
    cap = (np.maximum(frame_counts(counts, src[:, 0]), frame_counts(counts, src[:, 1])) if capacity is None
           else np.full(n_pairs, int(capacity), np.int64))
    for attempt in range(2):
        pairs = pair_table(src, cap)
        job = LogosFilter(ctx, table, pairs)
        if n_pairs:
            job.run()
        ctx.synchronize()
        lres = job.logos_results()
        over = lres["status"] == GMS_ERR_CAPACITY
        if attempt or not over.any():
            break
        cap = np.where(over, lres["n_out"], cap).astype(np.int64)   # room for what the overflowing pairs reported
    total_m = job.out_len
    out = dict(pairs=pairs, logos_results=lres, words=d_words.cpu().numpy()[:total_kp])
    if camera is not None:
        out.update(_two_view(ctx, frames, job.d_pairs, n_pairs, int(cap.max()) if n_pairs else 0, total_m, job.d_out, job.d_pres, camera,
                             dist, prob, ransac_threshold, max_iters, pairs, reg))
    res_out, _, pres = job.results()
    out.update(matches=np.zeros(0, DMATCH_DTYPE), out=res_out, results=pres)
    return out


def _run_bf(ctx, descs, src_pairs, cross_check, distance_coef, max_size, camera, dist, prob, ransac_threshold, max_iters, reg=None):
    """The bruteForceMatch flow on a resident DescriptorTable: every pair's survivors in one gms_bf_select_device run -> two-view with
    a camera. Pair p gets room for min(max_size, n(frame_a)) survivors, which its K never exceeds. Returns what run_dataset returns
    (`matches` empty: the putative matches stay in the workspace), plus bf_results (BF_RESULT_DTYPE per pair); `results` are
    gms_pair_result records, `pairs` the table the survivors are laid out by."""
    frames = descs.frames
    src = np.ascontiguousarray(src_pairs, dtype=PAIR_DTYPE)
    n_pairs = len(src)
    pairs = bf_select_table(descs, frame_pairs_of(src), max_size=max_size)
    run = BfSelect(ctx, descs, pairs, cross_check, distance_coef, max_size)
    if n_pairs:
        run.run()
    ctx.synchronize()
    total_m = run.out_len
    max_m = int(pairs["m"].max()) if n_pairs else 0
    out = dict(pairs=pairs)
    if camera is not None:
        out.update(_two_view(ctx, frames, run.d_pairs, n_pairs, max_m, total_m, run.d_out, run.d_pres, camera, dist, prob,
                             ransac_threshold, max_iters, pairs, reg))
    res_out, bf_res, pres = run.results()
    out.update(matches=np.zeros(0, DMATCH_DTYPE), out=res_out[:total_m], results=pres, bf_results=bf_res)
    return out
