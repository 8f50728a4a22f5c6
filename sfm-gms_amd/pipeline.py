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

torch here is device memory only; every stage is a call into csrc/libgms_hip.so. Used by tools/gms_filter_file.py and the tests."""
import numpy as np
import torch

from .batch import (BfSelect, DescriptorTable, FrameTable, LogosFilter, LogosTable, _to_dev, _words_device, bf_select_table, frame_counts,
                    frame_pairs_of, logos_dictionary, pair_table)
from .api import logos_dict_args
from .types import DMATCH_DTYPE, GMS_ERR_CAPACITY, PAIR_DTYPE, RESULT_DTYPE, TWO_VIEW_DTYPE, desc_layout, make_camera


def _two_view(ctx, frames, d_pairs, n_pairs, max_m, total_m, d_out, d_res, camera, dist, prob, ransac_threshold, max_iters):
    """gms_two_view_batch_device on the survivors d_out and their gms_pair_result records d_res, laid out by the pair table d_pairs ->
    the two-view part of run_dataset's result: two_view, coords1, coords2, mask, points3d as host arrays."""
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
    ctx.synchronize()
    return dict(two_view=d_tv.cpu().numpy().view(TWO_VIEW_DTYPE)[:n_pairs], coords1=d_c1.cpu().numpy().reshape(-1, 2)[:total_m],
                coords2=d_c2.cpu().numpy().reshape(-1, 2)[:total_m], mask=d_mask.cpu().numpy()[:total_m],
                points3d=d_p3.cpu().numpy().reshape(-1, 3)[:total_m])


def run_dataset(ctx, ds, withRotation=False, withScale=False, thresholdFactor=6.0, match=None, camera=None, dist=None, prob=0.7,
                ransac_threshold=1.0, max_iters=1000, device="cuda:0", method="gms", dictionary=None, logos_capacity=None,
                cross_check=True, distance_coef=4.0, max_size=500, train_dictionary=None):
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
    4.0 / 500 by default); see _run_bf."""
    if method == "bf":
        return _run_bf(ctx, ds, cross_check, distance_coef, max_size, camera, dist, prob, ransac_threshold, max_iters, device)
    if method == "logos":
        trained = None
        if dictionary is None and train_dictionary not in (None, False):
            dictionary, trained = _train_dictionary(ctx, ds, dictionary_training_options(train_dictionary), device)
        r = _run_logos(ctx, ds, dictionary, logos_capacity, camera, dist, prob, ransac_threshold, max_iters, device)
        if trained is not None:
            r.update(dictionary=dictionary, dictionary_result=trained)
        return r
    if method != "gms":
        raise ValueError(f"unknown method {method!r}")
    frames = FrameTable(ctx, ds.frames, ds.sizes, device=device)
    dev = frames.device
    pairs = np.ascontiguousarray(ds.pairs, dtype=PAIR_DTYPE).copy()
    n_pairs = len(pairs)
    counts = np.diff(frames.frame_off_host)
    do_match = (ds.descriptors is not None and len(ds.matches) == 0) if match is None else bool(match)
    if do_match:
        if ds.descriptors is None:
            raise ValueError("the dataset carries no descriptors to match")
        # BFMatcher::match without cross-check: one match per keypoint of the query frame (FeatureMatchUtil.cpp:66-68)
        table = pair_table(frame_pairs_of(pairs), counts[pairs["frame_a"]] if n_pairs else 0)
        pairs["m"], pairs["match_off"] = table["m"], table["match_off"]
    total_m = int((pairs["match_off"] + pairs["m"]).max()) if n_pairs else 0
    max_m = int(pairs["m"].max()) if n_pairs else 0
    d_pairs = _to_dev(pairs, dev) if n_pairs else torch.zeros(24, dtype=torch.uint8, device=dev)
    if do_match:
        descs = DescriptorTable(ctx, frames, ds.descriptors, ds.desc_kind)
        d_matches = torch.zeros(max(total_m, 1) * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        descs.match_device(d_pairs.data_ptr(), n_pairs, max_m, d_matches.data_ptr())
    else:
        m_host = np.ascontiguousarray(ds.matches, dtype=DMATCH_DTYPE)
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
        out.update(_two_view(ctx, frames, d_pairs, n_pairs, max_m, total_m, d_out, d_res, camera, dist, prob, ransac_threshold, max_iters))
    ctx.synchronize()
    out.update(matches=d_matches.cpu().numpy().view(DMATCH_DTYPE)[:total_m], out=d_out.cpu().numpy().view(DMATCH_DTYPE)[:total_m],
               results=d_res.cpu().numpy().view(RESULT_DTYPE)[:n_pairs])
    return out


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


def _run_logos(ctx, ds, dictionary, capacity, camera, dist, prob, ransac_threshold, max_iters, device):
    """descriptors -> words (the exact nearest dictionary row) -> one LOGOS table for all frames -> every pair in one filter run ->
    two-view with a camera. Pair p gets room for `capacity` survivors (default: the larger of its two frames); pairs that overflow
    are reported with the count they need, and the batch is run once more with that room. Returns what run_dataset returns
    (`matches` empty: LOGOS has no putative matches), plus words (per keypoint) and logos_results (LOGOS_RESULT_DTYPE per pair);
    `results` are gms_pair_result records, `pairs` the table the survivors are laid out by."""
    if ds.descriptors is None or dictionary is None:
        raise ValueError("method='logos' needs the dataset's descriptors and a dictionary")
    frames = FrameTable(ctx, ds.frames, ds.sizes, device=device)
    dev = frames.device
    kind = int(ds.desc_kind)
    dt, width = desc_layout(kind)
    dic = np.ascontiguousarray(dictionary, dtype=dt).reshape(-1, width)
    total_kp = frames.total
    if total_kp:
        desc = np.concatenate([np.ascontiguousarray(d, dtype=dt).reshape(-1, width) for d in ds.descriptors])
        if len(desc) != total_kp:
            raise ValueError("one descriptor per keypoint")
        d_words, held = _words_device(ctx, kind, desc, dic, dev)   # (held: the launch's inputs, alive until this function returns)
    else:
        d_words = torch.zeros(1, dtype=torch.int32, device=dev)
    table = LogosTable(ctx, frames, d_words, len(dic))
    src = frame_pairs_of(np.ascontiguousarray(ds.pairs, dtype=PAIR_DTYPE))
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
                             dist, prob, ransac_threshold, max_iters))
    res_out, _, pres = job.results()
    out.update(matches=np.zeros(0, DMATCH_DTYPE), out=res_out, results=pres)
    return out


def _run_bf(ctx, ds, cross_check, distance_coef, max_size, camera, dist, prob, ransac_threshold, max_iters, device):
    """descriptors -> every pair's bruteForceMatch survivors in one gms_bf_select_device run -> two-view with a camera. Pair p gets
    room for min(max_size, n(frame_a)) survivors, which its K never exceeds. Returns what run_dataset returns (`matches` empty: the
    putative matches stay in the workspace), plus bf_results (BF_RESULT_DTYPE per pair); `results` are gms_pair_result records,
    `pairs` the table the survivors are laid out by."""
    if ds.descriptors is None:
        raise ValueError("method='bf' needs the dataset's descriptors")
    frames = FrameTable(ctx, ds.frames, ds.sizes, device=device)
    descs = DescriptorTable(ctx, frames, ds.descriptors, ds.desc_kind)
    src = np.ascontiguousarray(ds.pairs, dtype=PAIR_DTYPE)
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
                             ransac_threshold, max_iters))
    res_out, bf_res, pres = run.results()
    out.update(matches=np.zeros(0, DMATCH_DTYPE), out=res_out[:total_m], results=pres, bf_results=bf_res)
    return out
