#!/usr/bin/env python3
"""tools/gms_filter_file.py -- a GMSFRM01 dataset file (include/gms.h "ingest format") to filtered matches on the GPU:

    python tools/gms_filter_file.py seq.gmsf [--rot] [--scale] [--thr 6.0] [--match] [--camera fx fy cx cy] [--dist k1 k2 p1 p2 k3]
                                             [--prob 0.7] [--ransac-threshold 1.0] [--out result.npz]
                                             [--logos DICT.npy | --logos-train N [--logos-train-rows first|all] [--logos-seed S]] [--logos-capacity N]
                                             [--bf [--bf-coef 4.0] [--bf-max 500] [--no-cross-check]]

The file is read by the library's C reader (gms_dataset_read); with descriptors and no matches in it (or --match) the putative
matches come from gms_bfmatch_device (FeatureMatchUtil.cpp:66-68), then gms_filter_device (matchGMS, FeatureMatchUtil.cpp:69), and
with --camera the two-view stage of structureFromMotion (SfMUtil.cpp:25-82: findEssentialMat, recoverPose, undistort + triangulate).
--logos DICT.npy runs the reference's SIFT_matchLOGOS flow instead (FeatureMatchUtil.cpp:86-131): the file's descriptors get their
visual words from the dictionary (its rows like the descriptors: [k, 128] float32 or [k, 32] uint8), then LOGOS filters every pair of
the file (gms_logos_filter_device), then the two-view stage as above. --logos-train N trains the dictionary of N words first
(gms_logos_dict_train_device: deterministic k-means, not OpenCV's dictionary) on frame 0's descriptors, as the reference clusters
desc1, or on every frame's with --logos-train-rows all.
--bf runs the reference's DEFAULT_SIFT flow (bruteForceMatch, FeatureMatchUtil.cpp:20-31): cross-checked brute-force matches of every
pair, sorted by distance, kept within --bf-coef times the smallest distance and at most --bf-max (gms_bf_select_device), then the
two-view stage as above; --no-cross-check for the reference's match() helper.
Prints one JSON line; --out keeps every array (numpy .npz)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--rot", action="store_true")
    ap.add_argument("--scale", action="store_true")
    ap.add_argument("--thr", type=float, default=6.0)
    ap.add_argument("--match", action="store_true", help="brute-force match the descriptors even if the file holds matches")
    ap.add_argument("--camera", type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"))
    ap.add_argument("--dist", type=float, nargs=5, metavar=("K1", "K2", "P1", "P2", "K3"))
    ap.add_argument("--prob", type=float, default=0.7, help="findEssentialMat's confidence (SfMUtil.cpp:39 passes 0.7)")
    ap.add_argument("--ransac-threshold", type=float, default=1.0)
    ap.add_argument("--out")
    ap.add_argument("--logos", metavar="DICT.npy", help="LOGOS with this visual-word dictionary instead of GMS")
    ap.add_argument("--logos-train", type=int, metavar="N", help="LOGOS with a dictionary of N words trained on the file's descriptors")
    ap.add_argument("--logos-train-rows", choices=("first", "all"), default="first", help="train on frame 0's rows (default) or on all")
    ap.add_argument("--logos-seed", type=int, default=0)
    ap.add_argument("--logos-capacity", type=int, help="survivors per pair before a rerun (default: the larger frame)")
    ap.add_argument("--bf", action="store_true", help="bruteForceMatch (cross-check, sort, ratio prune) instead of GMS")
    ap.add_argument("--bf-coef", type=float, default=4.0, help="kDistanceCoef: keep d <= coef * d_min")
    ap.add_argument("--bf-max", type=int, default=500, help="kMaxMatchingSize: at most this many survivors per pair")
    ap.add_argument("--no-cross-check", action="store_true", help="plain forward matches (the reference's match() helper)")
    a = ap.parse_args()
    if a.logos and a.logos_train is not None:
        ap.error("--logos DICT.npy and --logos-train N exclude each other")
    pkg = importlib.import_module("sfm-gms_amd")
    io = importlib.import_module("sfm-gms_amd.io")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    ds = io.load_c(a.path)
    with pkg.GmsContext(0) as ctx:
        if a.bf:
            r = pipeline.run_dataset(ctx, ds, camera=a.camera, dist=a.dist, prob=a.prob, ransac_threshold=a.ransac_threshold, method="bf",
                                     cross_check=not a.no_cross_check, distance_coef=a.bf_coef, max_size=a.bf_max)
        elif a.logos or a.logos_train is not None:
            train = None if a.logos else {"n_words": a.logos_train, "rows": a.logos_train_rows, "seed": a.logos_seed}
            r = pipeline.run_dataset(ctx, ds, camera=a.camera, dist=a.dist, prob=a.prob, ransac_threshold=a.ransac_threshold,
                                     method="logos", dictionary=np.load(a.logos) if a.logos else None, logos_capacity=a.logos_capacity,
                                     train_dictionary=train)
        else:
            r = pipeline.run_dataset(ctx, ds, a.rot, a.scale, a.thr, match=True if a.match else None, camera=a.camera, dist=a.dist,
                                     prob=a.prob, ransac_threshold=a.ransac_threshold)
    res = r["results"]
    line = {"file": a.path, "frames": len(ds.frames), "pairs": len(res), "matches": int(r["pairs"]["m"].sum()),
            "kept": int(res["n_inliers"][res["status"] == 0].sum()), "failed_pairs": int((res["status"] != 0).sum()),
            "flags": [a.rot, a.scale, a.thr]}
    if a.bf:
        br = r["bf_results"]
        line.update(method="bf", matches=None, candidates=int(br["n_candidates"].sum()), within_ratio=int(br["n_ratio"].sum()),
                    flags=[not a.no_cross_check, a.bf_coef, a.bf_max])
    elif a.logos or a.logos_train is not None:
        lr = r["logos_results"]
        line.update(method="logos", matches=None, candidates=int(lr["n_candidates"].sum()), supported=int(lr["n_supported"].sum()))
        if "dictionary_result" in r:
            dr = r["dictionary_result"]
            line.update(dictionary={"words": int(a.logos_train), "attempt": int(dr["attempt"]), "iterations": int(dr["iterations"]),
                                    "compactness": int(dr["compactness"]), "empty_clusters": int(dr["empty_clusters"])})
    if "two_view" in r:
        tv = r["two_view"]
        ok = tv["status"] == 0
        fin = np.maximum(tv["n_finite"][ok], 1)
        line.update(two_view_ok=int(ok.sum()), ransac_inliers=int(tv["n_ransac"][ok].sum()), pose_inliers=int(tv["n_pose"][ok].sum()),
                    triangulated=int(tv["n_triangulated"][ok].sum()),
                    reprojection_rms=[float(np.sqrt((tv["sum_sq_err1"][ok] / fin).mean())) if ok.any() else None,
                                      float(np.sqrt((tv["sum_sq_err2"][ok] / fin).mean())) if ok.any() else None])
    if a.out:
        np.savez(a.out, **r)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
