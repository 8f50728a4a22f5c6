#!/usr/bin/env python3
"""The reference's structureFromMotion (SfMUtil.cpp:4-83, main.cpp:71-75) on two photographs, every stage on the GPU
(structureFromMotion in sfm-gms_amd/api.py -> pipeline.run_images): pixels -> keypoints and rows -> the method's matches ->
findEssentialMat(RANSAC, 0.7, 1.0) -> recoverPose -> undistort + triangulate. Prints one JSON line: pose, point count, reprojection RMS.

    python tools/gms_sfm_pair.py [pair.npz] [--method gms|bf|logos] [--max-keypoints 10000] [--threshold 20] [--levels 8] [--detector fast|dog] [--contrast 128] [--refine] [--bgr] [--check] [--camera camera.npz] [--out x.npz]

pair.npz: arrays left, right ([H, W] grey or [H, W, 3] BGR, uint8) and camera = (fx, fy, cx, cy), optionally dist = (k1, k2, p1, p2, k3);
default: the committed pair of the reference's SourceImages, tests/golden/image_sfm_pair_1008x756.npz (its camera is stated, not
calibrated). --camera: a file with camera (and optionally dist), as tools/gms_calibrate.py --out writes it, in place of the pair's own:
the committed calibration photographs have the pair's scale, so their calibration applies to it. --bgr: hand the grey images over
as three equal channels (the BGR entry, gms_bgr_to_gray_device). --detector dog: difference-of-Gaussians keypoints with
--contrast in 1/256 grey level in the place of --threshold; --refine: its keypoints refined to 1/16 pixel and 1/16 layer. --check (method gms): runs the CPU statements (tests/sfm_images_ref.py; with
--detector dog tests/dog_ref.py's detector, with --refine tests/dog_refine_ref.py's, in front of them) beside it and compares every stage; test infrastructure, about ten seconds."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pair", nargs="?", default=os.path.join(ROOT, "tests", "golden", "image_sfm_pair_1008x756.npz"))
    ap.add_argument("--method", choices=("gms", "bf", "logos"), default="logos")
    ap.add_argument("--max-keypoints", type=int, default=10000)
    ap.add_argument("--threshold", type=int, default=20)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--detector", choices=("fast", "dog"), default="fast")
    ap.add_argument("--contrast", type=int, default=128)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--bgr", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--camera")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.refine and a.detector != "dog":
        ap.error("--refine needs --detector dog")
    pkg = importlib.import_module("sfm-gms_amd")
    z = np.load(a.pair)
    left, right = np.ascontiguousarray(z["left"], dtype=np.uint8), np.ascontiguousarray(z["right"], dtype=np.uint8)
    camera = tuple(float(v) for v in z["camera"])
    dist = tuple(float(v) for v in z["dist"]) if "dist" in z.files else None
    if a.camera:
        zc = np.load(a.camera)
        camera = tuple(float(v) for v in zc["camera"])
        dist = tuple(float(v) for v in zc["dist"]) if "dist" in zc.files else None
    imgs = [np.ascontiguousarray(np.stack([im] * 3, axis=2)) for im in (left, right)] if a.bgr and left.ndim == 2 else [left, right]
    kw = dict(method=a.method, max_keypoints=a.max_keypoints, threshold=a.threshold, n_levels=a.levels, detector=a.detector, contrast=a.contrast, refine=a.refine)
    t0 = time.perf_counter()
    r = pkg.structureFromMotion(*imgs, camera, dist, **kw)
    ms = (time.perf_counter() - t0) * 1e3
    tv = r["two_view"]
    n_pose = int((r["mask"] != 0).sum())
    rms = float(np.sqrt((tv["sum_sq_err1"] + tv["sum_sq_err2"]) / (2 * max(n_pose, 1))) * (camera[0] + camera[1]) / 2)
    line = {"image": [int(left.shape[1]), int(left.shape[0])], "input": "bgr" if imgs[0].ndim == 3 else "grey", "method": a.method,
            "camera": [round(v, 4) for v in camera], "dist": None if dist is None else [round(v, 6) for v in dist],
            "detector": a.detector, "refine": a.refine, "max_keypoints": a.max_keypoints, "keypoints": [len(r["keypoints1"]), len(r["keypoints2"])], "survivors": len(r["matches"]),
            "ransac_inliers": int(tv["n_ransac"]), "ransac_iterations": int(tv["ransac_iters"]), "after_recover_pose": int(tv["n_pose"]),
            "points": len(r["points3D"]), "behind_a_camera": int(tv["n_behind"]), "reprojection_rms_px": round(rms, 4),
            "t": [round(float(v), 4) for v in r["t"]], "R": [[round(float(v), 5) for v in row] for row in r["R"]],
            "first_call_ms": round(ms, 2)}
    ok = True
    if a.check:
        if a.method != "gms" or left.ndim != 2:
            ap.error("--check restates method gms on grey images")
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gms_oracle as oracle
        import sfm_images_ref
        if a.detector == "dog":
            import dog_refine_ref
            c = dog_refine_ref.sfm_chain(oracle, left, right, camera, a.contrast, a.max_keypoints, a.levels, refine=a.refine)
        else:
            c = sfm_images_ref.chain(oracle, left, right, camera, a.max_keypoints, a.threshold, a.levels)
        ref = c["two_view"]
        n_ref = int((ref["mask"] != 0).sum())
        chk = {"keypoints": r["keypoints1"].tobytes() == c["keypoints"][0].tobytes() and r["keypoints2"].tobytes() == c["keypoints"][1].tobytes(),
               "matches": r["detail"]["matches"].tobytes() == c["matches"].tobytes(), "survivors": r["matches"].tobytes() == c["survivors"].tobytes(),
               "ransac": int(tv["ransac_iters"]) == ref["iters"] and int(tv["n_ransac"]) == ref["n_ransac"],
               "mask": bool(np.array_equal(r["mask"], ref["mask"])),
               "pose_1e-9": bool(max(np.abs(r["E"] - ref["E"]).max(), np.abs(r["R"] - ref["R"]).max(), np.abs(r["t"] - ref["t"]).max()) < 1e-9),
               "points": r["points3D"].shape == ref["points"].shape and bool(np.allclose(r["points3D"], ref["points"], rtol=1e-6, atol=1e-9))}
        line["check_vs_cpu"] = {k: bool(v) for k, v in chk.items()}
        line["cpu"] = {"survivors": len(c["survivors"]), "ransac_inliers": ref["n_ransac"], "after_recover_pose": ref["n_pose"], "behind_a_camera": ref["behind"],
                       "reprojection_rms_px": round(float(np.sqrt((ref["sum_sq_err1"] + ref["sum_sq_err2"]) / (2 * max(n_ref, 1))) * (camera[0] + camera[1]) / 2), 4),
                       "t": [round(float(v), 4) for v in ref["t"]]}
        ok = all(chk.values())
    if a.out:
        np.savez_compressed(a.out, **{k: r[k] for k in ("points3D", "R", "t", "E", "matches", "mask", "keypoints1", "keypoints2")})
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
