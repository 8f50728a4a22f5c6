#!/usr/bin/env python3
"""A dense, coloured cloud from two photographs and a camera: structureFromMotion recovers the pose, denseStereo
rectifies by it, runs semi-global matching and reprojects every matched pixel into camera 1's frame; the cloud is written as a PLY
file on the host. Prints one JSON line: the turn chosen, the share of rectified pixels that are valid, the dense point count beside
the sparse cloud's, and the median distance (in the pair's unit, |t| = 1) from each sparse triangulated point to the dense point at
its rectified pixel.

    python tools/gms_dense_pair.py [pair.npz] [--method gms|bf|logos] [--max-keypoints 10000] [--num-disparities 128] [--min-disp16 16] [--speckle SIZE,DIFF16] [--check] [--ply cloud.ply]

pair.npz: arrays left, right ([H, W] grey or [H, W, 3] BGR, uint8) and camera = (fx, fy, cx, cy), optionally dist; default: the
committed pair of the reference's SourceImages, tests/golden/image_sfm_pair_1008x756.npz (its camera is stated, not calibrated).
--check: the numpy statement (tests/rectify_ref.py) beside it: the plan, both rectified images, the valid plane and the cloud of the
stage's own disparity map must be equal byte for byte (the matcher has its own check, tools/stereo_sgm_bench.py --check).
--speckle SIZE,DIFF16: filterSpeckles on the matcher's map before the reprojection (DIFF16 in sixteenths of a
pixel); the line then states the pixels removed, and --check also runs the stage without the filter and compares the filtered map
with the numpy statement (tests/speckle_ref.py) of the unfiltered one."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_ply(path, points, colors):
    colors = np.asarray(colors)
    rgb = np.repeat(colors[:, None], 3, axis=1) if colors.ndim == 1 else colors[:, ::-1]       # BGR -> RGB
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(points)}\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode())
        rec = np.zeros(len(points), np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))]))
        rec["p"], rec["c"] = points, rgb
        f.write(rec.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pair", nargs="?", default=os.path.join(ROOT, "tests", "golden", "image_sfm_pair_1008x756.npz"))
    ap.add_argument("--method", choices=("gms", "bf", "logos"), default="gms")
    ap.add_argument("--max-keypoints", type=int, default=10000)
    ap.add_argument("--num-disparities", type=int, default=128)
    ap.add_argument("--min-disp16", type=int, default=16)
    ap.add_argument("--speckle", help="SIZE,DIFF16")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--ply")
    a = ap.parse_args()
    pkg = importlib.import_module("sfm-gms_amd")
    z = np.load(a.pair)
    left, right = np.ascontiguousarray(z["left"], dtype=np.uint8), np.ascontiguousarray(z["right"], dtype=np.uint8)
    camera = tuple(float(v) for v in z["camera"])
    dist = tuple(float(v) for v in z["dist"]) if "dist" in z.files else None
    sfm = pkg.structureFromMotion(left, right, camera, dist, method=a.method, max_keypoints=a.max_keypoints)
    line = {"image": [int(left.shape[1]), int(left.shape[0])], "method": a.method, "t": [round(float(v), 4) for v in sfm["t"]],
            "sparse_points": len(sfm["points3D"])}
    plan = pkg.stereoRectify(camera, dist, sfm["R"], sfm["t"], (left.shape[1], left.shape[0]))
    line.update(rectifiable=plan.ok, turn=int(plan["turn"]), out_size=list(plan.out_size), baseline=round(float(plan["B"]), 6))
    if not plan.ok:
        print(json.dumps(line))
        return 1
    speckle = tuple(int(v) for v in a.speckle.split(",")) if a.speckle else None
    r = pkg.denseStereo(left, right, camera, dist, sfm["R"], sfm["t"], min_disp16=a.min_disp16, num_disparities=a.num_disparities, speckle=speckle)
    ow, oh = plan.out_size
    line.update(valid_share=round(float((r["valid"] != 0).mean()), 4), dense_points=int(r["count"]))
    if speckle:
        line.update(speckle=list(speckle), speckle_removed=int(r["removed"]))
    # every sparse point at its rectified pixel: the dense point there, when there is one
    X = np.asarray(sfm["points3D"], dtype=np.float64)
    p = X @ plan["R1"].T
    front = p[:, 2] > 0
    u = np.rint(plan["fx"] * p[front, 0] / p[front, 2] + plan["cx"]).astype(np.int64)
    v = np.rint(plan["fy"] * p[front, 1] / p[front, 2] + plan["cy"]).astype(np.int64)
    inside = (u >= 0) & (u < ow) & (v >= 0) & (v < oh)
    index = np.full(ow * oh, -1, np.int64)
    index[r["pixel"]] = np.arange(len(r["pixel"]))
    at = index[(v[inside] * ow + u[inside])]
    have = at >= 0
    d = np.linalg.norm(X[front][inside][have] - r["points"][at[have]].astype(np.float64), axis=1)
    line.update(sparse_with_a_dense_point=int(have.sum()), median_sparse_to_dense=None if not len(d) else round(float(np.median(d)), 5),
                median_sparse_depth=round(float(np.median(X[:, 2])), 4))
    ok = True
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import rectify_ref
        ref = rectify_ref.make_plan(camera, dist, sfm["R"], sfm["t"], (left.shape[1], left.shape[0]))
        r1, v1 = rectify_ref.rectify(left, camera, dist, ref, 1)
        r2, _ = rectify_ref.rectify(right, camera, dist, ref, 2)
        grey1 = r["rect1"] if left.ndim == 2 else None
        xyz, colors, pixel = rectify_ref.cloud(r["disp16"], r["valid"], r["rect1"], ref, -16, a.min_disp16)
        chk = {"plan": plan.record.tobytes() == ref.tobytes(), "rect1": grey1 is None or bool(np.array_equal(grey1, r1)),
               "rect2": left.ndim != 2 or bool(np.array_equal(r["rect2"], r2)), "valid": bool(np.array_equal(r["valid"], v1)),
               "cloud": r["points"].tobytes() == xyz.tobytes() and bool(np.array_equal(r["pixel"], pixel)) and bool(np.array_equal(r["colors"], colors))}
        if speckle:
            import speckle_ref
            plain = pkg.denseStereo(left, right, camera, dist, sfm["R"], sfm["t"], min_disp16=a.min_disp16, num_disparities=a.num_disparities)
            want, n_want = speckle_ref.components(plain["disp16"], -16, *speckle)
            chk["speckle"] = r["disp16"].tobytes() == want.tobytes() and int(r["removed"]) == n_want
            line["dense_points_unfiltered"] = int(plain["count"])
        line["check_vs_numpy"] = chk
        ok = all(chk.values())
    if a.ply:
        write_ply(a.ply, r["points"], r["colors"])
        line["ply"] = a.ply
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
