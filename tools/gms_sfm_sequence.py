#!/usr/bin/env python3
"""A sequence of photographs to poses, tracks and one cloud, every stage on the GPU (structureFromMotionMulti in sfm-gms_amd/api.py ->
pipeline.run_images(register=True): per pair the two-view stage, then gms_sfm_register_device joins the pairs).
Prints one JSON line: per pair n_links, r, S and status; per view the camera centre; tracks by length; the median spread.

    python tools/gms_sfm_sequence.py [images.npz] [--method gms|bf|logos] [--pairs chain|star|all] [--root 0] [--min-links 8] [--max-keypoints 2000] [--ply out.ply] [--unique] [--bundle] [--dense [--speckle SIZE,DIFF16] [--dense-poses pair|registration|bundle] [--dense-pairs a-b,c-d] [--fuse [--fuse-tol16 16] [--fuse-min-support 1]]] [--check]

images.npz: arrays images ([n, H, W] grey or [n, H, W, 3] BGR, uint8) and camera = (fx, fy, cx, cy), optionally dist. Default: views
1, 2, 3, 4 of the reference's SourceImages scene from the two committed fixtures (tests/golden/image_sfm_pair_1008x756.npz holds views 1
and 4, image_sfm_more_1008x756.npz views 2 and 3), with the pair's stated camera. --pairs: chain (i, i + 1); star (root, i); all:
every a < b in order (the pairs that close a loop are skipped by the plan). --ply: the cloud as an ASCII PLY file (x, y, z, and the
track's keypoint count as `obs`). --check: feeds the GPU's own two-view records to the numpy statement (tests/sfm_register_ref.py)
and compares: integers exactly, doubles to 1e-9; test infrastructure. --bundle: bundle adjustment behind the registration
(gms_sfm_ba_device): reprojection RMS before and after, accepted iterations, tracks used and excluded, the camera
centres after; with --check also against tests/sfm_ba_ref.py under the tolerance measured on these records. --dense: the dense
cloud of every pair; --fuse: the clouds fused into one by depth consistency (gms_dense_fuse_device):
the points per pair, the fused total and a histogram of `support`; --ply then writes the fused cloud (x, y, z, the colour, support);
with --check the dense stage is run once more to read its maps back, the numpy statement (tests/dense_fuse_ref.py) fuses them, and
every output byte is compared. --speckle SIZE,DIFF16 (with --dense): the speckle filter on every pair's map before the reprojection
(DIFF16 in sixteenths of a pixel): the pixels removed per pair; with --check the stage is run with and without the
filter, and the filtered maps and clouds must equal the numpy statements (tests/speckle_ref.py, tests/rectify_ref.py).
--dense-poses registration | bundle (the latter with --bundle): the dense stage and the fusion on pair records derived from the
registration's / the bundle-adjusted views (gms_sfm_pair_poses_device) instead of each pair's own two-view pose;
--dense-pairs a-b,c-d: those frame pairs are matched densely in place of the sparse pair list (the per-pair figures of the dense
stage and the fusion then follow that list). With --check the records must equal the numpy statement (tests/sfm_pair_pose_ref.py)
on the GPU's own views and every plan tests/rectify_ref.py's on its record, byte for byte; the other checks run on those records.
--unique: one-to-one matches per pair in front of the registration (gms_match_unique_device): per pair the live and
the kept matches; the tracks, and with --bundle the observations, are then built from the kept matches only. With --check the keep
plane and the counts must equal the numpy statement (tests/match_unique_ref.py) on the GPU's own records byte for byte, and the
registration is compared with that statement's register_keep."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def default_images():
    a, b = np.load(os.path.join(GOLDEN, "image_sfm_pair_1008x756.npz")), np.load(os.path.join(GOLDEN, "image_sfm_more_1008x756.npz"))
    return np.stack([a["left"], b["second"], b["third"], a["right"]]), tuple(float(v) for v in a["camera"]), None


def pair_list(kind, n, root):
    if kind == "chain":
        return [(i, i + 1) for i in range(n - 1)]
    if kind == "star":
        return [(root, i) for i in range(n) if i != root]
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def write_ply(path, cloud, obs):
    keep = np.isfinite(cloud).all(1)
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {int(keep.sum())}\nproperty double x\nproperty double y\nproperty double z\nproperty int obs\nend_header\n")
        for p, o in zip(cloud[keep], obs[keep]):
            f.write(f"{p[0]:.9g} {p[1]:.9g} {p[2]:.9g} {int(o)}\n")


def write_fused_ply(path, f):
    col = f["colors"] if f["colors"].ndim == 2 else np.stack([f["colors"]] * 3, axis=1)   # BGR, or grey three times
    with open(path, "w") as out:
        out.write(f"ply\nformat ascii 1.0\nelement vertex {len(f['points'])}\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar support\nend_header\n")
        for p, c, s in zip(f["points"], col, f["support"]):
            out.write(f"{p[0]:.9g} {p[1]:.9g} {p[2]:.9g} {int(c[2])} {int(c[1])} {int(c[0])} {int(s)}\n")


def dense_inputs(pkg, r, a):
    """What the dense stage and the fusion read of the run: `r` itself, or with --dense-poses the records derived from the views."""
    if a.dense_poses == "pair":
        return r
    tv, reg = r["dense_pose_records"]
    fp = np.array(a.dense_pairs, np.int64).reshape(-1, 2) if a.dense_pairs else np.stack([r["pairs"]["frame_a"], r["pairs"]["frame_b"]], 1)
    pairs = np.zeros(len(fp), pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = fp[:, 0], fp[:, 1]
    return dict(r, pairs=pairs, two_view=tv, registration=reg, views=r["views_ba" if a.dense_poses == "bundle" else "views"])


def check_pose_records(rd, images, camera, dist):
    """--dense-poses --check: the records against tests/sfm_pair_pose_ref.py on the GPU's own views, and every returned plan against
    tests/rectify_ref.py on its record, byte for byte. Test infrastructure."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rectify_ref
    import sfm_pair_pose_ref as pp
    views = np.zeros(len(rd["views"]), pp.VIEW_DTYPE)
    for k in views.dtype.names:
        views[k] = np.asarray(rd["views"][k]).reshape(views[k].shape)
    fp = np.stack([rd["pairs"]["frame_a"], rd["pairs"]["frame_b"]], 1)
    tv, reg = pp.pair_poses(views, fp)
    plans = True
    for i, d in enumerate(rd["dense"]):
        if d is not None:
            p = d["plan"][0]
            want = rectify_ref.make_plan(camera, dist, tv["R"][i], tv["t"][i], (images.shape[2], images.shape[1]), (int(p["out_w"]), int(p["out_h"])))
            plans &= np.asarray(want).tobytes() == d["plan"].tobytes()
    return {"two_view": rd["two_view"].tobytes() == tv.tobytes(), "registration": rd["registration"].tobytes() == reg.tobytes(), "plans": bool(plans)}


def check_speckle(r, images, camera, dist, a):
    """--dense --speckle --check: the dense stage once more with and without the filter, the maps read back: every filtered map must
    equal the numpy statement (tests/speckle_ref.py) of the unfiltered one, and the cloud the numpy chain (tests/rectify_ref.py) on
    the filtered map. Test infrastructure."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rectify_ref
    import speckle_ref
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    ctx = importlib.import_module("sfm-gms_amd.api").default_context()
    d_photos = torch.from_numpy(np.ascontiguousarray(images)).to(f"cuda:{ctx.device}")
    plain, filt = [], []
    pipeline._dense_pairs(ctx, d_photos, r, camera, dist, 16, a.dense_cap, None, False, plain)
    pipeline._dense_pairs(ctx, d_photos, r, camera, dist, 16, a.dense_cap, None, False, filt, a.speckle)
    maps = removed = clouds = True
    for (p, idx), (f, _) in zip(plain, filt):
        plans = f.plans()
        for j in range(len(idx)):
            want, n_want = speckle_ref.components(p.d_disp16[j].cpu().numpy(), -16, *a.speckle)
            got = f.d_disp16[j].cpu().numpy()
            maps &= got.tobytes() == want.tobytes()
            removed &= int(f.d_removed[j]) == n_want
            image = (f.d_color if f.d_color is not None else f.d_rect1)[j].cpu().numpy()
            xyz = rectify_ref.cloud(got, f.d_valid[j].cpu().numpy(), image, plans[j:j + 1], -16, 16)[0]
            k = min(int(f.d_count[j]), f.cap)
            clouds &= int(f.d_count[j]) == len(xyz) and f.d_xyz[j, :k].cpu().numpy().tobytes() == xyz[:k].tobytes()
    return {"maps": bool(maps), "removed": bool(removed), "clouds": bool(clouds)}


def check_fusion(pkg, r, images, camera, dist, a):
    """The dense stage once more on the same records (it is deterministic), its maps read back, tests/dense_fuse_ref.py on them, and
    the fused cloud the run returned compared byte for byte. Test infrastructure."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dense_fuse_ref as fr
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    api = importlib.import_module("sfm-gms_amd.api")
    ctx = api.default_context()
    d_photos = torch.from_numpy(np.ascontiguousarray(images)).to(f"cuda:{ctx.device}")
    runs = []
    dense = pipeline._dense_pairs(ctx, d_photos, r, camera, dist, 16, a.dense_cap, None, True, runs, a.speckle)
    same_dense = all((x is None) == (y is None) and (x is None or x["points"].tobytes() == y["points"].tobytes()) for x, y in zip(dense, r["dense"]))
    channels = 3 if images.ndim == 4 else 1
    srcs, pair_of = {}, []
    for run, idx in runs:
        plans, counts = run.plans(), run.d_count.cpu().numpy()
        for j, i in enumerate(idx):
            v = r["views"][int(r["pairs"]["frame_a"][i])]
            g = r["registration"][i]
            srcs[i] = fr.source(run.d_disp16[j].cpu().numpy(), run.d_valid[j].cpu().numpy(), plans[j:j + 1], run.d_xyz[j].cpu().numpy()[:run.cap],
                                count=int(counts[j]), color=run.d_cloud_color[j].cpu().numpy()[:run.cap], filtered16=-16, min_disp16=16,
                                view=(v["R"], v["t"], int(v["registered"])), reg=(float(g["S"]), int(g["status"])))
    pair_of = np.array(sorted(srcs), np.int32)
    want = fr.fuse([srcs[i] for i in pair_of], None, channels, a.fuse_tol16, a.fuse_min_support) if len(pair_of) else None
    f = r["dense_fused"]
    if want is None:
        return {"dense_repeats": bool(same_dense), "empty": len(f["points"]) == 0}
    counts = np.zeros(len(r["pairs"]) + 1, np.int32)
    counts[pair_of], counts[-1] = want["counts"][:-1], want["counts"][-1]
    colors = want["colors"] if channels == 3 else want["colors"][:, 0]
    return {"dense_repeats": bool(same_dense), "counts": bool(np.array_equal(f["counts"], counts)),
            "points": f["points"].tobytes() == want["points"].tobytes(), "colors": f["colors"].tobytes() == np.ascontiguousarray(colors).tobytes(),
            "source": bool(np.array_equal(f["source"], pair_of[want["source"]])), "index": bool(np.array_equal(f["index"], want["index"])),
            "support": bool(np.array_equal(f["support"], want["support"])), "conflict": bool(np.array_equal(f["conflict"], want["conflict"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("images", nargs="?")
    ap.add_argument("--method", choices=("gms", "bf", "logos"), default="gms")
    ap.add_argument("--pairs", choices=("chain", "star", "all"), default="chain")
    ap.add_argument("--root", type=int, default=0)
    ap.add_argument("--min-links", type=int, default=8)
    ap.add_argument("--max-keypoints", type=int, default=2000)
    ap.add_argument("--ply")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--bundle", action="store_true")
    ap.add_argument("--unique", action="store_true", help="one-to-one matches per pair in front of the registration (DESIGN.md 4.10e)")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--fuse", action="store_true")
    ap.add_argument("--fuse-tol16", type=int, default=16)
    ap.add_argument("--fuse-min-support", type=int, default=1)
    ap.add_argument("--dense-cap", type=int, default=None)
    ap.add_argument("--speckle", help="SIZE,DIFF16: the speckle filter on every pair's map (DESIGN.md 4.13c)")
    ap.add_argument("--dense-poses", choices=("pair", "registration", "bundle"), default="pair")
    ap.add_argument("--dense-pairs", help="a-b,c-d: the frame pairs to match densely (needs --dense-poses registration or bundle)")
    a = ap.parse_args()
    if a.fuse and not a.dense:
        ap.error("--fuse needs --dense")
    if a.speckle and not a.dense:
        ap.error("--speckle needs --dense")
    a.speckle = tuple(int(v) for v in a.speckle.split(",")) if a.speckle else None
    if a.dense_poses != "pair" and not a.dense:
        ap.error("--dense-poses needs --dense")
    if a.dense_poses == "bundle" and not a.bundle:
        ap.error("--dense-poses bundle needs --bundle")
    if a.dense_pairs and a.dense_poses == "pair":
        ap.error("--dense-pairs needs --dense-poses registration or bundle")
    a.dense_pairs = [tuple(int(v) for v in p.split("-")) for p in a.dense_pairs.split(",")] if a.dense_pairs else None
    if a.images:
        z = np.load(a.images)
        images, camera = np.ascontiguousarray(z["images"], dtype=np.uint8), tuple(float(v) for v in z["camera"])
        dist = tuple(float(v) for v in z["dist"]) if "dist" in z.files else None
    else:
        images, camera, dist = default_images()
    n = len(images)
    if not 0 <= a.root < n:
        ap.error("--root: a frame index")
    pairs = pair_list(a.pairs, n, a.root)
    pkg = importlib.import_module("sfm-gms_amd")
    r = pkg.structureFromMotionMulti(images, camera, dist, method=a.method, pairs=pairs, root=a.root, min_links=a.min_links,
                                     max_keypoints=a.max_keypoints, keep_tables=True, bundle=a.bundle, unique=a.unique,
                                     **(dict(dense=True, dense_cap=a.dense_cap, dense_speckle=a.speckle) if a.dense else {}),
                                     **(dict(dense_poses=a.dense_poses, dense_pairs=a.dense_pairs) if a.dense_poses != "pair" else {}),
                                     **(dict(fuse=True, fuse_tol16=a.fuse_tol16, fuse_min_support=a.fuse_min_support) if a.fuse else {}))
    reg, views, tv = r["registration"], r["views"], r["two_view"]
    centres = [None if not v["registered"] else [round(float(x), 5) for x in -v["R"].T @ v["t"]] for v in views]
    obs, spread, cloud = r["cloud_obs"], r["cloud_spread"], r["cloud"]
    depth = cloud[:, 2][np.isfinite(cloud[:, 2])]
    many = spread[r["cloud_est"] > 1]
    line = {"images": [int(n), int(images.shape[2]), int(images.shape[1])], "method": a.method, "pairs": a.pairs, "root": a.root,
            "min_links": a.min_links, "max_keypoints": a.max_keypoints, "keypoints": np.diff(r["tables"][0].frame_off_host).tolist(),
            "per_pair": [{"pair": [int(p["frame_a"]), int(p["frame_b"])], "survivors": int(t["n_points"]), "points": int(t["n_triangulated"]),
                          "two_view_status": int(t["status"]), "status": int(g["status"]), "n_links": int(g["n_links"]),
                          "r": round(float(g["r"]), 6), "S": round(float(g["S"]), 6)} for p, t, g in zip(r["pairs"], tv, reg)],
            "camera_centres": centres, "registered": int(r["summary"]["n_registered"][0]), "ok_pairs": int(r["summary"]["n_ok_pairs"][0]),
            "tracks": int(r["summary"]["n_tracks"][0]), "estimates": int(r["summary"]["n_points"][0]),
            "tracks_with_two_keypoints_of_a_frame": int(r["summary"]["n_multi"][0]),
            "tracks_by_keypoints": {str(k): int(c) for k, c in enumerate(np.bincount(obs, minlength=3)) if k >= 2 and c},
            "median_depth": None if not len(depth) else round(float(np.median(depth)), 5),
            "median_spread": None if not len(many) else round(float(np.median(many)), 6),
            "median_spread_over_median_depth": None if not len(many) or not len(depth) else round(float(np.median(many) / np.median(depth)), 6)}
    if a.unique:
        line["unique"] = {"live_per_pair": r["unique_counts"][:, 0].tolist(), "kept_per_pair": r["unique_counts"][:, 1].tolist()}
    if a.bundle:
        s, st = r["ba_summary"][0], np.bincount(r["track_status"], minlength=4)
        line["bundle"] = {"rms_px_before": round(float(s["rms0_px"]), 4), "rms_px_after": round(float(s["rms_px"]), 4),
                          "cost_before": round(float(s["cost0"]), 3), "cost_after": round(float(s["cost"]), 3),
                          "iterations_run": int(s["iters_run"]), "iterations_accepted": int(s["iters_accepted"]), "cg_iterations": int(s["cg_iters"]),
                          "observations": int(s["n_obs"]), "active": int(s["n_active"]), "free_frames": int(s["n_frames_free"]),
                          "tracks_used": int(s["n_tracks_used"]), "tracks_excluded_two_keypoints_of_a_frame": int(st[1]),
                          "tracks_excluded_fewer_than_two": int(st[2]), "tracks_kept_cloud_point_at_retriangulation": int(st[3]),
                          "camera_centres": [None if not v["registered"] else [round(float(x), 5) for x in -v["R"].T @ v["t"]] for v in r["views_ba"]]}
    ok = True
    rd = dense_inputs(pkg, r, a) if a.dense else r
    if a.dense:
        line["dense_points_per_pair"] = [0 if d is None else int(d["count"]) for d in r["dense"]]
        if a.dense_poses != "pair":
            line["dense_poses"] = {"from": a.dense_poses, "pairs": [[int(p["frame_a"]), int(p["frame_b"])] for p in rd["pairs"]],
                                   "status": rd["two_view"]["status"].tolist(), "S": [round(float(v), 6) for v in rd["registration"]["S"]]}
            if a.check:
                line["dense_poses"]["check_vs_statement"] = check_pose_records(rd, images, camera, dist)
                ok = ok and all(line["dense_poses"]["check_vs_statement"].values())
        if a.speckle:
            line["speckle"] = {"size": a.speckle[0], "diff16": a.speckle[1], "removed_per_pair": [0 if d is None else int(d["removed"]) for d in r["dense"]]}
            if a.check:
                line["speckle"]["check_vs_statement"] = check_speckle(rd, images, camera, dist, a)
                ok = ok and all(line["speckle"]["check_vs_statement"].values())
    if a.fuse:
        f = r["dense_fused"]
        line["fused"] = {"tol16": a.fuse_tol16, "min_support": a.fuse_min_support, "kept_per_pair": f["counts"][:-1].tolist(), "total": int(f["counts"][-1]),
                         "sum_of_parts": int(sum(line["dense_points_per_pair"])),
                         "support_histogram": {str(k): int(c) for k, c in enumerate(np.bincount(f["support"])) if c},
                         "conflict_histogram": {str(k): int(c) for k, c in enumerate(np.bincount(f["conflict"])) if c}}
        if a.check:
            chk = check_fusion(pkg, rd, images, camera, dist, a)
            line["fused"]["check_vs_statement"] = chk
            ok = ok and all(chk.values())
    if a.check and a.bundle:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import sfm_ba_ref as ba_ref
        frames = r["tables"][0]
        kp = frames.d_kp.cpu().numpy().view(pkg.KEYPOINT_DTYPE)[:int(frames.frame_off_host[-1])]
        cam9 = tuple(camera) + (tuple(dist) if dist is not None else (0.0,) * 5)
        args = (np.stack([kp["x"], kp["y"]], 1), frames.frame_off_host, r["pairs"], r["out"], r["mask"], views, reg, r["track"], r["cloud"],
                r["cloud_id"], cam9)
        fwd, rev = ba_ref.bundle_adjust(*args), ba_ref.bundle_adjust(*args, order=-1)

        def rel(x, y, floor):
            x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
            return float((np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), floor)).max()) if x.size else 0.0

        def apart(p, q):
            return max(rel(p["views_ba"]["R"], q["views_ba"]["R"], 1.0), rel(p["views_ba"]["t"], q["views_ba"]["t"], 1.0),
                       rel(p["cloud_ba"], q["cloud_ba"], 1.0), rel(p["ba_summary"]["cost"], q["ba_summary"]["cost"], 1e-300))
        tol = max(16.0 * apart(fwd, rev), 1e-12)   # 16 times what the order of the sums is worth, DESIGN.md 4.10c
        ints = ("n_obs", "n_active", "n_tracks_used", "n_tracks_multi", "n_frames_free", "iters_run", "iters_accepted", "status")
        chk = {"ba_integers": bool(np.array_equal(r["track_status"], fwd["track_status"]) and all(s[k] == fwd["ba_summary"][0][k] for k in ints)),
               "ba_doubles": apart(r, fwd) <= tol}
        line["bundle"]["check_vs_statement"] = dict(chk, tolerance=tol, apart=apart(r, fwd))
        ok = ok and all(chk.values())
    if a.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import sfm_register_ref as ref
        keep = None
        if a.unique:
            import match_unique_ref as unique_ref
            keep, counts = unique_ref.unique(r["tables"][0].frame_off_host, r["pairs"], r["out"], r["mask"], tv)
            line["unique"]["check_vs_statement"] = {"keep": r["keep"].tobytes() == keep.tobytes(), "counts": r["unique_counts"].tobytes() == counts.tobytes()}
            ok = ok and all(line["unique"]["check_vs_statement"].values())
            want = unique_ref.register_keep(r["tables"][0].frame_off_host, r["pairs"], r["out"], r["mask"], r["points3d"], tv, a.root, a.min_links,
                                            keep=keep)
        else:
            want = ref.register(r["tables"][0].frame_off_host, r["pairs"], r["out"], r["mask"], r["points3d"], tv, a.root, a.min_links)

        def near(x, y, size=0.0):
            x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
            fin = np.isfinite(x) & np.isfinite(y)
            same = (x[~fin] == y[~fin]) | (np.isnan(x[~fin]) & np.isnan(y[~fin]))
            return bool(x.shape == y.shape and same.all() and (np.abs(x[fin] - y[fin]) <= 1e-9 * np.maximum(np.maximum(np.abs(x[fin]), np.abs(y[fin])), size)).all())
        fin = want["cloud"][np.isfinite(want["cloud"])]
        chk = {"plan": r["register_plan"].tobytes() == want["plan"].tobytes(),
               "pair_integers": all(np.array_equal(reg[f], want["registration"][f]) for f in ("n_links", "depth", "link", "role", "status")),
               "scales_1e-9": near(reg["r"], want["registration"]["r"]) and near(reg["S"], want["registration"]["S"]),
               "views_1e-9": near(views["R"], want["views"]["R"], 1.0) and near(views["t"], want["views"]["t"], 1.0)
               and np.array_equal(views["registered"], want["views"]["registered"]),
               "points_1e-9": near(r["points_world"], want["points_world"][:len(r["points_world"])], 1.0),
               "tracks": bool(np.array_equal(r["track"], want["track"][:len(r["track"])])),
               "cloud": bool(np.array_equal(r["cloud_id"], want["cloud_id"]) and np.array_equal(obs, want["cloud_obs"])
                             and np.array_equal(r["cloud_est"], want["cloud_est"]) and near(cloud, want["cloud"], 1.0)
                             and near(spread, want["cloud_spread"], 1.0 + (np.abs(fin).max() if fin.size else 0.0))),
               "summary": r["summary"].tobytes() == want["summary"].tobytes()}
        line["check_vs_statement"] = {k: bool(v) for k, v in chk.items()}
        ok = ok and all(chk.values())
    if a.ply and a.fuse:
        write_fused_ply(a.ply, r["dense_fused"])
    elif a.ply:
        write_ply(a.ply, cloud, obs)
    print(json.dumps(line))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
