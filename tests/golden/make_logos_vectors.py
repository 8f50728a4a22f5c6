"""Generator of tests/golden/refdll_logos.npz: cv::xfeatures2d::matchLOGOS run WHOLE out of the reference DLL.

logos_runner.c maps SfM-GMS/bin/opencv_xfeatures2d452.dll and calls its matchLOGOS (export RVA 0x7fbc0) on each case
below. Only inputs and the DLL's (queryIdx, trainIdx) are stored; every DMatch it returned carried imgIdx -1 and distance
0, which the generator checks.

Substitutions (see logos_runner.c): the allocator and memmove / memset are this process's; logf and acosf, which the DLL
takes from the Windows CRT, are this process's libm. That last one is the residue of the fixture: a libm result may
differ in the last bit from the CRT's, and a decision sitting on that bit could flip.

Known behaviour of the DLL that the fixture does NOT cover:
  - frames of 1..5 keypoints: the DLL's nearest-neighbour pass copies NUM = 5 entries out of a list of n - 1, reading
    past its end, so its result there is undefined; the cases keep n >= 6 or n == 0;

The tie rule of the neighbour selection is the order the DLL's std::sort (MSVC introsort, not stable) leaves equal squared
distances in. tests/logos_ref.py and logos_core.h restate that sort; `sort_*` entries pin it directly: records of
(distance, index) with many equal distances, and the order the DLL's own sort function (logos_runner.c "sort") leaves them
in. Cases whose neighbour sets tie across the fifth place are named in `tie_cases`.

usage (wherever the reference DLL is present): python tests/golden/make_logos_vectors.py <path/to/opencv_xfeatures2d452.dll>
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
               ("class_id", "<i4")])


def _records(kp4):
    k = np.zeros(len(kp4), KP)
    k["x"], k["y"], k["size"], k["angle"] = kp4[:, 0], kp4[:, 1], kp4[:, 2], kp4[:, 3]
    k["class_id"] = -1
    return k


def _random_kp(rng, n, w=640, h=480):
    return np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(2, 30, n), rng.uniform(0, 360, n)],
                    1).astype(np.float32)


def _moved(kp, theta, scale, t):
    """The same points rotated by theta about the origin, scaled and shifted; keypoint angles turned the LOGOS way."""
    c, s = np.cos(theta), np.sin(theta)
    x, y = kp[:, 0].astype(np.float64), kp[:, 1].astype(np.float64)
    out = kp.copy()
    out[:, 0] = scale * (c * x - s * y) + t[0]
    out[:, 1] = scale * (s * x + c * y) + t[1]
    out[:, 2] = kp[:, 2] * scale
    out[:, 3] = np.mod(kp[:, 3] - np.degrees(theta), 360.0)
    return out.astype(np.float32)


def cases():
    """name -> (kp1 (n1, 4) float32 [x, y, size, angle], kp2, nn1 int32, nn2 int32)."""
    rng = np.random.default_rng(20261015)
    out = {}
    for n, words in ((6, 2), (17, 3), (64, 8), (300, 20), (2000, 50), (10000, 50)):
        out[f"random_n{n}"] = (_random_kp(rng, n), _random_kp(rng, n), rng.integers(0, words, n), rng.integers(0, words, n))
    for name, n, theta, scale in (("rot30_s1.3", 300, 0.5, 1.3), ("rot_m115_s0.7", 2000, -2.0, 0.7),
                                  ("rot57_s1.0", 3000, 1.0, 1.0)):
        kp1 = _random_kp(rng, n)
        kp2 = _moved(kp1, theta, scale, (40.0, -25.0))
        l1 = rng.integers(0, 20, n)
        l2 = l1.copy()
        l2[: n // 3] = rng.integers(0, 20, n // 3)           # a third outliers
        out[name] = (kp1, kp2, l1, l2)
    kp1 = _random_kp(rng, 200)
    out["single_label_n200"] = (kp1, _moved(kp1, 0.2, 1.1, (5.0, 5.0)), np.zeros(200), np.zeros(200))
    kp1 = _random_kp(rng, 600)
    kp1[:, :2] = np.round(kp1[:, :2] / 20.0) * 20.0                  # integer grid: ties and duplicate points
    kp2 = kp1.copy()
    kp2[:, :2] += np.float32(3.0)
    l1 = rng.integers(0, 20, 600)
    out["grid_ties_n600"] = (kp1, kp2, l1, l1.copy())
    kp1 = _random_kp(rng, 300)
    kp1[150:] = kp1[:150]                                            # every point twice
    l1 = rng.integers(0, 10, 300)
    l1[150:] = l1[:150]
    out["duplicates_n300"] = (kp1, _moved(kp1, 0.3, 1.0, (7.0, 1.0)), l1, l1.copy())
    for name, n, theta, scale in (("int_rot0.3_n800", 800, 0.3, 1.0), ("int_rot90_n600", 600, np.pi / 2, 1.0),
                                  ("int_rot_m0.2_s1.2_n500", 500, -0.2, 1.2)):
        kp1 = _random_kp(rng, n)
        kp1[:, :2] = np.round(kp1[:, :2])                            # integer coordinates: distance ties, not symmetric
        kp2 = _moved(kp1, theta, scale, (3.0, 4.0))
        kp2[:, :2] = np.round(kp2[:, :2])
        l1 = rng.integers(0, 20, n)
        l2 = l1.copy()
        l2[: n // 4] = rng.integers(0, 20, n // 4)
        out[name] = (kp1, kp2, l1, l2)
    for name, theta in (("rot_near_pi_n1000", np.pi - 0.005), ("rot_near_mpi_n1000", -np.pi + 0.01)):
        kp1 = _random_kp(rng, 1000)                                   # histogram peak at the first / last bins
        out[name] = (kp1, _moved(kp1, theta, 1.0, (700.0, 500.0)), rng.integers(0, 20, 1000), None)
    kp_a = _random_kp(rng, 200, 300, 300)                             # two identical groups far apart, turned by 0.5 and by
    kp_b = kp_a.copy()                                                # -1.0: their smoothed bins tie, the first one wins
    kp_b[:, 0] += 5000.0
    l_a = rng.integers(0, 10, 200)
    kp2_a = _moved(kp_a, 0.5, 1.0, (0.0, 0.0))
    kp2_b = _moved(kp_a, -1.0, 1.0, (0.0, 0.0))
    kp2_b[:, 0] += 5000.0
    out["tied_peak_n400"] = (np.concatenate([kp_a, kp_b]), np.concatenate([kp2_a, kp2_b]), np.concatenate([l_a, l_a + 10]),
                             np.concatenate([l_a, l_a + 10]))
    out.update(detector_case())
    out["empty_first"] = (np.zeros((0, 4), np.float32), _random_kp(rng, 50), np.zeros(0), rng.integers(0, 5, 50))
    out["empty_both"] = (np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), np.zeros(0), np.zeros(0))
    return {k: (a, b, np.asarray(c, np.int32), np.asarray(c if d is None else d, np.int32)) for k, (a, b, c, d) in out.items()}


def detector_case():
    """Keypoints of the committed 1080p pair (image_main_scenario_1080p.npz) by oracle/detect_ref.c (threshold 20, at most 10000),
    labelled by the nearest of 50 of frame 1's descriptors (every len / 50-th) under Hamming distance, first minimum on ties."""
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import gms_oracle
    img = np.load(os.path.join(HERE, "image_main_scenario_1080p.npz"))
    kp1, rows1 = gms_oracle.detect(img["left"], 20, 10000)
    kp2, rows2 = gms_oracle.detect(img["right"], 20, 10000)
    words = rows1[np.arange(50) * (len(rows1) // 50)]

    def label(rows):
        x = np.unpackbits(rows[:, None, :] ^ words[None, :, :], axis=2).sum(2)
        return np.argmin(x, axis=1)

    def as4(kp):
        return np.stack([kp["x"], kp["y"], kp["size"], kp["angle"]], 1).astype(np.float32)

    return {"detector_1080p": (as4(kp1), as4(kp2), label(rows1), label(rows2))}


def has_tie(kp):
    """True when some point's fifth and sixth nearest other points are at the same float32 squared distance."""
    sys.path.insert(0, os.path.dirname(HERE))
    x, y = kp[:, 0], kp[:, 1]
    n = len(x)
    if n < 7:
        return False
    for s in range(0, n, 1024):
        e = min(n, s + 1024)
        dx = x[s:e, None] - x[None, :]
        dy = y[s:e, None] - y[None, :]
        d = dx * dx + dy * dy
        d[np.arange(e - s), np.arange(s, e)] = np.inf
        d.sort(axis=1)
        if np.any(d[:, 4] == d[:, 5]):
            return True
    return False


def main(dll):
    data = open(dll, "rb").read()
    out = {"dll_sha256": np.array(hashlib.sha256(data).hexdigest())}
    ties = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "logos_runner")
        subprocess.check_call(["gcc", "-O1", "-o", exe, os.path.join(HERE, "logos_runner.c"), "-lm"])
        for name, (kp1, kp2, nn1, nn2) in cases().items():
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([len(kp1), len(kp2)], np.int32).tobytes())
                f.write(_records(kp1).tobytes() + _records(kp2).tobytes() + nn1.tobytes() + nn2.tobytes())
            subprocess.check_call([exe, dll, fin, fout])
            raw = open(fout, "rb").read()
            m = int(np.frombuffer(raw[:8], np.int64)[0])
            dm = np.frombuffer(raw[8:], np.int32).reshape(m, 4)
            assert np.all(dm[:, 2] == -1) and np.all(dm[:, 3] == 0)
            out[f"{name}_kp1"], out[f"{name}_kp2"] = kp1, kp2
            out[f"{name}_nn1"], out[f"{name}_nn2"] = nn1, nn2
            out[f"{name}_matches"] = dm[:, :2].copy()
            if has_tie(kp1) or has_tie(kp2):
                ties.append(name)
            print(f"{name}: {len(kp1)} x {len(kp2)} -> {m} matches")
        rng = np.random.default_rng(52)
        for t, (n, levels) in enumerate(((20, 3), (33, 4), (41, 5), (100, 6), (1000, 10), (5000, 40), (20000, 200))):
            rec = np.zeros(n, [("d", "<f4"), ("i", "<i4")])
            rec["d"] = rng.integers(0, levels, n).astype(np.float32)
            rec["i"] = np.arange(n)
            fin, fout = os.path.join(tmp, "sin.bin"), os.path.join(tmp, "sout.bin")
            with open(fin, "wb") as f:
                f.write(np.int32(n).tobytes() + rec.tobytes())
            subprocess.check_call([exe, dll, fin, fout, "sort"])
            res = np.fromfile(fout, rec.dtype)
            out[f"sort_{t}_d"] = rec["d"].copy()
            out[f"sort_{t}_order"] = res["i"].copy()
    out["tie_cases"] = np.array(sorted(ties))
    np.savez_compressed(os.path.join(HERE, "refdll_logos.npz"), **out)
    print("tie cases:", ties)


if __name__ == "__main__":
    main(sys.argv[1])
