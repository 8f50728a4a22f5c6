"""A numpy statement of the pyramid keypoint source (gms_detect_pyramid_batch_device, include/gms.h): the level
sizes, the resize, the quotas and the mapping to level-0 coordinates, with the per-level detector taken from the existing CPU
statement (oracle.detect = oracle/detect_ref.c, unchanged). Everything is integer or single-rounded fp32, so the GPU is compared with
this byte for byte.

    level_sizes(w, h, n_levels)                 [(w_l, h_l)]: level 0 = the image, w_l = (5 w_{l-1} + 3) // 6, stop at n_levels or
                                                before the first level with width or height <= 32
    resize(img, w_dst, h_dst)                   bilinear, pixel centres aligned, 8-bit fixed-point weights, round to nearest, edges clamped
    quotas(sizes, max_keypoints)                q_l = max_keypoints * area_l // sum(areas), the remainder to level 0
    build(img, n_levels)                        the level images
    detect(oracle, img, threshold, max_keypoints, n_levels) -> (keypoints, rows, level_counts)
"""
import numpy as np

MAX_LEVELS = 16
BORDER = 16


def level_sizes(w, h, n_levels):
    if not 1 <= n_levels <= MAX_LEVELS:
        raise ValueError("n_levels outside [1, 16]")
    sizes = []
    while len(sizes) < n_levels and w > 2 * BORDER and h > 2 * BORDER:
        sizes.append((int(w), int(h)))
        w, h = (5 * w + 3) // 6, (5 * h + 3) // 6
    return sizes


def _axis(n_src, n_dst):
    """Fixed-point source coordinate of every output index: (first tap, second tap, weight of the second tap out of 256)."""
    if n_dst > n_src:
        raise ValueError("the pyramid only shrinks")
    i = np.arange(n_dst, dtype=np.int64)
    fixed = (2 * i + 1) * n_src * 128 // n_dst - 128          # = floor(256 * ((i + 0.5) * n_src / n_dst - 0.5)), >= 0
    i0 = fixed >> 8
    return i0, np.minimum(i0 + 1, n_src - 1), fixed & 255


def resize(img, w_dst, h_dst):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h_src, w_src = img.shape
    x0, x1, ax = _axis(w_src, w_dst)
    y0, y1, ay = _axis(h_src, h_dst)
    p = img.astype(np.int64)
    ax, ay = ax[None, :], ay[:, None]
    top = (256 - ax) * p[y0][:, x0] + ax * p[y0][:, x1]
    bot = (256 - ax) * p[y1][:, x0] + ax * p[y1][:, x1]
    return (((256 - ay) * top + ay * bot + 32768) >> 16).astype(np.uint8)


def quotas(sizes, max_keypoints):
    areas = [w * h for w, h in sizes]                          # Python integers: no overflow
    q = [int(max_keypoints) * a // sum(areas) for a in areas]
    q[0] = int(max_keypoints) - sum(q[1:])
    return q


def build(img, n_levels):
    h, w = img.shape
    levels = [np.ascontiguousarray(img, dtype=np.uint8)]
    for wl, hl in level_sizes(w, h, n_levels)[1:]:
        levels.append(resize(levels[-1], wl, hl))
    return levels


def detect(oracle, img, threshold=20, max_keypoints=10000, n_levels=8):
    """-> (keypoints in level-0 coordinates, level 0 first; [n, 32] rows; counts per level, length n_levels, 0 for unused levels)."""
    h, w = img.shape
    levels = build(img, n_levels)
    sizes = [(l.shape[1], l.shape[0]) for l in levels]
    kps, rows, counts = [], [], np.zeros(n_levels, dtype=np.int32)
    for l, (level, q) in enumerate(zip(levels, quotas(sizes, max_keypoints))):
        kp, r = oracle.detect(level, threshold, q)
        fx, fy = np.float32(w) / np.float32(sizes[l][0]), np.float32(h) / np.float32(sizes[l][1])
        half = np.float32(0.5)
        kp = kp.copy()
        kp["x"] = (kp["x"].astype(np.float32) + half) * fx - half      # each operation rounds once, in fp32
        kp["y"] = (kp["y"].astype(np.float32) + half) * fy - half
        kp["size"] = np.float32(31.0) * fx
        kp["octave"] = l
        kps.append(kp)
        rows.append(r)
        counts[l] = len(kp)
    return np.concatenate(kps), np.concatenate(rows).reshape(-1, 32), counts
