"""The CPU statements of what pipeline.run_images / structureFromMotion do between pixels and a pose, each made of
statements the suite already has:

    grey(bgr)                 (299 R + 587 G + 114 B + 500) // 1000 on [.., 3] B, G, R bytes (gms_bgr_to_gray_device)
    pack(kp_blocks, rows_blocks, counts, max_keypoints)
                              the detector's [n, max_keypoints] blocks -> frames back to back with their offsets (gms_detect_pack_device)
    chain(oracle, left, right, camera, ...)
                              grad_desc_ref.detect on both images -> oracle.bf_match (NORM_L2, nearest neighbour) -> oracle.match =
                              matchGMS(true, true, 6.0) -> oracle.gather -> sfm_ref.two_view(prob 0.7, threshold 1.0): the reference's
                              structureFromMotion with algo 2 (SfMUtil.cpp:4-83 through FeatureMatchUtil.cpp:52-84)
    pose_checks(...)          what a right pose on real photographs has to satisfy, for the CPU's and the GPU's result alike
"""
import numpy as np

import grad_desc_ref
import sfm_ref


def grey(bgr):
    v = np.asarray(bgr).astype(np.int64)
    return ((299 * v[..., 2] + 587 * v[..., 1] + 114 * v[..., 0] + 500) // 1000).astype(np.uint8)


def pack(kp_blocks, rows_blocks, counts, max_keypoints):
    """kp_blocks [n, max_keypoints] records, rows_blocks [n, max_keypoints, width] -> (records, rows, frame_off int64 [n + 1]):
    frame_off[i + 1] = frame_off[i] + min(counts[i], max_keypoints), record and row j of image i at frame_off[i] + j."""
    take = np.minimum(np.maximum(np.asarray(counts, dtype=np.int64), 0), max_keypoints)
    frame_off = np.concatenate([[0], np.cumsum(take)]).astype(np.int64)
    kp = np.zeros(frame_off[-1], dtype=kp_blocks.dtype)
    rows = np.zeros((frame_off[-1],) + rows_blocks.shape[2:], dtype=rows_blocks.dtype)
    for i, c in enumerate(take):
        kp[frame_off[i]:frame_off[i] + c] = kp_blocks[i, :c]
        rows[frame_off[i]:frame_off[i] + c] = rows_blocks[i, :c]
    return kp, rows, frame_off


def chain(oracle, left, right, camera, max_keypoints=4000, threshold=20, n_levels=8, factor=6.0, prob=0.7, ransac_threshold=1.0):
    size = (left.shape[1], left.shape[0])
    (kp1, r32_1, _, rows1), (kp2, r32_2, _, rows2) = (grad_desc_ref.detect(oracle, img, threshold, max_keypoints, n_levels) for img in (left, right))
    matches = oracle.bf_match(rows1, rows2, False)
    rc, out, _, res = oracle.match(size, size, kp1, kp2, matches, True, True, factor)
    assert rc == 0
    _, w1, w2 = oracle.gather(kp1, kp2, out)
    tv = sfm_ref.two_view(w1, w2, camera, None, prob, ransac_threshold)
    return dict(keypoints=(kp1, kp2), rows32=(r32_1, r32_2), rows128=(rows1, rows2), matches=matches, survivors=out, result=res, two_view=tv)


def pose_checks(n_kp1, n_kp2, n_survivors, n_pose, n_behind, sum_sq_err1, sum_sq_err2, camera, ransac_threshold=1.0):
    """-> the reprojection RMS in pixels, after asserting: keypoints on both images; at least 1000 GMS survivors (2659 on the committed
    pair at 4000 keypoints); recoverPose keeps at least half of them; no triangulated point behind a camera; RMS below
    ransac_threshold pixels -- findEssentialMat's inliers lie within that distance of their epipolar lines, so an RMS at or above it
    means a wrong pose."""
    assert n_kp1 > 0 and n_kp2 > 0
    assert n_survivors >= 1000
    assert 2 * n_pose >= n_survivors
    assert n_behind == 0
    rms = float(np.sqrt((sum_sq_err1 + sum_sq_err2) / (2 * n_pose)) * (camera[0] + camera[1]) / 2)
    assert rms < ransac_threshold
    return rms
