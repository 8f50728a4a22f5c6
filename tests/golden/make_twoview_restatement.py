"""Generator of tests/golden/twoview/restatement.npz: what the numpy restatement of the two-view stage (oracle/sfm_ref.py) returns on
the configurations of tests/twoview_scenes.py -- sfm_ref.find_essential_mat's (E, mask, iterations) for every RANSAC case, and
sfm_ref.five_point's models on the 300 minimal samples of each well-posed family. The restatement takes about a minute for all of
them; the GPU tests compare with this record, and tests/test_twoview_core.py runs the restatement afresh and holds the record to it
(decisions exact, matrices within 1e-12). It reads nothing but this repository.

usage: python tests/golden/make_twoview_restatement.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import twoview_scenes as scenes


def main():
    out = {}
    for name in scenes.RANSAC_CASES:
        E, mask, iters = scenes.restatement_ransac(name)
        out[f"ransac_E_{name}"] = np.zeros((3, 3)) if E is None else E
        out[f"ransac_mask_{name}"], out[f"ransac_iters_{name}"] = mask, np.int32(iters)
    for fam in scenes.GENERIC_FAMILIES:
        models = scenes.restatement_models(fam)
        out[f"models_count_{fam}"] = np.array([len(m) for m in models], dtype=np.int32)
        out[f"models_{fam}"] = np.array([m for ms in models for m in ms]).reshape(-1, 9)
    os.makedirs(os.path.dirname(scenes.GOLDEN), exist_ok=True)
    np.savez_compressed(scenes.GOLDEN, **out)
    print(f"{scenes.GOLDEN}: {len(out)} arrays, {os.path.getsize(scenes.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
