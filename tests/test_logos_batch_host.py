"""CPU: the host side of the batched LOGOS path -- the C ABI's argument checks and buffer sizes, and the Python layer's pair tables
and argument handling -- without a device."""
import importlib
import types

import numpy as np
import pytest

NULL = None


def test_entry_points_refuse_bad_arguments_before_any_device_work(pkg):
    lib = pkg.load_library()
    kp = np.zeros(4, pkg.KEYPOINT_DTYPE)
    off = np.array([0, 4], np.int64)
    w = np.zeros(4, np.int32)
    pairs = np.zeros(1, pkg.PAIR_DTYPE)
    res = np.zeros(1, pkg.LOGOS_RESULT_DTYPE)
    # no context
    assert lib.gms_logos_prepare_device(NULL, NULL, off.ctypes.data, 1, 4, NULL, 50, NULL, 0, NULL) == -1
    assert lib.gms_logos_host_batch(NULL, kp.ctypes.data, off.ctypes.data, 1, w.ctypes.data, 50, pairs.ctypes.data, 1, NULL,
                                    res.ctypes.data) == -1
    assert lib.gms_logos_words_device(NULL, 1, NULL, 10, NULL, 50, NULL) == -1
    assert lib.gms_logos_filter_device(NULL, NULL, NULL, 1, NULL, 0, NULL, NULL, NULL) == -1
    # sizes refuse what the entry points refuse: no words, too many words, negative sizes
    for n_words in (0, 65536, -3):
        assert lib.gms_logos_table_bytes(100, 2, n_words) == 0
    assert lib.gms_logos_table_bytes(100, -1, 50) == 0
    assert lib.gms_logos_workspace_bytes(0, -1, 0) == 0 and lib.gms_logos_workspace_bytes(0, 1, -1) == 0


def test_table_and_workspace_sizes_grow_with_their_arguments(pkg):
    lib = pkg.load_library()
    t = [lib.gms_logos_table_bytes(n, 3, 50) for n in (0, 1, 1000, 10000)]
    assert t == sorted(t) and t[0] > 0 and all(x % 16 == 0 for x in t)
    # 16 (point) + 4 (word) + 20 (neighbours) + 4 (sorted) + 4 (tie list) bytes per keypoint, at least
    assert t[3] - t[2] >= 9000 * 48
    assert lib.gms_logos_table_bytes(1000, 3, 100) - lib.gms_logos_table_bytes(1000, 3, 50) >= 3 * 50 * 4 - 16  # (16-byte sections)
    # the filter needs one int64 per query keypoint of the batch; the tie pass a slice of two words per other point per lane
    assert lib.gms_logos_workspace_bytes(0, 1100, 90) >= 1100 * 90 * 8
    assert lib.gms_logos_workspace_bytes(10000, 0, 0) >= 512 * 8 * 9999


def test_logos_pair_table_defaults_and_bad_indices():
    batch = importlib.import_module("sfm-gms_amd.batch")
    table = types.SimpleNamespace(n_frames=3, counts=np.array([10, 40, 25], np.int64))
    p = batch.logos_pair_table(table, [(0, 1), (2, 0), (1, 1), (0, 7), (-1, 2)])
    assert p["m"].tolist() == [40, 25, 40, 10, 25]            # the larger frame; an index out of range counts as empty
    assert p["match_off"].tolist() == [0, 40, 65, 105, 115]
    q = batch.logos_pair_table(table, [(0, 1), (2, 0)], capacity=[5, 9])
    assert q["m"].tolist() == [5, 9] and q["match_off"].tolist() == [0, 5]


def test_run_dataset_checks_its_method_and_inputs_first(pkg):
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    io = importlib.import_module("sfm-gms_amd.io")
    ds = io.Dataset([np.zeros(3, pkg.KEYPOINT_DTYPE)], [(64, 64)], None, -1, pairs=np.zeros(0, pkg.PAIR_DTYPE),
                    matches=np.zeros(0, pkg.DMATCH_DTYPE))
    with pytest.raises(ValueError, match="unknown method"):
        pipeline.run_dataset(None, ds, method="orb")
    with pytest.raises(ValueError, match="descriptors and a dictionary"):
        pipeline.run_dataset(None, ds, method="logos", dictionary=np.zeros((5, 128), np.float32))
