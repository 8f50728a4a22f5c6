"""CPU: the Python layer's shared plumbing -- per-frame counts, pair tables, the run-again-on-overflow merge and the descriptor
layout -- without a device. The expected tables are what bf_select_table / logos_pair_table returned before these helpers existed."""
import importlib
import types

import numpy as np
import pytest

FRAME_PAIRS = [(0, 1), (2, 0), (1, 1), (0, 7), (-1, 2)]   # (the last two: a frame index out of range on either side)
COUNTS = np.array([10, 40, 25], np.int64)


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def test_frame_counts_out_of_range_and_no_frames():
    batch = _batch()
    n = len(COUNTS)
    assert batch.frame_counts(COUNTS, [-1, 0, n - 1, n]).tolist() == [0, 10, 25, 0]
    assert batch.frame_counts(COUNTS, np.array([1, 1, 2], np.int32)).tolist() == [40, 40, 25]
    for none in (np.zeros(0, np.int64), []):
        assert batch.frame_counts(none, [-1, 0, 1, 5]).tolist() == [0, 0, 0, 0]
    assert batch.frame_counts(COUNTS, []).tolist() == []


def test_pair_table_capacities(pkg):
    batch = _batch()
    for cap, m, off in ((7, [7] * 5, [0, 7, 14, 21, 28]),                         # one room for all
                        ([5, 2, 9, 0, 4], [5, 2, 9, 0, 4], [0, 5, 7, 16, 16]),   # one per pair
                        ([5, -2, 9, 0, 4], [5, -2, 9, 0, 4], [0, 5, 5, 14, 14])):  # a negative room takes none (bf_select_table)
        t = batch.pair_table(FRAME_PAIRS, cap)
        assert t.dtype == pkg.PAIR_DTYPE
        assert t["frame_a"].tolist() == [a for a, _ in FRAME_PAIRS] and t["frame_b"].tolist() == [b for _, b in FRAME_PAIRS]
        assert t["m"].tolist() == m and t["match_off"].tolist() == off and (t["reserved"] == 0).all()
    for empty in ([], np.zeros((0, 2), np.int64)):
        for cap in (3, [], np.zeros(0, np.int64)):
            t = batch.pair_table(empty, cap)
            assert t.shape == (0,) and t.dtype == pkg.PAIR_DTYPE
    with pytest.raises(ValueError):
        batch.pair_table(FRAME_PAIRS, [1, 2])   # neither one room nor one per pair


def test_bf_select_and_logos_tables_keep_their_results():
    """The tables both wrappers returned before pair_table, for the same pairs: default, scalar and per-pair room, and no pairs."""
    batch = _batch()
    descs = types.SimpleNamespace(frames=types.SimpleNamespace(frame_off_host=np.concatenate([[0], np.cumsum(COUNTS)])))
    table = types.SimpleNamespace(n_frames=3, counts=COUNTS)
    bf = lambda cap: batch.bf_select_table(descs, FRAME_PAIRS, cap, max_size=30)
    logos = lambda cap: batch.logos_pair_table(table, FRAME_PAIRS, cap)
    for make, cap, m, off in ((bf, None, [10, 25, 30, 10, 0], [0, 10, 35, 65, 75]),        # min(max_size, n_a); a bad frame_a: 0
                              (bf, 7, [7] * 5, [0, 7, 14, 21, 28]),
                              (bf, [5, -2, 9, 0, 4], [5, -2, 9, 0, 4], [0, 5, 5, 14, 14]),
                              (logos, None, [40, 25, 40, 10, 25], [0, 40, 65, 105, 115]),   # the larger frame; a bad index: empty
                              (logos, 7, [7] * 5, [0, 7, 14, 21, 28]),
                              (logos, [5, 2, 9, 0, 4], [5, 2, 9, 0, 4], [0, 5, 7, 16, 16])):
        t = make(cap)
        assert t["m"].tolist() == m and t["match_off"].tolist() == off, cap
    assert batch.bf_select_table(descs, [], None).shape == (0,) and batch.logos_pair_table(table, [], None).shape == (0,)
    no_frames = types.SimpleNamespace(frames=types.SimpleNamespace(frame_off_host=np.array([0], np.int64)))
    t = batch.bf_select_table(no_frames, [(0, 1)], None)
    assert t["m"].tolist() == [0] and t["match_off"].tolist() == [0]
    t = batch.logos_pair_table(types.SimpleNamespace(n_frames=0, counts=np.zeros(0, np.int64)), [(0, 1)], None)
    assert t["m"].tolist() == [0] and t["match_off"].tolist() == [0]


def _stub(pkg, statuses, n_outs, calls):
    """A run callable whose k-th call reports statuses[k] / n_outs[k] and writes i + 100 * (k + 1) + j as queryIdx of pair i's
    j-th record, wherever the pair's match_off puts it."""
    def run(recs):
        k = len(calls)
        calls.append(recs.copy())
        res = np.zeros(len(recs), pkg.LOGOS_RESULT_DTYPE)
        res["status"], res["n_out"] = statuses[k], n_outs[k]
        out = np.zeros(int((recs["match_off"] + np.maximum(recs["m"], 0)).max()), pkg.DMATCH_DTYPE)
        for i, r in enumerate(recs):
            if res["status"][i] == 0:
                out["queryIdx"][r["match_off"]:r["match_off"] + res["n_out"][i]] = 100 * (k + 1) + 10 * i + np.arange(res["n_out"][i])
        return out, res
    return run


def test_run_with_retry_reruns_only_the_overflowing_pairs(pkg):
    batch = _batch()
    ty = importlib.import_module("sfm-gms_amd.types")
    recs = batch.pair_table([(0, 1), (1, 2), (2, 0)], [4, 3, 5])
    calls = []
    run = _stub(pkg, [(0, ty.GMS_ERR_CAPACITY, ty.GMS_ERR_DOMAIN), (0,)], [(2, 6, 0), (6,)], calls)
    got, res = batch.run_with_retry(recs, run)
    assert len(calls) == 2
    assert calls[0].tobytes() == recs.tobytes()
    again = calls[1]                                            # pair 1 alone, with the room it asked for, from offset 0
    assert (again["frame_a"].tolist(), again["frame_b"].tolist(), again["m"].tolist(), again["match_off"].tolist()) == ([1], [2], [6], [0])
    assert [g.dtype for g in got] == [pkg.DMATCH_DTYPE] * 3
    assert got[0]["queryIdx"].tolist() == [100, 101]            # first run, at its own offset
    assert got[1]["queryIdx"].tolist() == [200 + j for j in range(6)]   # second run
    assert len(got[2]) == 0                                     # GMS_ERR_DOMAIN: no survivors
    assert res["status"].tolist() == [0, 0, ty.GMS_ERR_DOMAIN] and res["n_out"].tolist() == [2, 6, 0]
    # a pair that overflows again keeps the second run's record and has no survivors; it is not run a third time
    calls = []
    run = _stub(pkg, [(ty.GMS_ERR_CAPACITY, 0, 0), (ty.GMS_ERR_CAPACITY,)], [(9, 1, 2), (11,)], calls)
    got, res = batch.run_with_retry(recs, run)
    assert len(calls) == 2 and calls[1]["m"].tolist() == [9] and calls[1]["frame_a"].tolist() == [0]
    assert [len(g) for g in got] == [0, 1, 2] and res["status"].tolist() == [ty.GMS_ERR_CAPACITY, 0, 0] and res["n_out"][0] == 11
    assert got[1]["queryIdx"].tolist() == [110] and got[2]["queryIdx"].tolist() == [120, 121]
    # no overflow: one run
    calls = []
    got, res = batch.run_with_retry(recs, _stub(pkg, [(0, 0, ty.GMS_ERR_BAD_ARG)], [(4, 0, 3)], calls))
    assert len(calls) == 1 and [len(g) for g in got] == [4, 0, 0]


def test_desc_layout(pkg):
    ty = importlib.import_module("sfm-gms_amd.types")
    api = importlib.import_module("sfm-gms_amd.api")
    assert ty.desc_layout(pkg.GMS_DESC_HAMMING256) == (np.uint8, 32)
    assert ty.desc_layout(np.int32(pkg.GMS_DESC_L2_F32X128)) == (np.float32, 128)
    for bad in (-1, 2, 7):
        with pytest.raises(ValueError, match="GMS_DESC_HAMMING256 or GMS_DESC_L2_F32X128"):
            ty.desc_layout(bad)
        with pytest.raises(ValueError, match="kind: GMS_DESC_HAMMING256 or GMS_DESC_L2_F32X128"):
            api.logos_dict_args(bad, 50, 3, 100)
    assert api.logos_dict_args(pkg.GMS_DESC_HAMMING256, 50, 3, 100) == (np.uint8, 32)


def test_concat_frames_and_its_callers_placeholders(pkg):
    ty = importlib.import_module("sfm-gms_amd.types")
    frames = [np.zeros(3, pkg.KEYPOINT_DTYPE), np.zeros(0, pkg.KEYPOINT_DTYPE), np.ones(2, pkg.KEYPOINT_DTYPE)]
    kp, off = ty.concat_frames(frames)
    assert kp.dtype == pkg.KEYPOINT_DTYPE and len(kp) == 5 and kp["x"].tolist() == [0, 0, 0, 1, 1]
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 3, 5]
    for none in ([], [np.zeros(0, pkg.KEYPOINT_DTYPE)] * 2):
        kp, off = ty.concat_frames(none)
        assert kp.shape == (0,) and kp.dtype == pkg.KEYPOINT_DTYPE and off.dtype == np.int64 and off.tolist() == [0] * (len(none) + 1)
