"""-m gpu: LOGOS at the edges of its domain, byte for byte. The named cases of tests/logos_cases.py (frames of 0 to 8 keypoints, empty
frames inside a table, coincident points, tied lattices, the value limits of angle and size, n_words at the 64-lane chunk edges, the
one-shot scan at 1024 queries, the k-NN tile at 256 points) through the one-shot gms_logos_match and through the batched path, each
against the statement tests/logos_ref.py and against each other; gms_logos_host_batch on a table with empty frames; the two refusals
the batched path makes on the device; and the keypoint domain on both paths.

No test here passes a finite |angle| > 3601 degrees: at the refused values used (logos_cases.REFUSED) the unguarded wrap loop ends
within 11 rounds, so a missing guard shows as a wrong status and cannot hang a kernel."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import logos_cases as LC
import logos_ref
from logos_gpu import GMS_ERR_BAD_ARG, GMS_ERR_DOMAIN, device_run, kp_records, oneshot, pkg, want_dmatch

pytestmark = pytest.mark.gpu
CASES = [c["name"] for c in LC.all_cases()]
CANARY = 0x5A


@functools.lru_cache(maxsize=None)
def _oneshot(name, a, b):
    c = LC.case(name)
    return oneshot(kp_records(c["frames"][a]), kp_records(c["frames"][b]), c["words"][a], c["words"][b])


def _lres(n_cand, n_supp, n_out, peak_bin, status=0):
    r = np.zeros(1, pkg.LOGOS_RESULT_DTYPE)
    r["n_candidates"], r["n_supported"], r["n_out"], r["peak_bin"], r["status"] = n_cand, n_supp, n_out, peak_bin, status
    return r[0]


def _statement_record(want, detail):
    return _lres(detail[0], detail[1], len(want), detail[2])


def _check_batch(ctx, table, fp, wants, ws_bytes=None):
    """One gms_logos_filter_device launch over the (frame_a, frame_b) pairs fp on a canary-filled d_out. wants[k]: the statement's
    (survivors, (n_candidates, n_supported, peak_bin)), or a status for a pair that must be refused with nothing written. Every range
    has exactly the room its survivors need (five records where the pair is refused); one canary record lies between two ranges
    and three behind the last."""
    n = len(fp)
    pairs = np.zeros(n, pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [p[0] for p in fp], [p[1] for p in fp]
    room = np.array([5 if isinstance(w, int) else len(w[0]) for w in wants], np.int64)
    pairs["m"] = room
    pairs["match_off"] = np.concatenate(([0], np.cumsum(room + 1)[:-1]))
    out, lres, pres = device_run(ctx, table, pairs, prefill=CANARY, extra=3, ws_bytes=ws_bytes)
    image = np.full(len(out), CANARY, np.uint8)
    for k, w in enumerate(wants):
        if isinstance(w, int):
            want_l, kept, st = _lres(0, 0, 0, -1, w), 0, w
        else:
            o = int(pairs["match_off"][k]) * 16
            image[o:o + 16 * len(w[0])] = np.frombuffer(want_dmatch(w[0]).tobytes(), np.uint8)
            want_l, kept, st = _statement_record(*w), len(w[0]), 0
        assert lres[k].tobytes() == want_l.tobytes(), (fp[k], lres[k], want_l)
        assert (pres["n_inliers"][k], pres["best_scale"][k], pres["best_rot"][k], pres["status"][k]) == (kept, -1, -1, st), fp[k]
    assert out.tobytes() == image.tobytes()      # survivors where they belong; every canary between and behind the ranges intact
    return lres


# ---- 1. every case through the one-shot -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_oneshot_equals_statement(name):
    for a, b in LC.case(name)["pairs"]:
        want, detail = LC.expected(name, a, b)
        got, res = _oneshot(name, a, b)
        assert got.tobytes() == want_dmatch(want).tobytes(), (a, b)
        assert res.tobytes() == _statement_record(want, detail).tobytes(), (a, b, res)


# ---- 2. every case through the batched path: one table per case, one launch over all its pairs ----------------------------------
@pytest.mark.parametrize("name", CASES)
def test_batch_equals_statement_and_oneshot(ctx, name):
    batch = importlib.import_module("sfm-gms_amd.batch")
    c = LC.case(name)
    table = batch.LogosTable(ctx, [kp_records(f) for f in c["frames"]], list(c["words"]), c["n_words"])
    fp = list(c["pairs"])
    lres = _check_batch(ctx, table, fp, [LC.expected(name, a, b) for a, b in fp])
    for k, (a, b) in enumerate(fp):
        assert lres[k].tobytes() == _oneshot(name, a, b)[1].tobytes(), (a, b)
    # the same pairs in reverse order with a workspace that held something else before
    got, lres2 = batch.logos_pairs(ctx, table, fp[::-1])
    for k, (a, b) in enumerate(fp[::-1]):
        assert got[k].tobytes() == _oneshot(name, a, b)[0].tobytes() and lres2[k].tobytes() == lres[len(fp) - 1 - k].tobytes()


def test_pairs_with_an_empty_frame_are_ok_and_empty(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    c = LC.case("empty_in_table")
    table = batch.LogosTable(ctx, [kp_records(f) for f in c["frames"]], list(c["words"]), c["n_words"])
    n = LC.EMPTY_TABLE_COUNTS
    fp = [(a, b) for a, b in c["pairs"] if n[a] == 0 or n[b] == 0]
    assert len(fp) == 100 - 49
    empty = (np.zeros((0, 2), np.int32), (0, 0, -1))
    lres = _check_batch(ctx, table, fp, [empty] * len(fp))
    assert (lres["status"] == 0).all()
    # only empty frames in a table: no keypoint at all
    none = batch.LogosTable(ctx, [kp_records(np.zeros((0, 4)))] * 3, [np.zeros(0, np.int32)] * 3, 5)
    _check_batch(ctx, none, [(0, 1), (2, 2)], [empty] * 2)


# ---- 3. gms_logos_host_batch on the table with empty frames ---------------------------------------------------------------------
def test_host_batch_with_empty_frames(ctx):
    lib = pkg.load_library()
    c = LC.case("empty_in_table")
    kp_all, frame_off = pkg.types.concat_frames([kp_records(f) for f in c["frames"]])
    frame_off = np.ascontiguousarray(frame_off, np.int64)
    words = np.ascontiguousarray(np.concatenate(c["words"]), np.int32)
    fp = list(c["pairs"])
    wants = [LC.expected("empty_in_table", a, b) for a, b in fp]
    pairs = np.zeros(len(fp), pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [p[0] for p in fp], [p[1] for p in fp]
    room = np.array([len(w[0]) for w in wants], np.int64)
    pairs["m"] = room
    pairs["match_off"] = np.concatenate(([0], np.cumsum(room + 1)[:-1]))
    total = int(pairs["match_off"][-1] + room[-1])
    out = np.zeros(total, pkg.DMATCH_DTYPE)
    res = np.zeros(len(fp), pkg.LOGOS_RESULT_DTYPE)
    rc = lib.gms_logos_host_batch(ctx._h, kp_all.ctypes.data, frame_off.ctypes.data, len(c["frames"]), words.ctypes.data, c["n_words"],
                                  pairs.ctypes.data, len(fp), out.ctypes.data, res.ctypes.data)
    assert rc == 0
    for k, w in enumerate(wants):
        o = int(pairs["match_off"][k])
        assert res[k].tobytes() == _statement_record(*w).tobytes(), fp[k]
        assert out[o:o + len(w[0])].tobytes() == want_dmatch(w[0]).tobytes(), fp[k]


# ---- 4. the two refusals the batched path makes on the device -------------------------------------------------------------------
class _PrepareWorkspaceFor:
    """A context whose prepare workspace is sized for frames of at most max_kp keypoints (what a caller who sized it for other
    frames would pass); everything else is the context's."""

    def __init__(self, ctx, max_kp):
        self._ctx, self._max_kp = ctx, max_kp

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def logos_workspace_bytes(self, max_frame_kp, n_pairs, max_query_kp):
        return self._ctx.logos_workspace_bytes(min(max_frame_kp, self._max_kp) if n_pairs == 0 else max_frame_kp, n_pairs, max_query_kp)


def test_tied_frame_larger_than_the_prepare_slice_is_refused(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    we = LC.case("word_edges_63")
    frames = [LC.case("coincident_40")["frames"][0], we["frames"][0], LC.case("coincident_7")["frames"][0]]
    words = [np.zeros(40, np.int32), we["words"][0], np.zeros(7, np.int32)]
    assert ctx.logos_workspace_bytes(7, 0, 0) == 512 * 8 * 6        # slices of six records: coincident_7's m = 6 just fits
    table = batch.LogosTable(_PrepareWorkspaceFor(ctx, 7), [kp_records(f) for f in frames], words, 63)
    with np.errstate(all="ignore"):
        exact = {k: logos_ref.match(frames[k], frames[k], words[k], words[k], detail=True) for k in (1, 2)}
    assert len(exact[1][0]) >= 300 and exact[2][1] == (49, 0, -1)
    fp = [(0, 0), (1, 1), (0, 1), (2, 2), (1, 0), (2, 0), (0, 2), (1, 1)]
    _check_batch(ctx, table, fp, [GMS_ERR_BAD_ARG if 0 in p else exact[p[0]] for p in fp])
    # with the workspace the table asks for, the same frames are all served
    table = batch.LogosTable(ctx, [kp_records(f) for f in frames], words, 63)
    lres = _check_batch(ctx, table, [(0, 0), (1, 1)], [LC.expected("coincident_40", 0, 0), exact[1]])
    assert (lres["status"] == 0).all()


def test_pair_whose_queries_do_not_fit_the_filter_workspace_is_refused(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    c = LC.case("tiny")
    table = batch.LogosTable(ctx, [kp_records(f) for f in c["frames"]], list(c["words"]), c["n_words"])
    fp = list(c["pairs"])
    fixed = ctx.logos_workspace_bytes(0, len(fp), 0)
    assert fixed > 512 * 8                                             # the filter's fixed part, not the prepare minimum
    queries = sum(len(c["frames"][a]) for a, _ in fp)
    assert len(c["frames"][fp[-1][0]]) == 40
    wants = [LC.expected("tiny", a, b) for a, b in fp]
    _check_batch(ctx, table, fp, wants, ws_bytes=fixed + 8 * queries)                       # exactly enough
    _check_batch(ctx, table, fp, wants[:-1] + [GMS_ERR_BAD_ARG], ws_bytes=fixed + 8 * (queries - 1))   # one query short


# ---- 5. the keypoint domain -----------------------------------------------------------------------------------------------------
def test_batch_marks_frames_outside_the_domain(ctx):
    batch = importlib.import_module("sfm-gms_amd.batch")
    c = LC.domain_refusals()
    frames = [kp_records(f) for f in c["frames"]]
    for f, (field, v) in enumerate(LC.REFUSED):
        bad = ~logos_ref.kp_ok(c["frames"][f][:, 0], c["frames"][f][:, 1], c["frames"][f][:, 3])
        assert bad.sum() == 1 and (np.isnan(v) or frames[f][field][bad][0] == np.float32(v))
    table = batch.LogosTable(ctx, frames, list(c["words"]), c["n_words"])
    with np.errstate(all="ignore"):
        clean = logos_ref.match(c["frames"][5], c["frames"][5], c["words"][5], c["words"][5], detail=True)
    assert len(clean[0]) >= 50
    fp = list(c["pairs"])
    _check_batch(ctx, table, fp, [clean if p == (5, 5) else GMS_ERR_DOMAIN for p in fp])
    got, res = oneshot(frames[5], frames[5], c["words"][5], c["words"][5])
    assert got.tobytes() == want_dmatch(clean[0]).tobytes() and res.tobytes() == _statement_record(*clean).tobytes()


@pytest.mark.parametrize("f", range(len(LC.REFUSED)))
@pytest.mark.parametrize("role", [0, 1])
def test_oneshot_refuses_outside_the_domain(f, role):
    lib = pkg.load_library()
    c = LC.domain_refusals()
    kps = [kp_records(c["frames"][5]), kp_records(c["frames"][5])]
    kps[role] = kp_records(c["frames"][f])
    l = np.ascontiguousarray(c["words"][5])
    out = np.full(16 * 64, CANARY, np.uint8)
    n = C.c_int64(9)
    res = np.zeros(1, pkg.LOGOS_RESULT_DTYPE)
    rc = lib.gms_logos_match(kps[0].ctypes.data, 50, kps[1].ctypes.data, 50, l.ctypes.data, l.ctypes.data, out.ctypes.data, 64,
                             C.byref(n), res.ctypes.data)
    assert rc == GMS_ERR_DOMAIN and n.value == 0 and res[0].tobytes() == _lres(0, 0, 0, -1, GMS_ERR_DOMAIN).tobytes()
    assert (out == CANARY).all()
    with pytest.raises(pkg.GmsError) as e:
        pkg.matchLOGOS(kps[0], kps[1], l, l)
    assert e.value.code == GMS_ERR_DOMAIN
