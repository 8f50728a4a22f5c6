"""CPU: the definition of the LOGOS dictionary trainer (DESIGN.md §6b "Training the dictionary"). tests/logos_dict_ref.py states it in
numpy; sfm-gms_amd/csrc/logos_dict_core.h is what the kernels run, compiled here for the host (tests/cpp/logos_dict_host.cpp). The
GPU is held to the statement's bytes in tests/test_gpu_logos_dict.py."""
import ctypes as C

import numpy as np
import pytest

import logos_dict_cases as cases
import logos_dict_ref as ref
import logos_words_ref
import hostbuild as hb

HAMMING, L2 = ref.HAMMING, ref.L2


def blobs(kind, n_words, per_blob, seed):
    """n_words planted blobs, shuffled -> (rows, blob of each row). L2: centres 600 apart on their own axis pairs, noise within
    +-1 per element (so rows of one blob are within 128 * 4 = 512 of each other squared, rows of two blobs at least 598^2 apart).
    Hamming: centres with disjoint runs of 2 set bytes (16 bits; 32 apart), at most 2 bits flipped per row (rows of one blob within
    4 of each other, of two blobs at least 28 apart). A covered blob's rows weigh at most 512 * 256 against 598^2 * 256 for one uncovered
    row (L2), at most 4 against 28 (Hamming), so k-means++ draws nearly every new centre from a blob that has none, and the best of
    three trials is one of those; the test checks that the statement does so for every seed it tries."""
    rng = np.random.default_rng(seed)
    which = np.repeat(np.arange(n_words), per_blob)
    rng.shuffle(which)
    if kind == L2:
        assert n_words <= 128
        centres = np.zeros((n_words, 128), np.float32)
        centres[np.arange(n_words), np.arange(n_words)] = 600.0
        rows = centres[which] + rng.uniform(-1.0, 1.0, (len(which), 128)).astype(np.float32)
        return rows.astype(np.float32), which
    assert n_words <= 16
    centres = np.zeros((n_words, 32), np.uint8)
    for c in range(n_words):
        centres[c, 2 * c:2 * c + 2] = 0xFF
    rows = centres[which].copy()
    for i in range(len(rows)):
        for b in rng.choice(256, 2, replace=False):
            rows[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return rows, which


def random_rows(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == L2:
        return rng.uniform(0.0, 255.0, (n, 128)).astype(np.float32)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def test_the_statements_distances_are_the_words_calls():
    a, b = random_rows(HAMMING, 500, 8), random_rows(HAMMING, 70, 9)
    assert ref.distances(a, b, HAMMING).tobytes() == logos_words_ref.hamming_distances(a, b).tobytes()
    x, y = random_rows(L2, 300, 8), random_rows(L2, 70, 9)
    assert ref.distances(x, y, L2).tobytes() == logos_words_ref.l2_distances(x, y).tobytes()


# ---- the statement's own properties ---------------------------------------------------------------------------------------------
def test_draws_are_a_function_of_their_five_keys():
    base = ref.draw(7, 1, 2, 3, 1)
    assert base == ref.draw(7, 1, 2, 3, 1)
    others = {ref.draw(8, 1, 2, 3, 1), ref.draw(7, 2, 2, 3, 1), ref.draw(7, 1, 0, 3, 1), ref.draw(7, 1, 2, 4, 1), ref.draw(7, 1, 2, 3, 2)}
    assert base not in others and len(others) == 5
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF   # splitmix64's first output for state 0
    assert ref.mulhi64((1 << 64) - 1, 10) == 9 and ref.mulhi64(1 << 63, 10) == 5 and ref.mulhi64(0, 10) == 0


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_same_seed_same_bytes_other_seed_or_set_other_draws(kind):
    rows = random_rows(kind, 300, 1)
    a = ref.train_set(rows, kind, 8, 2, 20, seed=5, set_index=0, detail=True)
    b = ref.train_set(rows, kind, 8, 2, 20, seed=5, set_index=0, detail=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    c = ref.train_set(rows, kind, 8, 2, 20, seed=6, set_index=0, detail=True)
    d = ref.train_set(rows, kind, 8, 2, 20, seed=5, set_index=1, detail=True)
    assert a[3][0]["seed_rows"] != c[3][0]["seed_rows"] and a[3][0]["seed_rows"] != d[3][0]["seed_rows"]
    assert a[3][0]["seed_rows"] != a[3][1]["seed_rows"]   # attempts draw differently too


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_compactness_never_rises_and_the_winner_is_the_minimum(kind):
    rows = random_rows(kind, 400, 2)
    for seed in range(3):
        dic, rec, labels, runs = ref.train_set(rows, kind, 10, 3, 100, seed=seed, detail=True)
        comps = [r["compactness"] for r in runs]
        # the mean minimises the sum of squared distances of a cluster, the bit majority its Hamming sum
        assert all(r["compactness"] <= r["seed_compactness"] for r in runs)
        assert rec["compactness"] == min(comps) and rec["attempt"] == comps.index(min(comps))
        assert rec["iterations"] == runs[rec["attempt"]]["iterations"] <= 100
        # the labels returned are the words of the rows under the dictionary returned
        assert np.array_equal(labels, logos_words_ref.words(rows, dic, kind))
        assert rec["empty_clusters"] == 10 - len(np.unique(labels))


@pytest.mark.parametrize("kind,n_words,per_blob", [(L2, 50, 6), (L2, 100, 3), (HAMMING, 16, 12)])
def test_planted_blobs_get_one_centre_each(kind, n_words, per_blob):
    rows, which = blobs(kind, n_words, per_blob, 3)
    for seed in (0, 1, 2, 12345, 2**63 + 11):
        dic, rec, labels = ref.train_set(rows, kind, n_words, 3, 100, seed=seed)
        assert rec["status"] == 0 and rec["empty_clusters"] == 0
        word_of_blob = {}
        for b, w in zip(which, labels):
            assert word_of_blob.setdefault(int(b), int(w)) == int(w)       # every row takes its blob's word
        assert sorted(word_of_blob.values()) == list(range(n_words))      # and every blob a word of its own


def test_hamming_majority_tie_gives_zero():
    rows = np.zeros((4, 32), np.uint8)
    rows[:2, 0] = 0b0000_0101     # bits 0 and 2 set in two of four rows: ties
    rows[:3, 1] = 0b0000_0010     # bit 9 set in three of four
    new = ref.update(rows, np.zeros(4, np.int32), np.zeros((1, 32), np.uint8), HAMMING)
    assert new[0, 0] == 0 and new[0, 1] == 0b10 and not new[0, 2:].any()


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_an_empty_cluster_keeps_its_centre_and_is_counted(kind):
    rows = random_rows(kind, 20, 4)
    centres = rows[:3].copy()
    labels = np.array([0, 2] * 10, np.int32)
    new = ref.update(rows, labels, centres, kind)
    assert new[1].tobytes() == centres[1].tobytes() and new[0].tobytes() != centres[0].tobytes()
    # three distinct rows, five words: the duplicates leave two words without rows
    dup = np.concatenate([rows[:3]] * 4)
    dic, rec, lab = ref.train_set(dup, kind, 5, 2, 10, seed=1)
    assert rec["status"] == 0 and rec["empty_clusters"] == 2 and rec["compactness"] == 0
    assert np.array_equal(lab, logos_words_ref.words(dup, dic, kind))


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_zero_total_weight_draws_a_row_directly(kind):
    rows = np.concatenate([random_rows(kind, 1, 5)] * 9)     # one distinct row
    trace = []
    chosen = ref.seed_centres(rows, kind, 3, seed=3, set_index=2, attempt=1, trace=trace)
    assert [t["total"] for t in trace] == [0, 0]
    for t in trace:
        assert t["candidates"] == [ref.mulhi64(ref.draw(3, 2, 1, t["centre"], k), 9) for k in range(3)]
        assert t["potentials"] == [0, 0, 0] and t["kept"] == 0      # ties keep the lowest trial
    assert chosen[1:] == [t["candidates"][0] for t in trace]


def test_statuses_for_sets_outside_the_domain():
    ok = random_rows(L2, 12, 6)
    assert ref.train_set(ok, L2, 12, 1, 2)[1]["status"] == 0
    dic, rec, lab = ref.train_set(ok, L2, 13, 1, 2)
    assert rec["status"] == ref.GMS_ERR_BAD_ARG and rec["attempt"] == -1 and not dic.any() and (lab == -1).all()
    for bad in (np.nan, np.inf, -np.inf, 4096.5, -5000.0):
        x = ok.copy()
        x[7, 100] = bad
        assert ref.train_set(x, L2, 4, 1, 2)[1]["status"] == ref.GMS_ERR_DOMAIN
    x = ok.copy()
    x[0, 0], x[1, 1] = 4096.0, -4096.0
    assert ref.train_set(x, L2, 4, 1, 2)[1]["status"] == 0
    assert ref.train_set(random_rows(HAMMING, 3, 1), HAMMING, 4)[1]["status"] == ref.GMS_ERR_BAD_ARG
    # in a batch the other sets are unaffected
    x = np.concatenate([ok, ok[:5], ok])
    x[14, 3] = np.nan
    dicts, recs, labels = ref.train(x, [0, 12, 17, 29], L2, 4, 2, 10, seed=9)
    assert recs["status"].tolist() == [0, ref.GMS_ERR_DOMAIN, 0] and not dicts[1].any() and (labels[12:17] == -1).all()
    alone = ref.train_set(ok, L2, 4, 2, 10, seed=9, set_index=2)
    assert dicts[2].tobytes() == alone[0].tobytes() and recs[2].tobytes() == alone[1].tobytes()


def test_the_bounds_keep_every_sum_exact():
    # the largest L2 distance: 128 dimensions 8192 apart; its weight; a set's potential; the largest sum of quantised elements
    d_max = 128 * 8192.0 ** 2
    assert d_max == 2.0 ** 33 and np.float32(d_max) * np.float32(256) == 2.0 ** 41
    assert (2 ** 41) * ref.MAX_SET_ROWS == 2 ** 61 < 2 ** 63
    assert int(ref.quantise(np.float32(4096.0))) == 2 ** 32 and 2 ** 32 * ref.MAX_SET_ROWS == 2 ** 52 < 2 ** 53
    assert 256 * ref.MAX_SET_ROWS < 2 ** 63     # Hamming


def test_quantised_mean_by_hand():
    # 0.5, 0.25 and 2^-21 (rint(0.5) = 0: ties to even) -> S = 786432 -> 0.25 exactly; 1.5 2^-20 rounds to 2 2^-20
    x = np.array([0.5, 0.25, 2.0 ** -21], np.float32)
    assert ref.quantise(x).tolist() == [524288, 262144, 0]
    assert ref.l2_mean(786432, 3) == np.float32(0.25)
    assert ref.quantise(np.float32(1.5 * 2.0 ** -20)) == 2 and ref.quantise(np.float32(-2.5 * 2.0 ** -20)) == -2
    # one third: S = 3 * 349525 + 1 over 9 rows does not hit a float exactly: the double quotient is rounded once
    assert ref.l2_mean(1048576, 3) == np.float32(np.float64(1.0) / np.float64(3.0))
    rows = np.zeros((3, 128), np.float32)
    rows[:, 0] = x
    rows[:, 1] = [1.0, 2.0, 4.0]
    new = ref.update(rows, np.zeros(3, np.int32), np.zeros((1, 128), np.float32), L2)
    assert new[0, 0] == np.float32(0.25) and new[0, 1] == np.float32(np.float64(7 * 2 ** 20) / np.float64(3 * 2 ** 20))


# ---- logos_dict_core.h, built for the host, against the statement -----------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(hb.host_lib("logos_dict_host.cpp"))
    vp, u64, i64 = C.c_void_p, C.c_ulonglong, C.c_longlong
    lib.dict_host_draw.argtypes = [u64] * 5
    lib.dict_host_draw.restype = u64
    lib.dict_host_mulhi64.argtypes = [u64, u64]
    lib.dict_host_mulhi64.restype = u64
    lib.dict_host_l2.argtypes = [vp, i64, vp, vp, vp]
    lib.dict_host_hamming.argtypes = [vp, i64, vp, vp]
    lib.dict_host_in_domain.argtypes = [vp, i64, vp]
    lib.dict_host_quantise.argtypes = [vp, i64, vp]
    lib.dict_host_mean.argtypes = [vp, i64, C.c_int, vp]
    lib.dict_host_majority.argtypes = [i64, i64]
    lib.dict_host_workspace_bytes.argtypes = [C.c_int, i64, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.dict_host_workspace_bytes.restype = i64
    return lib


def test_host_draws_equal_the_statement(host):
    rng = np.random.default_rng(0)
    for _ in range(200):
        k = [int(v) for v in rng.integers(0, 2 ** 63, 5)]
        k[0] = k[0] * 2 + 1
        assert host.dict_host_draw(*k) == ref.draw(*k)
        assert host.dict_host_mulhi64(k[0], k[1]) == ref.mulhi64(k[0], k[1])


def test_host_distances_and_weights_equal_the_statement(host):
    rng = np.random.default_rng(1)
    rows = np.concatenate([rng.uniform(-4096, 4096, (200, 128)), rng.uniform(0, 1, (200, 128)), rng.uniform(0, 255, (200, 128))])
    rows = rows.astype(np.float32)
    centre = rng.uniform(-300, 300, 128).astype(np.float32)
    d, w = np.zeros(len(rows), np.float32), np.zeros(len(rows), np.uint64)
    host.dict_host_l2(rows.ctypes.data, len(rows), centre.ctypes.data, d.ctypes.data, w.ctypes.data)
    want = ref.distances(rows, centre[None], L2)[:, 0]
    assert d.tobytes() == want.tobytes() and w.tobytes() == ref.weights(want, L2).tobytes()
    h = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    hw = np.zeros(len(h), np.uint64)
    host.dict_host_hamming(h.ctypes.data, len(h), h[17].ctypes.data, hw.ctypes.data)
    assert hw.tobytes() == ref.weights(ref.distances(h, h[17:18], HAMMING)[:, 0], HAMMING).tobytes()
    x = np.array([0.0, 4096.0, -4096.0, 4096.0005, np.nan, np.inf, -np.inf, 1e-40], np.float32)
    ok = np.zeros(len(x), np.int32)
    host.dict_host_in_domain(x.ctypes.data, len(x), ok.ctypes.data)
    assert ok.tolist() == [1, 1, 1, 0, 0, 0, 0, 1]


def test_host_quantised_mean_equals_the_statement(host):
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-4096, 4096, 5000), rng.uniform(-1e-5, 1e-5, 1000), (rng.integers(-9, 9, 200) + 0.5) * 2.0 ** -20,
                        [1e-42, -1e-42, 4096.0, -4096.0]]).astype(np.float32)
    q = np.zeros(len(x), np.int64)
    host.dict_host_quantise(x.ctypes.data, len(x), q.ctypes.data)
    assert q.tobytes() == ref.quantise(x).tobytes()
    for n in (1, 3, 7, 100):
        rows = rng.uniform(0, 255, (n, 128)).astype(np.float32)
        out = np.zeros(128, np.float32)
        host.dict_host_mean(rows.ctypes.data, n, 128, out.ctypes.data)
        assert out.tobytes() == ref.update(rows, np.zeros(n, np.int32), np.zeros((1, 128), np.float32), L2)[0].tobytes()
    assert [host.dict_host_majority(o, 4) for o in range(5)] == [0, 0, 0, 1, 1]


def test_workspace_sizes_and_refused_arguments(host, pkg):
    lib = pkg.load_library()
    assert lib.gms_logos_dict_workspace_bytes(1, 10000, 1, 50, 3, 100) >= host.dict_host_workspace_bytes(1, 10000, 1, 50, 3, 100) > 0
    sizes = [lib.gms_logos_dict_workspace_bytes(0, n, 4, 50, 3, 100) for n in (0, 1000, 100000)]
    assert sizes == sorted(sizes) and sizes[2] - sizes[1] >= 99000 * 3 * 12      # a weight and a label per row and attempt
    for bad in [(2, 10, 1, 50, 3, 100), (1, -1, 1, 50, 3, 100), (1, 10, -1, 50, 3, 100), (1, 10, 1, 0, 3, 100), (1, 10, 1, 65536, 3, 100),
                (1, 10, 1, 50, 0, 100), (1, 10, 1, 50, 17, 100), (1, 10, 1, 50, 3, 0), (1, 10, 1, 50, 3, 1001), (1, 10, 65536, 50, 3, 100)]:
        assert lib.gms_logos_dict_workspace_bytes(*bad) == 0, bad
    off = np.array([0, 10], np.int64)
    res = np.zeros(1, pkg.LOGOS_DICT_RESULT_DTYPE)
    # no context / bad parameters: refused before any device work
    assert lib.gms_logos_dict_train_device(None, 1, None, off.ctypes.data, 1, 10, 5, 3, 100, 0, None, 0, None, res.ctypes.data, None) == -1
    assert lib.gms_logos_dict_train(1, None, off.ctypes.data, 1, 0, 3, 100, 0, None, res.ctypes.data, None) == -1
    assert lib.gms_logos_dict_train(3, None, off.ctypes.data, 1, 5, 3, 100, 0, None, res.ctypes.data, None) == -1
    assert lib.gms_logos_dict_train(1, None, None, 1, 5, 3, 100, 0, None, res.ctypes.data, None) == -1


def test_python_layer_checks_its_arguments_first(pkg):
    with pytest.raises(ValueError, match="n_words"):
        pkg.trainLogosDictionary(np.zeros((10, 32), np.uint8), pkg.GMS_DESC_HAMMING256, n_words=0)
    with pytest.raises(ValueError, match="kind"):
        pkg.trainLogosDictionary(np.zeros((10, 32), np.uint8), 5)
    import importlib
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    with pytest.raises(ValueError, match="rows"):
        pipeline.dictionary_training_options({"rows": "second"})
    assert pipeline.dictionary_training_options(True) == {"rows": "first", "n_words": 50, "attempts": 3, "max_iters": 100, "seed": 0}
    assert pipeline.dictionary_training_options({"n_words": 100, "rows": "all"})["n_words"] == 100


# ---- the cases of tests/logos_dict_cases.py reach the regimes they are named for ----------------------------------------------------
# The GPU is held to the statement's bytes on these inputs in tests/test_gpu_logos_dict.py; here the statement's own trace shows
# that each input makes the kernels leave the first pass of the loop it is there for.
def seeding_traces(rows, kind, args, set_index):
    """Per attempt: (the centres' rows, the trace of seed_centres)."""
    out = []
    for a in range(args["attempts"]):
        trace = []
        chosen = ref.seed_centres(rows, kind, args["n_words"], args["seed"], set_index, a, trace=trace)
        out.append((chosen, trace))
    return out


def assert_candidates_spread(rows, kind, args, set_index, min_chunks):
    cands = np.array([c for _, trace in seeding_traces(rows, kind, args, set_index) for t in trace for c in t["candidates"]])
    chunks = np.unique(cands // cases.CHUNK)
    print(f"set {set_index}: {len(rows)} rows, {cases.n_chunks(len(rows))} chunks; {len(cands)} candidates in {len(chunks)} chunks, "
          f"{int((cands >= len(rows) // 2).sum())} in the upper half, {int((cands >= cases.last_chunk(len(rows))).sum())} in the last chunk")
    assert len(chunks) >= min_chunks
    assert (cands >= len(rows) // 2).any()
    assert (cands >= cases.last_chunk(len(rows))).any()


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_long_sets_scan_several_chunks_per_thread(kind):
    sets, args = cases.long_sets(kind)
    assert [len(s) for s in sets] == [300, 65536, 65537, 131329] and (args["n_words"], args["attempts"], args["max_iters"]) == (4, 2, 3)
    # 256 chunks: the most with one chunk per thread of the scan; 257 and 514: two and three per thread. No long set starts at chunk 0.
    assert [cases.n_chunks(len(s)) for s in sets] == [2, 256, 257, 514]
    assert [-(-cases.n_chunks(len(s)) // 256) for s in sets] == [1, 1, 2, 3]
    assert [len(s) - cases.last_chunk(len(s)) for s in sets[1:]] == [256, 1, 1]
    for s in range(1, 4):
        assert ref.set_status(sets[s], kind, args["n_words"]) == 0
        assert_candidates_spread(sets[s], kind, args, s, 8)


def test_case_max_rows_set_and_one_row_more():
    sets, args = cases.max_rows_sets()
    assert [len(s) for s in sets] == [1 << 20, (1 << 20) + 1] and (args["n_words"], args["attempts"], args["max_iters"]) == (3, 1, 2)
    assert cases.n_chunks(len(sets[0])) == 4096      # 16 chunks per thread of the scan
    assert ref.set_status(sets[0], HAMMING, 3) == 0 and ref.set_status(sets[1], HAMMING, 3) == ref.GMS_ERR_BAD_ARG
    # two centres are drawn, three trials each, one attempt: six candidates in all, so six distinct chunks is the most there can be
    assert_candidates_spread(sets[0], HAMMING, args, 0, 6)


def longest_zero_run(sums):
    best = run = 0
    for v in sums:
        run = run + 1 if v == 0 else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_zero_weight_runs_make_the_prefix_flat(kind):
    sets, args = cases.zero_weight_runs(kind)
    rows = sets[0]
    assert len(rows) == 67513 and len(np.unique(rows, axis=0)) == 5 < args["n_words"] == 6
    assert (args["attempts"], args["max_iters"]) == (2, 3)
    seen = {"flat run": False, "chunk 0 empty": False, "last chunk empty": False, "equal potentials": False}
    for a, (chosen, trace) in enumerate(seeding_traces(rows, kind, args, 0)):
        w = None
        for t in trace:
            c = t["centre"]
            wc = ref.weights(ref.distances(rows, rows[chosen[c - 1]:chosen[c - 1] + 1], kind)[:, 0], kind)
            w = wc if w is None else np.minimum(w, wc)
            sums = np.add.reduceat(w, np.arange(0, len(rows), cases.CHUNK))
            assert int(sums.sum(dtype=np.uint64)) == t["total"]
            print(f"centre {c}: total {t['total']}, {int((sums == 0).sum())} of {len(sums)} chunks empty, longest run {longest_zero_run(sums)}, "
                  f"candidates {t['candidates']} potentials {t['potentials']} kept {t['kept']}")
            if t["total"] > 0:
                seen["flat run"] |= longest_zero_run(sums) >= 100
                seen["chunk 0 empty"] |= sums[0] == 0
                seen["last chunk empty"] |= sums[-1] == 0
            if len(set(t["potentials"])) == 1:
                seen["equal potentials"] = True
                assert t["kept"] == 0
        assert trace[-1]["centre"] == 5 and trace[-1]["total"] == 0      # the last centre: mulhi64(u, n) on a long set
        assert trace[-1]["candidates"] == [ref.mulhi64(ref.draw(args["seed"], 0, a, 5, k), len(rows)) for k in range(3)]
    assert all(seen.values()), seen


@pytest.mark.parametrize("kind,n_words", [(HAMMING, 512), (HAMMING, 513), (HAMMING, 1030), (L2, 129)])
def test_case_many_words_fill_more_than_one_tile(kind, n_words):
    sets, args = cases.many_words(kind, n_words)
    assert len(sets[0]) == (1100 if kind == HAMMING else 400) and (args["attempts"], args["max_iters"]) == (1, 3)
    dic, rec, labels = (v[0] if i != 2 else v for i, v in enumerate(cases.expected("many_words", kind, n_words)))
    assert rec["status"] == 0
    tiles = cases.tiles_at_minimum(sets[0], dic, kind)
    print(f"{n_words} words: record {rec}, highest label {labels.max()}, {int((tiles >= 2).sum())} rows nearest to words of two tiles")
    if n_words == 512:      # exactly one full tile: its last word is used, and there is no second tile to tie with
        assert labels.max() == 511
        return
    assert labels.max() >= (128 if kind == L2 else 512)
    if n_words == 1030:
        assert labels.max() >= 1024
    # such a row's label is the first word at the minimum, which lies in the earlier tile: "lowest index wins" across tiles
    assert (tiles >= 2).any()


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_many_sets_more_than_one_pass_of_the_plan(kind):
    sets, args = cases.many_sets(kind)
    assert len(sets) == 300 and all(len(s) == 3 if k in cases.TOO_FEW else 6 <= len(s) <= 14 for k, s in enumerate(sets))
    assert (args["n_words"], args["attempts"], args["max_iters"]) == (4, 2, 5)
    dic, rec, labels = cases.expected("many_sets", kind)
    assert rec["status"].tolist() == cases.many_sets_statuses(kind).tolist()
    assert rec["status"][[0, 255, 256, 299]].tolist() == [ref.GMS_ERR_BAD_ARG] * 4
    assert rec["status"][257] == (ref.GMS_ERR_DOMAIN if kind == L2 else 0) and int((rec["status"] != 0).sum()) == (5 if kind == L2 else 4)
    off = cases.flat(sets, kind)[1]
    for s in np.flatnonzero(rec["status"] != 0):
        assert not dic[s].any() and (labels[off[s]:off[s + 1]] == -1).all() and rec["attempt"][s] == -1
    for s in (1, 254, 258, 298):      # the neighbours of the failed sets are what they are alone
        alone = ref.train_set(sets[s], kind, set_index=s, **args)
        assert dic[s].tobytes() == alone[0].tobytes() and rec[s].tobytes() == alone[1].tobytes()
        assert labels[off[s]:off[s + 1]].tobytes() == alone[2].tobytes()


def test_case_l2_domain_edge_has_the_largest_sums():
    sets, args = cases.l2_domain_edge()
    rows = sets[0]
    assert len(rows) == 600 and (args["n_words"], args["attempts"], args["max_iters"]) == (8, 2, 6)
    assert (rows == 4096.0).any() and (rows == -4096.0).any() and np.abs(rows).max() == 4096.0
    corners = np.delete(rows, np.arange(0, 600, 7), axis=0)
    assert (np.abs(corners) == 4096.0).all() and (np.abs(rows[::7]) < 4096.0).any()
    dic, rec, labels = cases.expected("l2_domain_edge", L2)
    print(f"record {rec[0]}: compactness 2^{np.log2(float(rec[0]['compactness'])):.2f}")
    assert rec[0]["status"] == 0 and int(rec[0]["compactness"]) > 2 ** 47
    for x in cases.just_outside_the_domain():
        assert np.abs(x).max() > 4096.0 and np.float32(np.abs(x).max()) == np.nextafter(np.float32(4096.0), np.float32(np.inf))
        assert ref.set_status(x, L2, 8) == ref.GMS_ERR_DOMAIN


def test_case_l2_rounding_ties_tell_ties_to_even_from_half_away(monkeypatch):
    sets, args, blob = cases.l2_rounding_ties()
    rows = sets[0]
    scaled = rows.astype(np.float64) * 1048576.0
    ties = np.abs(scaled - np.floor(scaled)) == 0.5
    tie_rows = ties.all(axis=1)
    # the ordinary rows have elements that are no ties (of those with |x| >= 4 every other float is one: the spacing there is 2^-21)
    assert tie_rows.sum() == len(rows) - 2 * len(cases.TIE_BLOB_SIZES) and (~ties[~tie_rows]).sum() > 128
    assert (scaled[ties] > 0).any() and (scaled[ties] < 0).any()
    even = np.floor(scaled[ties]) % 2 == 0          # k + 0.5 with k even: rint rounds down; with k odd: up
    assert even.any() and (~even).any()
    dic, rec, labels = cases.expected("l2_rounding_ties", L2)
    assert rec[0]["status"] == 0 and rec[0]["empty_clusters"] == 0 and rec[0]["iterations"] >= 2      # an update ran
    counts = np.bincount(labels[:len(rows)], minlength=args["n_words"])
    assert sorted(counts.tolist()) == cases.TIE_BLOB_SIZES          # one cluster per blob: odd and even member counts
    assert all(len(set(labels[blob == b])) == 1 for b in range(len(counts)))

    def half_away(x):
        v = np.asarray(x, np.float32).astype(np.float64) * 1048576.0
        return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)

    assert half_away(np.float32(1.5 * 2.0 ** -20)) == 2 and half_away(np.float32(2.5 * 2.0 ** -20)) == 3 and half_away(np.float32(-0.5 * 2.0 ** -20)) == -1
    monkeypatch.setattr(ref, "quantise", half_away)
    other = ref.train_set(rows, L2, **args)
    assert other[2].tobytes() == labels.tobytes() and other[0].tobytes() != dic[0].tobytes()
    differ = (other[0] != dic[0]).any(axis=1)
    print(f"half away from zero changes {int((other[0] != dic[0]).sum())} elements, in the clusters of {counts[differ].tolist()} rows")
    assert (counts[differ] % 2 == 0).any() and (counts[differ] % 2 == 1).any()


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_launch_corners(kind):
    corners = cases.launch_corners(kind)
    # one assignment, no update: the labels are those of the seed centres
    sets, args = corners["one_iteration"]
    assert args["max_iters"] == 1
    for s, rows in enumerate(sets):
        dic, rec, labels, runs = ref.train_set(rows, kind, set_index=s, detail=True, **args)
        win = runs[rec["attempt"]]
        assert rec["status"] == 0 and rec["iterations"] == 1 and dic.tobytes() == rows[win["seed_rows"]].tobytes()
        assert labels.tobytes() == ref.assign(rows, rows[win["seed_rows"]], kind)[0].tobytes()
        assert rec["compactness"] == win["seed_compactness"]
    sets, args = corners["sixteen_attempts"]
    assert args["attempts"] == 16
    for s, rows in enumerate(sets):
        dic, rec, labels, runs = ref.train_set(rows, kind, set_index=s, detail=True, **args)
        comps = [r["compactness"] for r in runs]
        assert len(runs) == 16 and len(set(comps)) > 1 and rec["attempt"] == comps.index(min(comps))
    sets, args = corners["rows_equal_words"]
    assert len(sets[0]) == args["n_words"] == len(np.unique(sets[0], axis=0))
    dic, rec, labels = ref.train_set(sets[0], kind, set_index=0, **args)
    assert rec["status"] == 0 and rec["compactness"] == 0 and rec["empty_clusters"] == 0 and sorted(labels.tolist()) == list(range(9))
    sets, args = corners["rows_equal_words_with_repeats"]
    assert len(sets[0]) == args["n_words"] == 9 and len(np.unique(sets[0], axis=0)) == 6
    dic, rec, labels, runs = ref.train_set(sets[0], kind, set_index=0, detail=True, **args)
    assert rec["status"] == 0 and rec["compactness"] == 0 and rec["empty_clusters"] == 3
    trace = []
    ref.seed_centres(sets[0], kind, 9, args["seed"], 0, 0, trace=trace)
    assert [t["total"] for t in trace[-3:]] == [0, 0, 0] and trace[-4]["total"] > 0      # the last three centres: nothing left to weigh


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_workspace_guard_sets(kind):
    sets, args = cases.workspace_guard_sets(kind)
    assert [len(s) for s in sets] == [257, 5, 300] and args["n_words"] == 7
    dic, rec, labels = cases.expected("workspace_guard", kind)
    assert rec["status"].tolist() == [0, ref.GMS_ERR_BAD_ARG, 0] and (rec["iterations"][[0, 2]] >= 2).all()      # updates ran
