"""GPU: the LOGOS dictionary trainer (gms_logos_dict_train_device / gms_logos_dict_train, DESIGN.md §6b "Training the dictionary")
against the numpy statement tests/logos_dict_ref.py, byte for byte: dictionaries, records and labels. The tests named test_case_*
run the inputs of tests/logos_dict_cases.py, which tests/test_logos_dict_ref.py shows to leave the first pass of each kernel loop."""
import importlib
import os

import numpy as np
import pytest

import logos_dict_cases as cases
import logos_dict_ref as ref
from logos_dict_cases import clustered_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAMMING, L2 = ref.HAMMING, ref.L2


def _batch():
    return importlib.import_module("sfm-gms_amd.batch")


def check_against_statement(ctx, sets, kind, n_words, attempts=3, max_iters=100, seed=0):
    dic, rec, labels = _batch().logos_dictionary(ctx, sets, kind, n_words, attempts, max_iters, seed)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    flat = np.concatenate(sets) if off[-1] else np.zeros((0, 32 if kind == HAMMING else 128), np.uint8 if kind == HAMMING else np.float32)
    want_dic, want_rec, want_labels = ref.train(flat, off, kind, n_words, attempts, max_iters, seed)
    for s in range(len(sets)):
        print(f"set {s}: n={len(sets[s])} got {rec[s]} want {want_rec[s]}")
    assert rec.tobytes() == want_rec.tobytes()
    assert dic.tobytes() == want_dic.tobytes()
    assert np.concatenate(labels).tobytes() == want_labels.tobytes()
    return dic, rec, labels


@pytest.mark.parametrize("kind", [HAMMING, L2])
@pytest.mark.parametrize("n_words", [1, 50, 100])
def test_unequal_sets_in_one_call_equal_the_statement(ctx, kind, n_words):
    sizes = [1500, 100, 777, 333]
    sets = [clustered_rows(kind, n, 100 * n_words + k) for k, n in enumerate(sizes)]
    dic, rec, _ = check_against_statement(ctx, sets, kind, n_words, max_iters=40, seed=11 + n_words)
    assert (rec["status"] == 0).all() and (rec["iterations"] >= 1).all()


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_set_sizes_around_workgroup_boundaries(ctx, kind):
    # 256 rows per workgroup, 64 per wave, 4 per lane of the draw's scan; 64 words per tile of the L2 assignment
    sizes = [70, 255, 256, 257, 511, 512, 513, 64, 65, 1024, 1025]
    sets = [clustered_rows(kind, n, 7 * n) for n in sizes]
    check_against_statement(ctx, sets, kind, 64, attempts=2, max_iters=25, seed=3)
    check_against_statement(ctx, sets[:4], kind, 65, attempts=2, max_iters=25, seed=4)


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_duplicates_zero_weight_and_empty_clusters(ctx, kind):
    base = clustered_rows(kind, 3, 5)
    sets = [np.concatenate([base] * 30), np.concatenate([base[:1]] * 300), clustered_rows(kind, 400, 6)]
    dic, rec, _ = check_against_statement(ctx, sets, kind, 5, attempts=3, max_iters=20, seed=8)
    assert rec["empty_clusters"].tolist()[:2] == [2, 4] and rec["compactness"].tolist()[:2] == [0, 0]


def test_a_failing_set_leaves_the_others_alone(ctx):
    ok = [clustered_rows(L2, n, n) for n in (300, 290, 280)]
    alone = [ref.train_set(r, L2, 8, 2, 30, seed=21, set_index=s) for s, r in zip((0, 2, 4), ok)]
    bad_value, too_few = ok[1].copy(), clustered_rows(L2, 5, 1)
    bad_value[17, 5] = np.nan
    sets = [ok[0], bad_value, ok[1], too_few, ok[2]]
    dic, rec, labels = check_against_statement(ctx, sets, L2, 8, attempts=2, max_iters=30, seed=21)
    assert rec["status"].tolist() == [0, ref.GMS_ERR_DOMAIN, 0, ref.GMS_ERR_BAD_ARG, 0]
    assert not dic[1].any() and not dic[3].any() and (labels[1] == -1).all() and (labels[3] == -1).all()
    for s, want in zip((0, 2, 4), alone):
        assert dic[s].tobytes() == want[0].tobytes() and rec[s].tobytes() == want[1].tobytes()
    for bad in (np.inf, -np.inf, 4097.0, -1e30):
        x = ok[0].copy()
        x[-1, -1] = bad
        _, r, _ = _batch().logos_dictionary(ctx, [x], L2, 8, 1, 5)
        assert r["status"].tolist() == [ref.GMS_ERR_DOMAIN]
    hamming = [clustered_rows(HAMMING, 40, 2), clustered_rows(HAMMING, 7, 3)]
    _, r, _ = check_against_statement(ctx, hamming, HAMMING, 8, attempts=1, max_iters=10)
    assert r["status"].tolist() == [0, ref.GMS_ERR_BAD_ARG]


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_oneshot_equals_batched_and_repeats_itself(ctx, pkg, kind):
    rows = clustered_rows(kind, 900, 77)
    dic, rec, labels = pkg.trainLogosDictionary(rows, kind, n_words=50, max_iters=30, seed=5, detail=True)
    bdic, brec, blabels = _batch().logos_dictionary(ctx, [rows], kind, 50, 3, 30, 5)
    assert dic.tobytes() == bdic[0].tobytes() and rec.tobytes() == brec[0].tobytes() and labels.tobytes() == blabels[0].tobytes()
    again = pkg.trainLogosDictionary(rows, kind, n_words=50, max_iters=30, seed=5)
    assert again.tobytes() == dic.tobytes()
    other = pkg.trainLogosDictionary(rows, kind, n_words=50, max_iters=30, seed=6)
    assert other.tobytes() != dic.tobytes()
    # the labels are the words call's
    words = _batch().logos_words(ctx, rows, dic, kind)
    assert np.array_equal(words, labels)
    with pytest.raises(pkg.GmsError):
        pkg.trainLogosDictionary(rows[:10], kind, n_words=50)


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_graph_replay_on_new_rows_equals_the_direct_call(ctx, kind):
    import torch
    batch = _batch()
    first = [clustered_rows(kind, n, 40 + n) for n in (500, 300, 260)]
    fresh = [clustered_rows(kind, n, 90 + n) for n in (280, 520, 200)]      # other rows, other set sizes, fewer rows in all
    job = batch.LogosDictionary(ctx, kind, 3, 1060, n_words=20, attempts=2, max_iters=15, seed=2)
    job.load(first)
    dev = job.device
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    ctx.set_stream(s.cuda_stream)
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):
            job.run()
        job.load(fresh)
        job.d_dict.zero_()
        job.d_results.zero_()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        rep = job.results()
    finally:
        ctx.set_stream(None)
        g.reset()
        del g
    dic, rec, labels = batch.logos_dictionary(ctx, fresh, kind, 20, 2, 15, 2)
    assert rep[0].tobytes() == dic.tobytes() and rep[1].tobytes() == rec.tobytes()
    assert rep[2][:1000].tobytes() == np.concatenate(labels).tobytes()
    want = ref.train(np.concatenate(fresh), [0, 280, 800, 1000], kind, 20, 2, 15, 2)
    assert dic.tobytes() == want[0].tobytes() and rec.tobytes() == want[1].tobytes()
    assert (rec["status"] == 0).all()


def test_end_to_end_from_pixels(ctx, pkg):
    """The 1080p fixture -> detect -> 50 words trained on the left frame -> words -> matchLOGOS: the survivors are those obtained
    with the statement's dictionary."""
    batch = _batch()
    z = np.load(os.path.join(ROOT, "tests", "golden", "image_main_scenario_1080p.npz"))
    kps, rows = batch.detect_images(ctx, np.stack([z["left"], z["right"]]))
    dic = pkg.trainLogosDictionary(rows[0], pkg.GMS_DESC_HAMMING256, n_words=50, seed=1)
    want_dic, want_rec, _ = ref.train_set(rows[0], HAMMING, 50, 3, 100, seed=1)
    print(f"{len(rows[0])} rows; statement record {want_rec}")
    assert want_rec["status"] == 0 and dic.tobytes() == want_dic.tobytes()
    survivors = []
    for d in (dic, want_dic):
        w1, w2 = batch.logos_words(ctx, [rows[0], rows[1]], d, pkg.GMS_DESC_HAMMING256)
        survivors.append(pkg.matchLOGOS(kps[0], kps[1], w1, w2))
    print(f"{len(survivors[0])} survivors")
    assert survivors[0].tobytes() == survivors[1].tobytes() and len(survivors[0]) > 0


def test_run_dataset_trains_the_dictionary_it_is_not_given(ctx, pkg):
    io = importlib.import_module("sfm-gms_amd.io")
    pipeline = importlib.import_module("sfm-gms_amd.pipeline")
    rng = np.random.default_rng(4)
    frames, descs = [], []
    for f in range(3):
        n = 600 + 50 * f
        kp = np.zeros(n, pkg.KEYPOINT_DTYPE)
        kp["x"], kp["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
        kp["size"], kp["angle"] = rng.uniform(2, 8, n), rng.uniform(0, 360, n)
        frames.append(kp)
        descs.append(clustered_rows(L2, n, 300 + f))
    pairs = np.zeros(2, pkg.PAIR_DTYPE)
    pairs["frame_a"], pairs["frame_b"] = [0, 1], [1, 2]
    ds = io.Dataset(frames, [(640, 480)] * 3, descs, pkg.GMS_DESC_L2_F32X128, pairs=pairs, matches=np.zeros(0, pkg.DMATCH_DTYPE))
    with pytest.raises(ValueError, match="descriptors and a dictionary"):
        pipeline.run_dataset(ctx, ds, method="logos")
    for opts, train_rows in (({"n_words": 30, "max_iters": 20, "seed": 9}, descs[0]),
                             ({"n_words": 30, "max_iters": 20, "seed": 9, "rows": "all"}, np.concatenate(descs))):
        r = pipeline.run_dataset(ctx, ds, method="logos", train_dictionary=opts)
        dic = pkg.trainLogosDictionary(train_rows, pkg.GMS_DESC_L2_F32X128, n_words=30, max_iters=20, seed=9)
        assert r["dictionary"].tobytes() == dic.tobytes() and r["dictionary_result"]["status"] == 0
        e = pipeline.run_dataset(ctx, ds, method="logos", dictionary=dic)
        for key in ("out", "results", "logos_results", "words", "pairs"):
            assert np.asarray(r[key]).tobytes() == np.asarray(e[key]).tobytes(), key


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_unusable_offsets_fail_their_set_alone(ctx, kind):
    """Offsets live on the device: decreasing, negative and out-of-range ones give their sets GMS_ERR_BAD_ARG; a set that would overlap
    an earlier one is refused, and the sets that remain equal the statement."""
    import torch
    batch = _batch()
    rows = clustered_rows(kind, 1200, 55)
    cases = [[0, 500, 0, 500, 1200],            # set 1 ends before it starts; set 2 would run over set 0's rows again
             [0, 300, 200, 900, 1200],          # set 1 ends below its start; set 2 starts inside set 0
             [-5, 400, 1300, 1100, 1200],       # a negative start; an end past the rows; an end before its start; a good set
             [100, 400, 400, 2000, 700]]        # an empty set (too few rows); an end out of range; an end before its start
    for off in cases:
        off = np.asarray(off, np.int64)
        job = batch.LogosDictionary(ctx, kind, len(off) - 1, len(rows), n_words=8, attempts=2, max_iters=12, seed=6)
        job.load([rows] + [rows[:0]] * (len(off) - 2))
        job.d_set_off.copy_(torch.from_numpy(off))
        torch.cuda.synchronize(job.device)
        job.run()
        ctx.synchronize()
        dic, rec, labels = job.results()
        want_dic, want_rec, want_labels = ref.train(rows, off, kind, 8, 2, 12, 6)
        print(off.tolist(), rec["status"].tolist(), want_rec["status"].tolist())
        assert rec.tobytes() == want_rec.tobytes() and dic.tobytes() == want_dic.tobytes() and labels.tobytes() == want_labels.tobytes()
    assert want_rec["status"].tolist() == [0, ref.GMS_ERR_BAD_ARG, ref.GMS_ERR_BAD_ARG, ref.GMS_ERR_BAD_ARG]
    first = ref.train(rows, [0, 500, 0, 500, 1200], kind, 8, 2, 12, 6)[1]["status"].tolist()
    assert first == [0, ref.GMS_ERR_BAD_ARG, ref.GMS_ERR_BAD_ARG, 0]


# ---- tests/logos_dict_cases.py: past one scan pass, one tile, 256 sets ----------------------------------------------------------------
def check_case(ctx, name, kind, *key):
    """The GPU on a case's inputs against the statement's answer (computed once per session) -> (dictionaries, records, labels)."""
    sets, args = cases.inputs(name, kind, *key)
    dic, rec, labels = _batch().logos_dictionary(ctx, sets, kind, **args)
    labels = np.concatenate(labels)
    want_dic, want_rec, want_labels = cases.expected(name, kind, *key)
    for s in np.flatnonzero((rec != want_rec) | (dic != want_dic).any(axis=(1, 2)))[:10]:
        print(f"set {s}: n={len(sets[s])} got {rec[s]} want {want_rec[s]}")
    print(f"{len(sets)} sets, {len(labels)} rows: {int((labels != want_labels).sum())} labels differ; first records {rec[:4]}")
    assert rec.tobytes() == want_rec.tobytes()
    assert dic.tobytes() == want_dic.tobytes()
    assert labels.tobytes() == want_labels.tobytes()
    return dic, rec, labels


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_long_sets_scan_several_chunks_per_thread(ctx, kind):
    """Sets of 256, 257 and 514 chunks behind a short one: seed_pick_kernel's scan with one, two and three chunks per thread, its
    bisection over hundreds of entries, update_kernel over hundreds of passes."""
    dic, rec, _ = check_case(ctx, "long_sets", kind)
    assert (rec["status"] == 0).all() and (rec["iterations"] >= 2).all()


def test_case_max_rows_set_and_one_row_more(ctx):
    """Hamming: 2^20 rows (4096 chunks, 16 per thread of the scan) train; 2^20 + 1 rows are refused."""
    dic, rec, labels = check_case(ctx, "max_rows", HAMMING)
    assert rec["status"].tolist() == [0, ref.GMS_ERR_BAD_ARG] and rec["iterations"][0] == 2
    assert dic[0].any() and not dic[1].any() and (labels[:1 << 20] >= 0).all() and (labels[1 << 20:] == -1).all()


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_zero_weight_runs_make_the_prefix_flat(ctx, kind):
    """Five distinct rows in long runs, six words: chunks without weight in front, behind and in runs of over a hundred; three
    candidates with equal potentials; the last centre drawn with no weight left."""
    dic, rec, _ = check_case(ctx, "zero_weight_runs", kind)
    assert rec["status"].tolist() == [0] and rec["compactness"].tolist() == [0] and rec["empty_clusters"].tolist() == [1]


@pytest.mark.parametrize("kind,n_words", [(HAMMING, 512), (HAMMING, 513), (HAMMING, 1030), (L2, 129)])
def test_case_many_words_fill_more_than_one_tile(ctx, kind, n_words):
    """One full tile, one word more, three tiles: labels of the later tiles, and rows equally near to words of two tiles."""
    dic, rec, labels = check_case(ctx, "many_words", kind, n_words)
    assert rec["status"].tolist() == [0] and labels.max() >= min(n_words - 1, 1024)


@pytest.mark.parametrize("kind", [HAMMING, L2])
def test_case_many_sets_more_than_one_pass_of_the_plan(ctx, kind):
    """300 sets: plan_kernel's strided loop past its first pass, locate() over 301 entries, failed sets at both ends and at 255 / 256."""
    sets, args = cases.many_sets(kind)
    dic, rec, labels = check_case(ctx, "many_sets", kind)
    assert rec["status"].tolist() == cases.many_sets_statuses(kind).tolist()
    off = cases.flat(sets, kind)[1]
    for s in np.flatnonzero(rec["status"] != 0):
        assert not dic[s].any() and (labels[off[s]:off[s + 1]] == -1).all()
    set_of_row = np.repeat(np.arange(len(sets)), np.diff(off))
    assert (labels[rec["status"][set_of_row] == 0] >= 0).all()


def test_case_l2_domain_edge_has_the_largest_sums(ctx):
    """Rows at the corners of [-4096, 4096]^128: weights near 2^41, a compactness above 2^47, sums of q near 2^32 per row."""
    dic, rec, _ = check_case(ctx, "l2_domain_edge", L2)
    assert rec["status"].tolist() == [0] and int(rec["compactness"][0]) > 2 ** 47
    for x in cases.just_outside_the_domain():
        d, r, lab = _batch().logos_dictionary(ctx, [x], L2, 8, 1, 2)
        assert r["status"].tolist() == [ref.GMS_ERR_DOMAIN] and not d.any() and (lab[0] == -1).all()


def test_case_l2_rounding_ties_are_rounded_to_even(ctx):
    """Elements of the form (k + 0.5) 2^-20: the statement's bytes come out only with ties to even (the CPU test shows that rounding
    half away from zero gives other bytes on this input)."""
    dic, rec, _ = check_case(ctx, "l2_rounding_ties", L2)
    assert rec["status"].tolist() == [0] and rec["iterations"][0] >= 2


@pytest.mark.parametrize("kind", [HAMMING, L2])
@pytest.mark.parametrize("corner", ["one_iteration", "sixteen_attempts", "rows_equal_words", "rows_equal_words_with_repeats"])
def test_case_launch_corners(ctx, kind, corner):
    dic, rec, _ = check_case(ctx, "launch_corners", kind, corner)
    assert (rec["status"] == 0).all()
    if corner == "one_iteration":
        assert (rec["iterations"] == 1).all()
