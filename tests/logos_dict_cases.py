"""Inputs of the LOGOS dictionary trainer's tests that reach past the first pass of each kernel loop (DESIGN.md §6b "Training the
dictionary"): sets longer than 256 chunks, runs of chunks without weight, more centres than one tile, more than 256 sets, the edge
of the L2 domain, rounding ties, and the corners of the launch sequence. A builder returns (sets, args): the training sets of one call
and n_words / attempts / max_iters / seed. tests/test_logos_dict_ref.py asserts, from the statement's own trace, that every case
reaches the regime it is named for; tests/test_gpu_logos_dict.py holds the GPU to the statement's bytes on the same inputs.

Where a condition depends on the draws, the seeds below were found by a search on the CPU and are literals: nothing is filtered or
skipped when the tests run."""
import functools

import numpy as np

import logos_dict_ref as ref

HAMMING, L2 = ref.HAMMING, ref.L2
CHUNK = 256                     # rows per workgroup of the row-parallel kernels (logos_dict_core.h: kChunk)
HAMMING_TILE, L2_TILE = 512, 64  # centres per LDS tile of the two assignment kernels


def clustered_rows(kind, n, seed, n_centres=12):
    """Rows around a few centres (so that k-means has something to find), with repeats among them."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, n_centres, n)
    if kind == L2:
        centres = rng.uniform(0.0, 200.0, (n_centres, 128)).astype(np.float32)
        rows = np.rint(centres[which] + rng.normal(0.0, 12.0, (n, 128))).astype(np.float32)    # SIFT-like: small integers
        rows[n // 2:] += rng.uniform(-0.5, 0.5, (n - n // 2, 128)).astype(np.float32)          # and rows that are not
        return np.clip(rows, -4096.0, 4096.0).astype(np.float32)
    centres = rng.integers(0, 256, (n_centres, 32), dtype=np.uint8)
    flips = (rng.random((n, 256)) < 0.12)
    return centres[which] ^ np.packbits(flips, axis=1)


def n_chunks(n):
    return (n + CHUNK - 1) // CHUNK


def last_chunk(n):
    """The first row of a set's last chunk."""
    return (n_chunks(n) - 1) * CHUNK


def flat(sets, kind):
    """(rows of all sets, offsets): the arguments of ref.train."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return np.concatenate(sets), off


# ---- 1. sets longer than 256 chunks -----------------------------------------------------------------------------------------------
LONG_SIZES = [300, 65536, 65537, 131329]     # 2, 256, 257 (the last of one row) and 514 chunks (the last of one row; per = 3)
LONG_ARGS = {HAMMING: dict(n_words=4, attempts=2, max_iters=3, seed=1), L2: dict(n_words=4, attempts=2, max_iters=3, seed=1)}
LONG_DATA_SEEDS = {HAMMING: [0, 0, 0, 0], L2: [0, 0, 0, 0]}     # per set, found by the search (tests/test_logos_dict_ref.py states what for)
LONG_HAMMING_FLIPS = 2e-5     # per bit


def hamming_clusters(n, seed, n_centres, flip_rate, outlier_from=None):
    """Rows that are copies of n_centres random centres with `flip_rate` of all bits flipped (drawn as positions: no [n, 256] array of
    draws for a million rows); rows from outlier_from on are the complement of centre 0. With few flips nearly every row repeats its
    centre, so that once the centres are covered one far row carries a share of the weight that a draw can hit."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (n_centres, 32), dtype=np.uint8)
    rows = centres[rng.integers(0, n_centres, n)]
    pos = rng.integers(0, n * 256, int(round(n * 256 * flip_rate)))
    np.bitwise_xor.at(rows.reshape(-1), pos >> 3, (1 << (pos & 7)).astype(np.uint8))
    if outlier_from is not None:
        rows[outlier_from:] = ~centres[0]
    return rows


def long_set(kind, n, seed):
    """A long set of three clusters whose last chunk holds outliers: the corner (4096, ..., 4096) for L2, the complement of a centre
    for Hamming. Four words for three clusters and one far point: when the clusters are covered the outliers carry a large share of
    the weight that is left, so a draw lands in the last chunk."""
    if kind == L2:
        rows = clustered_rows(L2, n, seed, n_centres=3)
        rows[last_chunk(n):] = 4096.0
        return rows
    return hamming_clusters(n, seed, 3, LONG_HAMMING_FLIPS, outlier_from=last_chunk(n))


def long_sets(kind):
    sets = [clustered_rows(kind, LONG_SIZES[0], LONG_DATA_SEEDS[kind][0])]
    sets += [long_set(kind, n, s) for n, s in zip(LONG_SIZES[1:], LONG_DATA_SEEDS[kind][1:])]
    return sets, dict(LONG_ARGS[kind])


MAX_SET_ROWS = ref.MAX_SET_ROWS
MAX_ROWS_ARGS = dict(n_words=3, attempts=1, max_iters=2, seed=1)
MAX_ROWS_DATA_SEED = 0
MAX_ROWS_FLIPS = 2.6e-4


def max_rows_sets():
    """Hamming: a set of exactly 2^20 rows (4096 chunks, per = 16; two clusters, the last chunk their outliers), then one of 2^20 + 1
    rows, which is refused."""
    first = hamming_clusters(MAX_SET_ROWS, MAX_ROWS_DATA_SEED, 2, MAX_ROWS_FLIPS, outlier_from=last_chunk(MAX_SET_ROWS))
    second = hamming_clusters(MAX_SET_ROWS + 1, MAX_ROWS_DATA_SEED + 1, 2, MAX_ROWS_FLIPS)
    return [first, second], dict(MAX_ROWS_ARGS)


# ---- 2. runs of chunks with zero weight -------------------------------------------------------------------------------------------
RUNS = [700, 30000, 513, 35000, 300]


def zero_weight_runs(kind):
    """One set of five distinct rows in runs, then 1000 more of the first: 67 513 rows, 264 chunks, six words for five distinct rows.
    A centre takes the weight of its whole run away, so the prefix the bisection walks has runs of equal entries; when one distinct row
    is left all three candidates are that row, and the last centre is drawn with no weight left at all."""
    rng = np.random.default_rng(12)
    base = (rng.uniform(-100.0, 300.0, (5, 128)).astype(np.float32) if kind == L2 else rng.integers(0, 256, (5, 32), dtype=np.uint8))
    which = np.concatenate([np.full(n, k) for k, n in enumerate(RUNS)] + [np.zeros(1000, np.int64)])
    return [base[which]], dict(n_words=6, attempts=2, max_iters=3, seed=5)


# ---- 3. more than one tile of centres ---------------------------------------------------------------------------------------------
TILE_SEEDS = {(HAMMING, 512): 0, (HAMMING, 513): 23, (HAMMING, 1030): 1, (L2, 129): 6}   # of the rows and of the call


def many_words(kind, n_words):
    """Rows that lie equally far from centres in two tiles at the final assignment, where the lowest index must win.

    Hamming: 1100 rows, each one of 1200 planted centres with 3 bits flipped, the planted centres one base row with 8 bits flipped.
    All rows lie within a few bits of each other, so distances are small integers, bit majorities keep them so, and ties are common.

    L2: a moved centre is a mean, and a row is hardly ever exactly as far from a mean as from another centre. So the 400 rows are built
    for it: 66 groups far apart, each of three integer points P, Q = P + 2 e_a and Y = P + e_b, two rows per point (and four more
    rows). 129 words leave most groups with two. Where those are P and then Y, Q joins P, the centre moves to the midpoint P + e_a,
    and P is at squared distance 1 from both it and Y: nothing changes, the assignment after it is the final one, and P's two rows
    are tied between a word of the first tile and a later one. All of this arithmetic is exact in fp32."""
    seed = TILE_SEEDS[(kind, n_words)]
    rng = np.random.default_rng(1000 + seed)

    def flip(rows, bits):
        pos = rng.integers(0, 256, (len(rows), bits))
        for f in range(bits):
            rows[np.arange(len(rows)), pos[:, f] >> 3] ^= (1 << (pos[:, f] & 7)).astype(np.uint8)
        return rows

    if kind == HAMMING:
        planted = flip(np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), 1200, axis=0), 8)
        rows = flip(planted[rng.integers(0, len(planted), 1100)], 3)
    else:
        groups = 66
        p = rng.integers(0, 40, (groups, 128)).astype(np.float32)
        axes = np.array([rng.choice(128, 2, replace=False) for _ in range(groups)])
        q, y = p.copy(), p.copy()
        q[np.arange(groups), axes[:, 0]] += 2.0
        y[np.arange(groups), axes[:, 1]] += 1.0
        rows = np.concatenate([p, p, q, q, y, y, y[:4]])
        rows = rows[rng.permutation(len(rows))]
        assert len(rows) == 400
    return [rows], dict(n_words=n_words, attempts=1, max_iters=3, seed=seed)


def tiles_at_minimum(rows, dictionary, kind):
    """Per row: the number of tiles of the assignment kernel that hold a word at the row's minimum distance."""
    d = ref.distances(rows, dictionary, kind)
    tile = np.arange(d.shape[1]) // (HAMMING_TILE if kind == HAMMING else L2_TILE)
    at_min = d == d.min(axis=1, keepdims=True)
    return np.array([len(np.unique(tile[m])) for m in at_min])


# ---- 4. more than 256 sets --------------------------------------------------------------------------------------------------------
MANY_SETS, TOO_FEW, NAN_SET = 300, (0, 255, 256, 299), 257


def many_sets(kind):
    """300 sets of 6 to 14 rows; those at 0, 255, 256 and 299 have 3 rows for 4 words, and for L2 set 257 holds a NaN."""
    rng = np.random.default_rng(31)
    sizes = rng.integers(6, 15, MANY_SETS)
    sizes[list(TOO_FEW)] = 3
    sets = [clustered_rows(kind, int(n), 5000 + s, n_centres=3) for s, n in enumerate(sizes)]
    if kind == L2:
        sets[NAN_SET][2, 77] = np.nan
    return sets, dict(n_words=4, attempts=2, max_iters=5, seed=17)


def many_sets_statuses(kind):
    want = np.zeros(MANY_SETS, np.int32)
    want[list(TOO_FEW)] = ref.GMS_ERR_BAD_ARG
    if kind == L2:
        want[NAN_SET] = ref.GMS_ERR_DOMAIN
    return want


# ---- 5. the edge of the L2 domain and rounding ties -------------------------------------------------------------------------------
def l2_domain_edge():
    """600 rows at the corners of [-4096, 4096]^128, every seventh uniform within it: the largest distances and sums the domain has."""
    rng = np.random.default_rng(41)
    rows = rng.choice(np.array([-4096.0, 4096.0], np.float32), (600, 128))
    rows[::7] = rng.uniform(-4096.0, 4096.0, (len(rows[::7]), 128)).astype(np.float32)
    rows[1, 0], rows[2, 0] = 4096.0, -4096.0
    return [rows], dict(n_words=8, attempts=2, max_iters=6, seed=3)


def just_outside_the_domain():
    """The edge case's rows with one element a float past +4096, and with one past -4096."""
    rows = l2_domain_edge()[0][0]
    out = []
    for row, col, v in ((599, 127, np.nextafter(np.float32(4096.0), np.float32(np.inf))),
                        (300, 5, np.nextafter(np.float32(-4096.0), np.float32(-np.inf)))):
        x = rows.copy()
        x[row, col] = v
        out.append(x)
    return out


TIE_BLOB_SIZES = [5, 6, 7, 8, 9, 10]


def l2_rounding_ties():
    """Six blobs of 5 .. 10 rows (odd and even counts) around integer centres within [-6, 6]. The first rows of a blob (all but two)
    are its centre plus an odd multiple of 2^-21 per element, of either sign, so that x * 2^20 is k + 0.5 exactly and rint's ties to
    even differ from rounding half away from zero; |x| < 8 keeps such a value a float. The other two rows are ordinary."""
    rng = np.random.default_rng(51)
    rows, blob = [], []
    for b, n in enumerate(TIE_BLOB_SIZES):
        centre = rng.integers(-6, 7, 128).astype(np.float64)
        odd = 2 * rng.integers(-2 ** 18, 2 ** 18, (n - 2, 128)) + 1      # |odd 2^-21| < 0.25
        rows.append((centre + odd * 2.0 ** -21).astype(np.float32))
        rows.append((centre + rng.uniform(-0.25, 0.25, (2, 128))).astype(np.float32))
        blob += [b] * n
    rows = np.concatenate(rows)
    order = rng.permutation(len(rows))
    return [rows[order]], dict(n_words=len(TIE_BLOB_SIZES), attempts=2, max_iters=6, seed=7), np.asarray(blob)[order]


# ---- 6. launch corners ------------------------------------------------------------------------------------------------------------
def launch_corners(kind):
    """name -> (sets, args): one assignment and no update; the most attempts; as many rows as words, all distinct; and with repeats."""
    distinct = clustered_rows(kind, 9, 61)
    assert len(np.unique(distinct, axis=0)) == 9
    repeats = distinct.copy()
    repeats[[3, 4, 8]] = repeats[[0, 0, 5]]
    return {"one_iteration": ([clustered_rows(kind, 700, 62), clustered_rows(kind, 90, 63)], dict(n_words=7, attempts=3, max_iters=1, seed=2)),
            "sixteen_attempts": ([clustered_rows(kind, 300, 64), clustered_rows(kind, 40, 65)], dict(n_words=6, attempts=16, max_iters=8, seed=3)),
            "rows_equal_words": ([distinct, clustered_rows(kind, 30, 66)], dict(n_words=9, attempts=2, max_iters=6, seed=4)),
            "rows_equal_words_with_repeats": ([repeats, clustered_rows(kind, 30, 67)], dict(n_words=9, attempts=2, max_iters=6, seed=4))}


# ---- 7. exact and dirty workspace -------------------------------------------------------------------------------------------------
def workspace_guard_sets(kind):
    """257, 5 and 300 rows for 7 words: two chunks with a last chunk of one row, a set that is refused, and another two chunks."""
    return [clustered_rows(kind, n, 70 + n) for n in (257, 5, 300)], dict(n_words=7, attempts=2, max_iters=8, seed=9)


# ---- the statement's answer, computed once per session ----------------------------------------------------------------------------
BUILDERS = {"long_sets": long_sets, "zero_weight_runs": zero_weight_runs, "many_sets": many_sets, "workspace_guard": workspace_guard_sets}


@functools.lru_cache(maxsize=None)
def expected(name, kind, *key):
    """ref.train on the case's inputs -> (dictionaries, records, labels). name: a key of BUILDERS, "many_words" (key: n_words),
    "launch_corners" (key: the corner's name), "max_rows", "l2_domain_edge" or "l2_rounding_ties"."""
    sets, args = inputs(name, kind, *key)
    rows, off = flat(sets, kind)
    return ref.train(rows, off, kind, **args)


def inputs(name, kind, *key):
    if name in BUILDERS:
        return BUILDERS[name](kind)
    if name == "many_words":
        return many_words(kind, *key)
    if name == "launch_corners":
        return launch_corners(kind)[key[0]]
    if name == "max_rows":
        return max_rows_sets()
    if name == "l2_domain_edge":
        return l2_domain_edge()
    if name == "l2_rounding_ties":
        return l2_rounding_ties()[:2]
    raise KeyError(name)
