"""-m gpu: the end of a pair in the byte-matrix kernel's default-flags body (dense_pair_plain) against
oracle/gms_ref.c, byte for byte: results record, survivors and mask. The body leaves the last grid type's increments in the matrix
(no fourth undo) and its verifying lanes store their verdicts straight into the mark table, over those bytes; the copy-out's count
table lies over them as well. The cases are the places where that can be wrong while tests/test_gpu_mark_table.py still passes:
  1. pairs whose grid-type-4 increments sit exactly under the mark table and under the count table, large counts, every
     matches-per-thread class with a wave tail and a dealt-unit tail, in query order and shuffled;
  2. cells cut by the image's border (column 0, row 0, the corner: two, two and one half cell) that stand under exactly one shifted
     grid type, clusters in the half cells nobody owns under a shifted grid type (hx = 39, hy = 39) whose motion would pass if that
     type's verdict were attributed to them, and matches whose left point is binned nowhere (the sink's entry);
  3. more than two workgroups per CU in one launch, the first 256 dense in the regions of case 1, the later ones sparse, with
     results that an inherited field or count would change;
  4. a restart in crowded mode that comes from the LAST grid type, a plain pair, and a hand-over to the general path, one launch.
What each constructed pair does -- which grid type carries a cluster, which cells exceed 255 -- is asserted from the oracle's own
stages (assignMatchPairs, verifyCellPairs per grid type) and numpy counts, never from the GPU's result.
The whole file runs again in child processes with GMS_IDENT=1 (the identity-query body for the pairs in query order) and GMS_DEAL=1
(the dealt instantiations).
(Case 1 at 10 240 matches and above: the 54 cells whose rows lie under the two tables hold at most 54 x 255 matches in the plain
mode, and coherent motion puts a cell's matches into one entry, so 7000 matches are confined to them and the rest are spread over
the image.)"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

W, H = 2000, 1000  # 100 x 50 pixels per left cell
Q_LAST_IDENT, Q_MISSES = 9, 10
FORCED_IDENT = os.environ.get("GMS_IDENT") == "1"
# gms_kernel_dense.h: a matrix row is 404 bytes; the mark table is 1621 entries of 8 bytes from byte 32768, the count table the first 8 KB
ROW_BYTES, TABLE_OFF, TABLE_BYTES, COUNT_BYTES = 404, 32768, 8 * 1621, 8192
ROWS_UNDER_TABLES = set(range(0, (COUNT_BYTES - 1) // ROW_BYTES + 1)) | set(range(TABLE_OFF // ROW_BYTES, (TABLE_OFF + TABLE_BYTES - 1) // ROW_BYTES + 1))


@pytest.fixture(scope="module")
def batch():
    return importlib.import_module("sfm-gms_amd.batch")


@pytest.fixture(scope="module")
def types():
    return importlib.import_module("sfm-gms_amd.types")


def _px(cells):
    """points in units of left cells -> pixels"""
    return np.asarray(cells, dtype=np.float64) * [W / 20.0, H / 20.0]


def _pair(xy1, xy2):
    """Match k = (query k, train k): a pair in query order with one match per keypoint of frame A."""
    idx = np.arange(len(xy1))
    return cases._pair(np.asarray(xy1, dtype=np.float32), np.asarray(xy2, dtype=np.float32), idx, idx, (W, H), (W, H))


def _shuffled(c, seed):
    return dict(c, matches=c["matches"][np.random.default_rng(seed).permutation(len(c["matches"]))])


def _oracle(oracle, c):
    rc, want, wmask, wres = oracle.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], False, False, 6.0)
    assert rc == 0
    return want, np.asarray(wmask, dtype=np.uint8), wres


def _per_type(oracle, c):
    """The oracle's stages one grid type at a time -> (left cell of every match [4, m] (-1: not binned), nLeft [4, 400],
    the match is an inlier under the grid type [4, m])."""
    p1 = np.stack([c["kp1"]["x"] / np.float32(W), c["kp1"]["y"] / np.float32(H)], axis=1).astype(np.float32)
    p2 = np.stack([c["kp2"]["x"] / np.float32(W), c["kp2"]["y"] / np.float32(H)], axis=1).astype(np.float32)
    mt = np.stack([c["matches"]["queryIdx"], c["matches"]["trainIdx"]], axis=1).astype(np.int32)
    rc, pairs, nleft, motion = oracle.assign_pairs(p1, p2, mt, 20, 20)
    assert rc == 0
    inl = []
    for t in range(4):
        cp = oracle.verify_cells(motion[t], nleft[t], 20, 20, 1)
        left, right = pairs[t, :, 0], pairs[t, :, 1]
        inl.append((left >= 0) & (cp[np.maximum(left, 0)] == right))
    return pairs[:, :, 0], nleft, np.array(inl)


def _launch(ctx, batch, types, cs, frames=None, frame_pairs=None, in_query_order=False):
    """One launch of the cases (pair i = frames (i, len(cs) + i) unless told otherwise) -> (pairs, matches, out, results, mask).
    in_query_order: every pair is an identity-query pair; with GMS_IDENT=1 all of them must stay on the identity body."""
    if frames is None:
        frames = batch.FrameTable(ctx, [c["kp1"] for c in cs] + [c["kp2"] for c in cs], [c["size1"] for c in cs] + [c["size2"] for c in cs])
    pairs = np.zeros(len(cs), dtype=types.PAIR_DTYPE)
    off = 0
    for i, c in enumerate(cs):
        a, b = (i, len(cs) + i) if frame_pairs is None else frame_pairs[i]
        pairs[i]["frame_a"], pairs[i]["frame_b"], pairs[i]["m"], pairs[i]["match_off"] = a, b, len(c["matches"]), off
        off += len(c["matches"])
    matches = np.concatenate([c["matches"] for c in cs])
    ctx.synchronize()
    before = ctx.query(Q_MISSES)
    out, results, mask = batch.filter_pairs(ctx, frames, pairs, matches, False, False, 6.0)
    if FORCED_IDENT:
        assert ctx.query(Q_LAST_IDENT) == 1
        if in_query_order:
            assert ctx.query(Q_MISSES) == before  # every pair stayed on the identity body
    return pairs, matches, out, results, mask


def _assert_pair(pairs, matches, out, results, mask, i, want, wmask, wres):
    o, m, k = int(pairs[i]["match_off"]), int(pairs[i]["m"]), int(results[i]["n_inliers"])
    assert results[i]["status"] == 0
    assert (k, int(results[i]["best_scale"]), int(results[i]["best_rot"])) == (wres["n_inliers"], wres["best_scale"], wres["best_rot"]), i
    assert out[o:o + k].tobytes() == want.tobytes(), i
    assert np.array_equal(mask[o:o + m], wmask), i


# ---- 1. the last grid type's increments under the mark table and the count table ---------------------------------------------------
# Under grid type 4 (shifted by half a cell both ways) cell (cx, cy) takes the points of [cx - 0.5, cx + 0.5) x [cy - 0.5, cy + 0.5):
# the three boxes below are cells 1..19 of row 4, 0..13 of row 5 (matrix rows 81..113) and row 0 (matrix rows 0..19).
REGION = [(0.51, 19.49, 3.51, 4.49), (0.01, 13.49, 4.51, 5.49), (0.01, 19.49, 0.01, 0.49)]  # x0, x1, y0, y1 in cells
MOTION = np.array([0.25, 9.0])  # cells; the region moves as one piece and stays inside the right grid
N_CONFINED = 7000  # about 170 per cell: below 255 under every grid type


def _region_points(rng, n):
    area = np.array([(x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in REGION])
    box = rng.choice(len(REGION), size=n, p=area / area.sum())
    lo = np.array([(x0, y0) for x0, x1, y0, y1 in REGION])[box]
    hi = np.array([(x1, y1) for x0, x1, y0, y1 in REGION])[box]
    return lo + rng.uniform(0, 1, (n, 2)) * (hi - lo)


def _region_case(seed, m, n_confined=N_CONFINED):
    """m matches in query order -> (case, number of matches confined to the region): coherent motion plus one match in four anywhere"""
    rng = np.random.default_rng(seed)
    k = min(m, n_confined)
    left = np.concatenate([_region_points(rng, k), np.stack([rng.uniform(0.01, 19.7, m - k), rng.uniform(0.01, 10.9, m - k)], axis=1)])
    right = left + MOTION + rng.uniform(-0.02, 0.02, left.shape)
    noise = rng.uniform(0, 1, m) < 0.25
    right[noise] = np.stack([rng.uniform(0.01, 19.99, noise.sum()), rng.uniform(0.01, 19.99, noise.sum())], axis=1)
    return _pair(_px(left), _px(right)), k


TAIL_SIZES = [512, 4096 + 63, 10240, 10241, 16384]


@pytest.fixture(scope="module")
def region_cases(oracle):
    """[(case, expected)] for TAIL_SIZES, built and checked once, never modified"""
    made = []
    for m in TAIL_SIZES:
        c, k = _region_case(6100 + m, m)
        left, nleft, inl = _per_type(oracle, c)
        assert set(left[3, :k].tolist()) <= ROWS_UNDER_TABLES  # the confined matches' rows under grid type 4 lie under the two tables
        assert len(set(left[3, :k].tolist())) >= (40 if m >= 4096 else 20)  # ... and most of those rows are touched (54 there are)
        assert nleft.max() <= 255  # the plain mode takes the pair
        assert m < 4096 or nleft[3].max() >= 100  # large counts in those rows
        made.append((c, _oracle(oracle, c)))
        assert made[-1][1][2]["n_inliers"] > m // 4
    return made


@pytest.mark.parametrize("shuffle", [False, True])
def test_last_types_increments_under_the_tables(ctx, oracle, batch, types, region_cases, shuffle):
    """All five sizes in one launch (one per matches-per-thread class: 512 and 4096 + 63 with a wave tail, 10 240, 10 241 with a
    dealt-unit tail, 16 384). Shuffling the list leaves every match's verdict as it is: the expected bytes are the oracle's on the
    shuffled list."""
    cs = [c if not shuffle else _shuffled(c, 77 + i) for i, (c, _) in enumerate(region_cases)]
    wants = [w if not shuffle else _oracle(oracle, c) for c, (_, w) in zip(cs, region_cases)]
    got = _launch(ctx, batch, types, cs, in_query_order=not shuffle)
    for i, w in enumerate(wants):
        _assert_pair(*got, i, *w)


# ---- 2. fields with no owner, cells cut by the border, the sink's entry ---------------------------------------------------------------
# Twelve coherent matches, three in each quadrant around a centre, all into one right cell (tests/test_gpu_mark_table.py): a cell pair
# of 12 stands while T <= 4 x (number of neighbour pairs) -- thresh = 6 sqrt(T / numpair) <= 12 --, and falls when a grid type cuts
# the twelve in two. At the border the cell of a shifted grid type lies INSIDE the unshifted one, so being whole cannot single the
# shifted type out; "spoilers" do -- matches to anywhere, placed where only the other grid types' 3 x 3 neighbourhoods reach:
#   column 0, grid type 2: centre (0.25, 6.5) -- types 3 and 4 cut it along y; type 1's neighbourhood reaches x < 2, type 2's x < 1.5:
#                          20 spoilers at x in [1.55, 1.95] make T = 32 > 24 for type 1 alone;
#   row 0, grid type 3:    the same, transposed;
#   corner, grid type 4:   centre (0.25, 0.25), whole under all four; numpair = 4, T <= 16: six spoilers at y in [1.55, 1.95], x < 1.4
#                          (types 1 and 2 see them) and six at x in [1.55, 1.95], y < 1.4 (types 1 and 3): T = 24, 18, 18, 12.
QUADRANT = np.array([(0.08, 0.08), (0.15, 0.05), (0.05, 0.15)])
OFFSETS = np.concatenate([QUADRANT * s for s in ((1, 1), (-1, 1), (1, -1), (-1, -1))])


def _border_case():
    """-> (case in query order, {name: (queryIdx range, ...)})"""
    rng = np.random.default_rng(21)
    left, right, where = [], [], {}

    def add(name, lpts, rpts):
        n0 = sum(len(p) for p in left)
        left.append(np.asarray(lpts, dtype=np.float64))
        right.append(np.asarray(rpts, dtype=np.float64))
        where[name] = np.arange(n0, n0 + len(lpts))

    def anywhere(n):
        return np.stack([rng.uniform(0.01, 19.99, n), rng.uniform(0.01, 19.99, n)], axis=1)

    def box(n, x0, x1, y0, y1):
        return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], axis=1)

    add("column0", (0.25, 6.5) + OFFSETS, (12.5, 3.5) + OFFSETS)
    add("column0_spoilers", box(20, 1.55, 1.95, 6.1, 6.9), anywhere(20))
    add("row0", (6.5, 0.25) + OFFSETS, (5.5, 14.5) + OFFSETS)
    add("row0_spoilers", box(20, 6.1, 6.9, 1.55, 1.95), anywhere(20))
    add("corner", (0.25, 0.25) + OFFSETS, (16.5, 10.5) + OFFSETS)
    add("corner_spoilers", np.concatenate([box(6, 0.1, 1.4, 1.55, 1.95), box(6, 1.55, 1.95, 0.1, 1.4)]), anywhere(12))
    # half cells hx = 39 / hy = 39: twelve that stand (in hx = 37: cell 19 of grid type 2 is hx 37, 38) and three followers of the same
    # motion half a cell further, in hx = 39 -- nobody's under the x-shifted grid types; alone in their cell under the others, 3 < thresh
    add("hx37_stands", (18.75, 12.5) + OFFSETS, (3.5, 8.5) + OFFSETS)
    add("hx39_followers", (19.75, 12.5) + QUADRANT * (1, -1), (3.5, 8.5) + QUADRANT * (1, -1))
    add("hy37_stands", (8.5, 18.75) + OFFSETS, (15.5, 5.5) + OFFSETS)
    add("hy39_followers", (8.5, 19.75) + QUADRANT * (-1, 1), (15.5, 5.5) + QUADRANT * (-1, 1))
    # left points at x = width / y = height exactly: cell 20 of an axis, binned under no grid type; their motion is the standing clusters'
    never = np.array([(20.0, 6.5), (20.0, 12.5), (20.0, 19.99), (8.5, 20.0), (20.0, 20.0), (20.0, 0.0)])
    add("binned_nowhere", never, np.array([(12.5, 3.5), (3.5, 8.5), (3.5, 8.5), (15.5, 5.5), (15.5, 5.5), (12.5, 3.5)]) + 0.01)
    return _pair(_px(np.concatenate(left)), _px(np.concatenate(right))), where


def _moved(c, idx, dx, dy):
    """the case with the left points idx moved by (dx, dy) cells"""
    kp1 = c["kp1"].copy()
    kp1["x"][idx] += np.float32(dx * W / 20.0)
    kp1["y"][idx] += np.float32(dy * H / 20.0)
    return dict(c, kp1=kp1)


@pytest.fixture(scope="module")
def border_case(oracle):
    c, where = _border_case()
    left, nleft, inl = _per_type(oracle, c)
    # each border cluster stands under exactly one grid type, the shifted one that cuts its cell at the image's border
    for name, g in (("column0", 1), ("row0", 2), ("corner", 3)):
        assert [bool(inl[t, where[name]].all()) for t in range(4)] == [t == g for t in range(4)], name
        assert not inl[[t for t in range(4) if t != g]][:, where[name]].any(), name
    assert set(left[1, where["column0"]].tolist()) == {6 * 20} and set(left[2, where["row0"]].tolist()) == {6} and set(left[3, where["corner"]].tolist()) == {0}
    # the followers in the last half column / row: binned under the unshifted axis only, nobody's inliers -- but half a cell back,
    # inside the cell of the shifted grid type that holds the twelve, they would be
    for name, t_shift, t_other, step in (("hx39_followers", (1, 3), (0, 2), (-0.5, 0.0)), ("hy39_followers", (2, 3), (0, 1), (0.0, -0.5))):
        idx = where[name]
        assert (left[list(t_shift)][:, idx] == -1).all() and (left[list(t_other)][:, idx] >= 0).all(), name
        assert not inl[:, idx].any(), name
        assert inl[:, where[name.replace("39_followers", "37_stands")]].any(axis=0).all(), name
        assert _per_type(oracle, _moved(c, idx, *step))[2][t_shift[0], idx].all(), name
    assert (left[:, where["binned_nowhere"]] == -1).all() and not inl[:, where["binned_nowhere"]].any()
    return c, where


@pytest.mark.parametrize("shuffle", [False, True])
def test_border_cells_unowned_fields_and_the_sink(ctx, oracle, batch, types, border_case, shuffle):
    c, where = border_case
    if shuffle:
        c = _shuffled(c, 5)
    want, wmask, wres = _oracle(oracle, c)
    q = c["matches"]["queryIdx"]
    for name in ("column0", "row0", "corner", "hx37_stands", "hy37_stands"):
        assert wmask[np.isin(q, where[name])].all(), name
    for name in ("hx39_followers", "hy39_followers", "binned_nowhere"):
        assert not wmask[np.isin(q, where[name])].any(), name
    got = _launch(ctx, batch, types, [c], in_query_order=not shuffle)
    _assert_pair(*got, 0, want, wmask, wres)


# ---- 3. workgroups that follow each other on a CU ---------------------------------------------------------------------------------------
def test_followers_inherit_neither_fields_nor_counts(ctx, oracle, batch, types):
    """520 pairs in one launch (256 CUs: every CU runs a second workgroup, eight a third). The first 256 are dense in the regions
    of case 1 (512 matches, all confined, most of them survivors). Behind them, alternately: noise over the SAME left frame that keeps
    one match in fourteen of the dense pair's motion -- a field inherited from a dense pair's table would make exactly those inliers;
    the oracle keeps none -- and a sparse pair of 200 matches with survivors, whose output positions come from the count table."""
    rng = np.random.default_rng(31)
    dense, k = _region_case(6001, 512)
    assert k == 512 and set(_per_type(oracle, dense)[0][3].tolist()) <= ROWS_UNDER_TABLES
    a = np.stack([dense["kp1"]["x"], dense["kp1"]["y"]], axis=1).astype(np.float64)
    r = _px(np.stack([rng.uniform(0.01, 19.99, 512), rng.uniform(0.01, 19.99, 512)], axis=1))
    r[::14] = np.stack([dense["kp2"]["x"], dense["kp2"]["y"]], axis=1)[::14]
    noise = _pair(a, r)
    sl = np.stack([rng.uniform(12.05, 15.95, 200), rng.uniform(12.05, 15.95, 200)], axis=1)  # 4 x 4 cells, 12 each
    sparse = _pair(_px(sl), _px(sl + (-7.0, -9.0) + rng.uniform(-0.02, 0.02, sl.shape)))
    wd, wn, ws = _oracle(oracle, dense), _oracle(oracle, noise), _oracle(oracle, sparse)
    assert wd[2]["n_inliers"] > 300 and wn[2]["n_inliers"] == 0 and 100 < ws[2]["n_inliers"]
    frames = batch.FrameTable(ctx, [dense["kp1"], dense["kp2"], noise["kp2"], sparse["kp1"], sparse["kp2"]], [(W, H)] * 5)
    n_pairs = 520
    kind = [0 if i < 256 else 1 + (i & 1) for i in range(n_pairs)]
    cs = [(dense, noise, sparse)[t] for t in kind]
    got = _launch(ctx, batch, types, cs, frames=frames, frame_pairs=[((0, 1), (0, 2), (3, 4))[t] for t in kind], in_query_order=True)
    for i, t in enumerate(kind):
        _assert_pair(*got, i, *(wd, wn, ws)[t])


# ---- 4. a crowded restart that comes from the last grid type, a plain pair, a hand-over ---------------------------------------------------
def _background(rng, skip=()):
    left, right = [], []
    for cy in range(2, 18):
        for cx in range(2, 18):
            if (cx, cy) in skip:
                continue
            k = int(rng.integers(8, 24))
            left.append(np.stack([cx + 0.5 + rng.uniform(-0.45, 0.45, k), cy + 0.5 + rng.uniform(-0.45, 0.45, k)], axis=1))
            right.append(left[-1] + rng.uniform(-0.03, 0.03, (k, 2)))
    return left, right


def _corner_crowd_case(seed):
    """Seventy matches in each of the four half cells around the cell corner (7, 9): 70 per cell under grid type 1, 140 under types
    2 and 3, all 280 in one cell under type 4 -- and into four right cells, so no entry comes near its limit. Shuffled."""
    rng = np.random.default_rng(seed)
    quad = [np.stack([7.0 + sx * rng.uniform(0.05, 0.45, 70), 9.0 + sy * rng.uniform(0.05, 0.45, 70)], axis=1) for sx in (-1, 1) for sy in (-1, 1)]
    left, right = _background(rng, skip=[(6, 8), (7, 8), (6, 9), (7, 9)])  # (the four cells that meet at the corner hold the 280 alone)
    left = quad + left
    right = [q + (5.0, 3.0) for q in quad] + right
    return _shuffled(_pair(_px(np.concatenate(left)), _px(np.concatenate(right))), seed)


def _one_entry_case(seed, n):
    """n matches from one unshifted left cell into ONE right cell, on the same background. Shuffled."""
    rng = np.random.default_rng(seed)
    blob = np.stack([0.5 + rng.uniform(-0.3, 0.3, n), 0.5 + rng.uniform(-0.3, 0.3, n)], axis=1)
    left, right = _background(rng)
    return _shuffled(_pair(_px(np.concatenate([blob] + left)), _px(np.concatenate([blob + (12.0, 3.0)] + right))), seed)


def test_restart_from_the_last_grid_type_and_hand_over_in_one_launch(ctx, oracle, batch, types):
    crowd, plain, entry = _corner_crowd_case(51), cases.random_pair(5401, n=3000, size1=(W, H), inlier_frac=0.6), _one_entry_case(52, 256)
    _, nleft, _ = _per_type(oracle, crowd)
    assert nleft[:3].max() <= 255 and nleft[3].max() == 280 and nleft[3, 9 * 20 + 7] == 280  # the restart comes from grid type 4 alone
    mt = entry["matches"]
    blob = mt["queryIdx"] < 256
    cell = lambda kp, idx: (np.floor(kp["y"][idx] / np.float32(H) * 20).astype(int) * 20 + np.floor(kp["x"][idx] / np.float32(W) * 20).astype(int))  # noqa: E731
    assert set(cell(entry["kp1"], mt["queryIdx"][blob]).tolist()) == {0} and len(set(cell(entry["kp2"], mt["trainIdx"][blob]).tolist())) == 1  # one entry of 256
    cs = [crowd, plain, entry]
    got = _launch(ctx, batch, types, cs)
    wants = [_oracle(oracle, c) for c in cs]
    assert all(w[2]["n_inliers"] > 0 for w in wants)
    for i, w in enumerate(wants):
        _assert_pair(*got, i, *w)


# ---- the other instantiations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["GMS_IDENT=1", "GMS_DEAL=1"])
def test_other_instantiations_whole_file_again(setting):
    """GMS_IDENT=1 / GMS_DEAL=1 (read once per process): the identity-query body for the pairs in query order -- they assert that
    GMS_QUERY_IDENT_MISSES does not move --, and the dealt instantiations."""
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "not whole_file_again"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, **dict(s.split("=") for s in setting.split(","))))
    assert res.returncode == 0, res.stdout[-3000:]
