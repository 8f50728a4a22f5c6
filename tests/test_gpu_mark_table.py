"""-m gpu: the mark table of the byte-matrix kernel's default-flags body (dense_pair_plain) against
oracle/gms_ref.c, byte for byte. The body keeps the verdicts of the four grid types in registers, builds one table of 1600 half
cells x 4 grid types behind the last one and marks every match from the one entry of its left half cell. The cases are the places
where such a table can be wrong while everything else is right: a cell pair that stands under exactly one grid type (each of the
four), the half cells at the image's border (where a shifted grid type has no cell) and left points that are binned nowhere,
workgroups that follow each other on a CU (nothing may be inherited from the LDS), every matches-per-thread class with wave and
unit tails in query order and shuffled, and the crowded mode and the hand-over to the general path in one launch.
The whole file runs again in child processes with GMS_IDENT=1 (the identity-query body for the pairs in query order) and GMS_DEAL=1
(the dealt instantiations)."""
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


def _oracle(oracle, c):
    rc, want, wmask, wres = oracle.match(c["size1"], c["size2"], c["kp1"], c["kp2"], c["matches"], False, False, 6.0)
    assert rc == 0
    return want, np.asarray(wmask, dtype=np.uint8), wres


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


def _check(ctx, oracle, batch, types, cs, in_query_order=False):
    got = _launch(ctx, batch, types, cs, in_query_order=in_query_order)
    wants = [_oracle(oracle, c) for c in cs]
    for i, w in enumerate(wants):
        _assert_pair(*got, i, *w)
    return wants


# ---- a cell pair that stands under exactly one grid type ----------------------------------------------------------------------------
# Twelve coherent matches, three in each quadrant around a centre, all into one right cell. Under a grid type that has the centre
# inside a cell they are one cell pair of 12: T = 12 + the noise in the nine cells, thresh = 6 sqrt(T / 9) < 12 up to T = 35. A grid
# type that cuts them in two along an axis sees 6 + 6 in neighbouring left cells and ONE right cell -- the neighbour's matches are not
# at the neighbouring right cell, so each half scores 6 against a thresh above 6 sqrt(12 / 9) = 6.9; cut in four, 3 against the same.
QUADRANT = np.array([(0.08, 0.08), (0.15, 0.05), (0.05, 0.15)])
OFFSETS = np.concatenate([QUADRANT * s for s in ((1, 1), (-1, 1), (1, -1), (-1, -1))])
ONE_TYPE = {"cell_centre": ((7.5, 9.5), 0), "vertical_edge": ((7.0, 9.5), 1), "horizontal_edge": ((7.5, 9.0), 2), "cell_corner": ((7.0, 9.0), 3)}


def _whole_under(left_cells, g):
    """all points in ONE cell of the grid type shifted by (g & 1, g >> 1) half cells"""
    cx = np.floor(left_cells[:, 0] + 0.5 * (g & 1)).astype(int)
    cy = np.floor(left_cells[:, 1] + 0.5 * (g >> 1)).astype(int)
    return len(set(zip(cx.tolist(), cy.tolist()))) == 1


def _one_type_case(name, shuffle):
    centre, g = ONE_TYPE[name]
    rng = np.random.default_rng(100 + g)
    blob_l = np.asarray(centre) + OFFSETS
    blob_r = np.asarray((12.5, 3.5)) + OFFSETS
    assert [_whole_under(blob_l, t) for t in range(4)] == [t == g for t in range(4)] and _whole_under(blob_r, 0)
    n_noise = 300
    left = np.concatenate([_px(blob_l), np.stack([rng.uniform(0, W - 1, n_noise), rng.uniform(0, H - 1, n_noise)], axis=1)])
    right = np.concatenate([_px(blob_r), np.stack([rng.uniform(0, W - 1, n_noise), rng.uniform(0, H - 1, n_noise)], axis=1)])
    c = _pair(left, right)
    if shuffle:
        c["matches"] = c["matches"][rng.permutation(len(left))]
    return c


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("name", list(ONE_TYPE))
def test_cell_pair_that_stands_under_one_grid_type(ctx, oracle, batch, types, name, shuffle):
    c = _one_type_case(name, shuffle)
    (want, wmask, wres), = _check(ctx, oracle, batch, types, [c], in_query_order=not shuffle)
    assert wres["n_inliers"] > 0
    assert wmask[c["matches"]["queryIdx"] < len(OFFSETS)].all()  # the blob's twelve are among the survivors


# ---- the image's border: half cells that a shifted grid type does not bin, and points binned nowhere ---------------------------------
def _edges_case(shuffle):
    rng = np.random.default_rng(7)
    left = []
    # first and last half column, first and last half row (x or y in [0, 0.5) and [19.5, 20) cells), the four corners' half cells
    for cx, cy, ex, ey in [(0.25, 6.5, 0.2, 0.4), (19.75, 6.5, 0.2, 0.4), (11.5, 0.25, 0.4, 0.2), (11.5, 19.75, 0.4, 0.2),
                           (0.25, 0.25, 0.2, 0.2), (19.75, 0.25, 0.2, 0.2), (0.25, 19.75, 0.2, 0.2), (19.75, 19.75, 0.2, 0.2)]:
        left.append(_px(np.stack([cx + rng.uniform(-ex, ex, 40), cy + rng.uniform(-ey, ey, 40)], axis=1)))
    left = np.clip(np.concatenate(left), 0, [W - 0.01, H - 0.01])
    right = np.clip(left + rng.uniform(-2, 2, left.shape), 0, [W - 0.01, H - 0.01])
    # left points at x = width (and y = height) exactly: cell 20 of an axis, binned under no grid type -- their code word is the sink's
    never = np.array([(W, 0.3 * H), (W, 0.5 * H), (W, H - 0.01), (0.4 * W, H), (W, H), (W, 0.0)], dtype=np.float64)
    never_r = _px(np.stack([19.75 + rng.uniform(-0.2, 0.2, len(never)), 6.5 + rng.uniform(-0.4, 0.4, len(never))], axis=1))
    noise = 200
    left = np.concatenate([left, never, np.stack([rng.uniform(0, W - 1, noise), rng.uniform(0, H - 1, noise)], axis=1)])
    right = np.concatenate([right, never_r, np.stack([rng.uniform(0, W - 1, noise), rng.uniform(0, H - 1, noise)], axis=1)])
    c = _pair(left, right)
    if shuffle:
        c["matches"] = c["matches"][rng.permutation(len(left))]
    return c


@pytest.mark.parametrize("shuffle", [False, True])
def test_border_half_cells_and_points_binned_nowhere(ctx, oracle, batch, types, shuffle):
    c = _edges_case(shuffle)
    (want, wmask, wres), = _check(ctx, oracle, batch, types, [c], in_query_order=not shuffle)
    q = c["matches"]["queryIdx"]
    for blob in range(8):  # every border blob has survivors: it stands under grid type 1 at least
        assert wmask[(q >= 40 * blob) & (q < 40 * blob + 40)].sum() > 20, blob
    assert not wmask[(q >= 320) & (q < 326)].any()  # the points binned nowhere are nobody's inliers


# ---- workgroups that follow each other on a CU -------------------------------------------------------------------------------------
def test_nothing_is_inherited_from_the_previous_workgroup(ctx, oracle, batch, types):
    """514 pairs of 512 matches in one launch (256 CUs: every CU runs a second workgroup, two a third), alternately a pair with many
    survivors and a pair of noise over the SAME left frame: the noise pair keeps one match in fourteen of the good pair's motion (a
    stale table entry of the good pair would make exactly those inliers) and sends the others anywhere, so that no cell pair stands.
    The oracle keeps nothing of it; neither may the kernel, behind whichever workgroup it runs."""
    rng = np.random.default_rng(11)
    n = 512
    a = np.stack([rng.uniform(0.35 * W, 0.65 * W, n), rng.uniform(0.35 * H, 0.65 * H, n)], axis=1)  # 6 x 6 cells, 14 each
    b = a + [3.0 * W / 20.0, 4.0 * H / 20.0] + rng.uniform(-2, 2, a.shape)
    r = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], axis=1)
    r[::14] = b[::14]
    good, noise = _pair(a, b), _pair(a, r)
    wg, wn = _oracle(oracle, good), _oracle(oracle, noise)
    assert wg[2]["n_inliers"] > 400 and wn[2]["n_inliers"] == 0
    frames = batch.FrameTable(ctx, [good["kp1"], good["kp2"], noise["kp2"]], [(W, H)] * 3)
    n_pairs = 514
    cs = [good if i % 2 == 0 else noise for i in range(n_pairs)]
    got = _launch(ctx, batch, types, cs, frames=frames, frame_pairs=[(0, 1) if i % 2 == 0 else (0, 2) for i in range(n_pairs)], in_query_order=True)
    for i in range(n_pairs):
        _assert_pair(*got, i, *(wg if i % 2 == 0 else wn))


# ---- every body: the three matches-per-thread classes, tails of a wave and of an 8-match unit ------------------------------------------
@pytest.fixture(scope="module")
def sized():
    """m -> (an identity-query pair of m matches over m keypoints, its shuffled twin), built once, never modified"""
    made = {}

    def get(m):
        if m not in made:
            c = cases.random_pair(5200 + m, n=m, size1=(W, H), inlier_frac=0.6)
            assert len(c["matches"]) == m == len(c["kp1"]) and (c["matches"]["queryIdx"] == np.arange(m)).all()
            made[m] = (c, dict(c, matches=c["matches"][np.random.default_rng(m).permutation(m)]))
        return made[m]
    return get


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("m", [1, 65, 4096, 4097, 4099, 10241])
def test_sizes_in_query_order_and_shuffled(ctx, oracle, batch, types, sized, m, shuffle):
    c = sized(m)[1 if shuffle else 0]
    (want, wmask, wres), = _check(ctx, oracle, batch, types, [c], in_query_order=not shuffle)
    assert m < 4096 or wres["n_inliers"] > 0  # (there is something to compare)


# ---- crowded mode and the hand-over to the general path, a normal pair between them ----------------------------------------------------
def _crowded_case(seed, n, ext):
    """n matches from one unshifted left cell into one right cell's neighbourhood, on a coherent background (shuffled)."""
    rng = np.random.default_rng(seed)
    left = [_px(np.stack([0.5 + rng.uniform(-ext, ext, n), 0.5 + rng.uniform(-ext, ext, n)], axis=1))]
    right = [left[0] + [12.0 * W / 20.0, 3.0 * H / 20.0]]
    for cy in range(2, 18):
        for cx in range(2, 18):
            k = int(rng.integers(8, 24))
            left.append(_px(np.stack([cx + 0.5 + rng.uniform(-0.45, 0.45, k), cy + 0.5 + rng.uniform(-0.45, 0.45, k)], axis=1)))
            right.append(left[-1] + rng.uniform(-3, 3, (k, 2)))
    c = _pair(np.concatenate(left), np.concatenate(right))
    c["matches"] = c["matches"][rng.permutation(len(c["matches"]))]
    return c


def test_crowded_mode_and_hand_over_in_one_launch(ctx, oracle, batch, types):
    """256 matches spread over one unshifted cell and over several right cells (crowded body: 16-bit nLeft, the same mark table), a
    normal pair, 256 from one left cell into ONE right cell (the entry's byte wraps: the general path takes the pair after the
    crowded body has been through some grid types), a pair whose one entry ends at 255 exactly (stays), a normal pair."""
    rng = np.random.default_rng(3)
    spread = _crowded_case(41, 256, 0.45)
    far = rng.permutation(256)[:100]  # a hundred of the crowded cell's matches go elsewhere: no entry near its limit
    kp2 = spread["kp2"].copy()
    kp2["x"][far] = rng.uniform(0, W - 1, len(far)).astype(np.float32)
    kp2["y"][far] = rng.uniform(0, H - 1, len(far)).astype(np.float32)
    spread = dict(spread, kp2=kp2)
    cs = [spread, cases.random_pair(5301, n=3000, size1=(W, H), inlier_frac=0.6), _crowded_case(42, 256, 0.3),
          _crowded_case(43, 255, 0.3), cases.random_pair(5302, n=5000, size1=(W, H), inlier_frac=0.5)]
    wants = _check(ctx, oracle, batch, types, cs)
    assert all(w[2]["n_inliers"] > 0 for w in wants)


# ---- the other instantiations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["GMS_IDENT=1", "GMS_DEAL=1", "GMS_IDENT=1,GMS_DEAL=1"])
def test_other_instantiations_whole_file_again(setting):
    """GMS_IDENT=1 / GMS_DEAL=1 (read once per process): the identity-query body for the pairs in query order -- they assert that
    GMS_QUERY_IDENT_MISSES does not move --, the dealt instantiations, and both."""
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "not whole_file_again"],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ, **dict(s.split("=") for s in setting.split(","))))
    assert res.returncode == 0, res.stdout[-3000:]
