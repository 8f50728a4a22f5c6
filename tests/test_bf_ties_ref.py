"""CPU: tests/bf_ties_ref.py -- the restatement of what the matrix-core L2 matcher ranks by and of its tie classes -- against plain
arithmetic and oracle/bf_ref.c, on the inputs of the GPU tests (tests/test_gpu_bf.py), whose stated properties are asserted here on
the reference side alone."""
import numpy as np
import pytest

import bf_ties_ref as T


def _plain_d2(q, t):
    d = np.asarray(q, dtype=np.int64)[:, None, :] - np.asarray(t, dtype=np.int64)[None, :, :]
    return (d * d).sum(axis=2)


def _integer_pairs():
    """(name, query, train) of every pair of integer-valued frames the GPU tests send to the matrix-core L2 kernel."""
    out = []
    rep = T.repeated_rows_frames()
    for k in range(len(T.REPEATED_ROWS_CASES)):
        out += [(f"repeated{k}", rep[2 * k], rep[2 * k + 1]), (f"repeated{k}_reverse", rep[2 * k + 1], rep[2 * k])]
    q, t, *_ = T.constructed_groups_of_eight()
    out.append(("constructed", q, t))
    mixed = T.mixed_record_frames("l2_mfma")
    out += [(f"mixed_{a}_{b}", mixed[a], mixed[b]) for a, b, m in dict.fromkeys(T.mixed_records())
            if 0 <= a < 4 and 0 <= b < 4 and len(mixed[a]) and len(mixed[b])]
    edge, flagged = T.l2_edge_frames()
    out += [("edge_0_1", edge[0], edge[1]), ("edge_1_0", edge[1], edge[0])]
    same = np.full((300, 128), 255.0, dtype=np.float32)
    out.append(("all_equal", same[:70], same))
    return out


INTEGER_PAIRS = _integer_pairs()


def test_d2_identity():
    rng = np.random.default_rng(1)
    q, t = rng.integers(0, 256, (40, 128)), rng.integers(0, 256, (90, 128))
    assert (T.d2_by_parts(q, t) == _plain_d2(q, t)).all()
    q, t = rng.choice([0, 255], (40, 128)), rng.choice([0, 255], (90, 128))
    q[0], q[1], t[0], t[1] = 0, 255, 255, 0           # the largest distance there is, both ways round
    assert (T.d2_by_parts(q, t) == _plain_d2(q, t)).all()
    assert T.d2_by_parts(q, t).max() == 128 * 255 * 255
    # P orders like d^2 up to one: d^2 - c(query) is 2 P or 2 P + 1
    a, w = T.train_side(t)
    p = (w >> 1)[None, :] + T.query_side(q) @ a.T
    rest = T.d2_by_parts(q, t) - T.bracket(T.query_side(q))[:, None] - 2 * p
    assert ((rest == 0) | (rest == 1)).all()


@pytest.mark.parametrize("name,q,t", INTEGER_PAIRS, ids=[p[0] for p in INTEGER_PAIRS])
def test_classes_name_the_block_of_the_first_minimum(oracle, name, q, t):
    want = oracle.bf_match(q, t, False)
    c = T.tie_classes(q, t)
    for i in range(len(q)):
        assert int(want["trainIdx"][i]) // 32 in T.candidate_blocks(c, i), (name, i)
    # and the final search over those blocks, one decision per group, is the oracle's answer
    idx, d2 = T.final_search(q, t, c, group_uniform=True)
    assert (idx == want["trainIdx"]).all() and (np.sqrt(d2.astype(np.float32)) == want["distance"]).all()


def test_all_equal_frame_is_the_many_blocks_class():
    same = np.full((300, 128), 255.0, dtype=np.float32)
    c = T.tie_classes(same[:70], same)
    assert (c.nt >= 2).all() and (c.blk == 0).all() and (c.hsel == 2).all()


def test_repeated_rows_mix_the_classes(oracle):
    """At least half of the aligned groups of eight queries hold both an nt == 1 and an nt >= 2 query -- and the search with one
    decision per LANE (row_shr:4 as the last add), which the kernel ran before, goes wrong there and nowhere else."""
    rep = T.repeated_rows_frames()
    for k, (n_q, n_t, pool) in enumerate(T.REPEATED_ROWS_CASES):
        q, t = rep[2 * k], rep[2 * k + 1]
        assert q.shape == (n_q, 128) and t.shape == (n_t, 128) and len(np.unique(t, axis=0)) <= pool
        c = T.tie_classes(q, t)
        mixed, groups = T.mixed_groups(c)
        assert groups == n_q // 8 and 2 * mixed >= groups
        want = oracle.bf_match(q, t, False)
        idx, d2 = T.final_search(q, t, c, group_uniform=False)
        wrong = np.nonzero(idx != want["trainIdx"])[0]
        assert len(wrong) > 0 and (c.nt[wrong] == 1).all()
        assert (idx[wrong] // 32 == want["trainIdx"][wrong] // 32).all()
        assert (np.sqrt(d2[wrong].astype(np.float32)) < want["distance"][wrong]).all()


def test_constructed_groups_are_what_they_say(oracle):
    q, t, roles, places, want_rows = T.constructed_groups_of_eight()
    assert len(t) <= 1500 and len(q) % 8 == 0
    for g in range(0, len(q), 8):
        assert sorted(roles[g:g + 8]) == sorted(T.GROUP_ROLES)
    d2 = _plain_d2(q, t)
    spots = [(b, r) for sp in places for b, r in sp]
    assert len(set(spots)) == len(spots)
    assert {(b // 4) & 1 for b, r in spots} == {0, 1}                 # both staging buffers
    assert {r >> 2 for b, r in spots} == {0, 1, 4, 7}                 # rows 0..3, 4..7, 16..19, 28..31: both lane halves
    for i, (role, sp) in enumerate(zip(roles, places)):
        rows = [b * 32 + r for b, r in sp]
        d = d2[i, rows]
        others = np.delete(d2[i], rows)
        assert others.min() > d.max() + 1000                          # nothing else comes near
        assert len({b for b, r in sp}) == len(sp) and rows == sorted(rows)
        want_d = {"copies": [0, 0, 0], "third_below": [1, 1, 0], "later_closer": [1, 0], "later_farther": [0, 1], "later_equal": [0, 0]}[role]
        assert (d - d.min()).tolist() == want_d
        if role == "later_equal":
            assert not (t[rows[0]] == t[rows[1]]).all()
        if role == "third_below":
            assert not (t[rows[0]] == t[rows[1]]).all()
    # the blocks share P: the classes are the ones the test is about
    c = T.tie_classes(q, t)
    for i, (role, sp) in enumerate(zip(roles, places)):
        assert (c.nt[i] >= 2) == (role in ("copies", "third_below")) and (c.nt[i] == 1) == (role not in ("copies", "third_below"))
    want = oracle.bf_match(q, t, False)
    assert (want["trainIdx"] == want_rows).all()
    idx, _ = T.final_search(q, t, c, group_uniform=False)             # the earlier search goes wrong on it
    assert (idx != want_rows).any()


def test_l2_edge_frames_are_flagged_as_stated():
    frames, flagged = T.l2_edge_frames()
    for f, bad in zip(frames, flagged):
        is_u8 = (f >= 0) & (f <= 255) & (f == np.floor(f))
        assert (not is_u8.all()) == bad
        if bad and len(f) == 40:
            assert (~is_u8).sum() == 1 and (not is_u8[0, 0] or not is_u8[-1, -1])
    assert np.signbit(frames[0][0, 0]) and frames[0].max() == 255.0
    ab = T.l2_edge_pairs(len(frames))
    assert {a for a, b in ab} == {b for a, b in ab} == set(range(len(frames)))


def test_hamming_extremes_reach_every_distance(oracle):
    frames = T.hamming_extreme_frames()
    seen = set()
    for a in range(len(frames)):
        for b in range(len(frames)):
            seen |= set(oracle.bf_match(frames[a], frames[b], True)["distance"].tolist())
    assert {0.0, 1.0, 255.0, 256.0} <= seen
    bits = np.unpackbits(frames[0], axis=1).sum(axis=1)
    assert [int(bits[r]) for r in (0, 31, 32, 63, 64, 127, 128)] == [0, 256, 1, 255, 0, 256, 1]
