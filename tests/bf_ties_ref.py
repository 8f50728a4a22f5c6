"""TEST INFRASTRUCTURE, NOT PRODUCT. CPU restatement of what the matrix-core L2 matcher (bf_mfma_kernel<false>, csrc/bf_kernels.hip)
ranks train rows by, of its tie bookkeeping, and of its final exact search -- this project's own kernel, not the reference.

For integer rows 0..255 (train side a, query side b):
    a' = a - 128        w = sum (a' + 1)^2        ~b' = 127 - b
    d^2 = w + 2 sum a'.~b' + [sum ~b'^2 + 2 sum ~b']               (a - b = (a' + 1) + ~b')
    P = floor(w / 2) + sum a'.~b'                                  what the accumulators hold
The row of the smallest d^2 has the smallest P, but two rows whose d^2 differ by one can share it. Per query and per lane half
(the rows r of a 32-row block with ((r >> 2) & 1) == half) the kernel keeps the first block that reached the minimal block minimum
(bestt), how often that value came back in later blocks (ties) and the last of them (bestt2); the two halves are merged, and the
final search sees per query: blk, nt = 0 / 1 / >= 2, blk2, and hsel (the half of blk that holds the minimum; 2 = either).

tie_classes()   that bookkeeping.
final_search()  the final search lane by lane -- eight lanes per query, the 16-byte pieces summed by DPP adds, eight queries per wave
                iteration. group_uniform=False models row_shr:4 as the last add: only lanes 4..7 of a group hold d^2 and every lane
                decides on its own value, which is the defect DESIGN.md section 4.5b records (a group that went through the second-block
                step loads its next "row" from two blocks once the wave enters the all-blocks loop for another group). True models
                the half-mirror add: every lane holds d^2, one decision per group.
The inputs of the GPU tests (tests/test_gpu_bf.py) are built here too, so that the CPU tests can state their properties."""
from collections import namedtuple

import numpy as np

K_BIG = 0x3FFFFFFF          # the start value of a row past the end of the frame
HALF_OF_ROW = (np.arange(32) >> 2) & 1

TieClasses = namedtuple("TieClasses", "nt blk blk2 hsel n_blocks")


def train_side(rows):
    """(a' [n, 128], w [n]) of integer rows 0..255."""
    a = np.asarray(rows).astype(np.int64) - 128
    return a, ((a + 1) ** 2).sum(axis=1)


def query_side(rows):
    """~b' [n, 128]."""
    return 127 - np.asarray(rows).astype(np.int64)


def bracket(nb):
    return (nb * nb).sum(axis=1) + 2 * nb.sum(axis=1)


def d2_by_parts(query, train):
    """d^2 [n_q, n_t] as the kernel assembles it."""
    a, w = train_side(train)
    nb = query_side(query)
    return w[None, :] + 2 * (nb @ a.T) + bracket(nb)[:, None]


def block_minima(query, train):
    """P of every (query, train row) folded as the matrix pass folds it: [2 halves][n_q, blocks], the frame padded to whole staging
    steps of 128 rows with the last row repeated under a norm that never wins."""
    a, w = train_side(train)
    nb = query_side(query)
    n_t = len(a)
    n_blk = 4 * ((n_t + 127) // 128)
    p = (w >> 1)[None, :] + nb @ a.T
    pad = n_blk * 32 - n_t
    if pad:
        p = np.concatenate([p, np.repeat(K_BIG + (nb @ a[-1])[:, None], pad, axis=1)], axis=1)
    p = p.reshape(len(nb), n_blk, 32)
    return [p[:, :, HALF_OF_ROW == h].min(axis=2) for h in (0, 1)]


def tie_classes(query, train):
    """What the final search sees per query (train must hold at least one row). nt is the kernel's own count, not clipped."""
    n_q = len(query)
    halves = []
    for mn in block_minima(query, train):
        bestv = np.full(n_q, K_BIG, dtype=np.int64)
        bestt, ties, bestt2 = (np.zeros(n_q, dtype=np.int64) for _ in range(3))
        for blk in range(mn.shape[1]):            # block_compare
            lt, eq = mn[:, blk] < bestv, mn[:, blk] == bestv
            ties = np.where(lt, 0, ties + eq)
            bestt2 = np.where(eq, blk, bestt2)
            bestv = np.where(lt, mn[:, blk], bestv)
            bestt = np.where(lt, blk, bestt)
        halves.append((bestv, bestt, ties, bestt2))
    # the merge, as a lane of half 0 runs it (the final search reads lane i & 31)
    (bv, bt, ti, b2), (ov, ot, oti, o2) = halves
    less, same = ov < bv, ov == bv
    lo, hi = np.minimum(bt, ot), np.maximum(bt, ot)
    nt = np.where(less, oti, np.where(same, np.where((ti | oti) != 0, 2, (lo != hi).astype(np.int64)), ti))
    hsel = np.where(less, 1, np.where(same, np.where(lo == hi, 2, np.where(bt == lo, 0, 1)), 0))
    blk = np.where(less, ot, np.where(same, lo, bt))
    blk2 = np.where(less, o2, np.where(same, hi, b2))
    return TieClasses(nt, blk, blk2, hsel, (len(train) + 31) // 32)


def candidate_blocks(c, i):
    """The blocks the final search walks for query i."""
    if c.nt[i] == 0:
        return [int(c.blk[i])]
    if c.nt[i] == 1:
        return [int(c.blk[i]), int(c.blk2[i])]
    return list(range(int(c.blk[i]), c.n_blocks))


def mixed_groups(c):
    """(aligned groups of eight consecutive queries that hold both an nt == 1 and an nt >= 2 query, groups in all)."""
    n = len(c.nt)
    groups = [c.nt[g:g + 8] for g in range(0, n, 8)]
    return sum(1 for g in groups if (g == 1).any() and (g >= 2).any()), len(groups)


def final_search(query, train, c, group_uniform):
    """(trainIdx, d^2) per query from the final search run lane by lane over waves of 128 query columns."""
    a, w = train_side(train)
    nb_all = query_side(query)
    m, n_t = len(query), len(a)
    lane = np.arange(64)
    piece, grp = lane & 7, lane >> 3
    cols = piece[:, None] * 16 + np.arange(16)[None, :]
    last_src = (lane & ~7) | (7 - piece) if group_uniform else lane - 4     # row_half_mirror / row_shr:4
    last_ok = np.ones(64, bool) if group_uniform else (lane & 15) >= 4      # (bound_ctrl: a lane without a source adds 0)
    out_idx, out_d2 = np.full(m, -1, dtype=np.int64), np.zeros(m, dtype=np.int64)

    for i0 in range(0, m, 8):                                    # a wave's iterations never straddle waves: 128 is a multiple of 8
        q = np.minimum(i0 + grp, m - 1)
        nt, blk2, hsel = c.nt[q], c.blk2[q], c.hsel[q]
        blk = c.blk[q].copy()
        nb = nb_all[q[:, None], cols]
        query_part = (nb * nb).sum(axis=1) + 2 * nb.sum(axis=1)

        def block_key(b, r):                                     # l2_block_key: b [64] per lane, r [64, ROWS]
            row = b[:, None] * 32 + r
            rr = np.minimum(row, n_t - 1)
            d2 = 2 * (a[rr[:, :, None], cols[:, None, :]] * nb[:, None, :]).sum(axis=2) + query_part[:, None]
            d2 = d2 + d2[lane ^ 1]
            d2 = d2 + d2[lane ^ 2]
            d2 = d2 + np.where(last_ok[:, None], d2[np.maximum(last_src, 0)], 0)
            d2 = d2 + w[rr]
            key = (((d2 & 0xFFFFFFFF) << 5) & 0xFFFFFFFF) | r
            return np.where(row < n_t, key, 0xFFFFFFFF).min(axis=1)

        all_rows = np.broadcast_to(np.arange(32), (64, 32))
        if not (hsel == 2).any():
            i = np.arange(16)
            key = block_key(blk, 8 * (i >> 2)[None, :] + 4 * hsel[:, None] + (i & 3)[None, :])
        else:
            key = block_key(blk, all_rows)
        if (nt == 1).any():
            b = np.where(nt == 1, blk2, blk)
            k2 = block_key(b, all_rows)
            take = (k2 >> 5) < (key >> 5)
            key, blk = np.where(take, k2, key), np.where(take, b, blk)
        if (nt >= 2).any():
            first = blk.copy()
            for bb in range(c.n_blocks):
                walk = (nt >= 2) & (bb > first)
                if not walk.any():
                    continue
                b = np.where(walk, bb, blk)
                k2 = block_key(b, all_rows)
                take = (k2 >> 5) < (key >> 5)
                key, blk = np.where(take, k2, key), np.where(take, b, blk)
        for g in range(8):
            if i0 + g < m:
                out_idx[i0 + g] = blk[8 * g + 7] * 32 + (key[8 * g + 7] & 31)
                out_d2[i0 + g] = key[8 * g + 7] >> 5
    return out_idx, out_d2


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
def sparse_rows(rng, n):
    """n rows of 128 values: 60 % zeros, the rest integers 0..39."""
    return np.where(rng.uniform(size=(n, 128)) < 0.4, rng.integers(0, 40, (n, 128)), 0).astype(np.float32)


REPEATED_ROWS_CASES = [(96, 1536, 600), (64, 1024, 400)]       # (queries, train rows, distinct train rows)
REPEATED_ROWS_SEED = 91


def repeated_rows_frames():
    """[query frame, train frame] per case of REPEATED_ROWS_CASES, from one generator: a train frame is drawn with replacement
    from a pool of distinct rows, the queries are independent of the pool."""
    rng = np.random.default_rng(REPEATED_ROWS_SEED)
    frames = []
    for n_q, n_t, pool in REPEATED_ROWS_CASES:
        rows = sparse_rows(rng, pool)
        frames += [sparse_rows(rng, n_q), rows[rng.integers(0, pool, n_t)].copy()]
    return frames


GROUP_ROLES = ["copies", "third_below", "later_closer", "later_farther", "later_closer", "later_equal", "later_closer", "later_farther"]
ROW_CHOICES = [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 28, 29, 30, 31]      # lane half 0, 1, 0, 1 of a block


def constructed_groups_of_eight(n_groups=4, n_t=1500, seed=17):
    """(queries, train, roles, places, want): every aligned group of eight queries holds, in an order that turns with the group,
    the roles of GROUP_ROLES. places[i] = the (block, row inside the block) of query i's planted rows in frame order, want[i] the
    train row that must win. Everything else in the frame is far from every query (asserted by the CPU tests).
      copies          the same nearest row in three blocks: the first wins
      third_below     d^2 = D + 1 in two blocks, D in a third, all three sharing P: the third wins
      later_closer    D + 1, then D in a later block, sharing P: the later wins
      later_farther   D, then D + 1;  later_equal: D, then another row at D: the earlier wins"""
    rng = np.random.default_rng(seed)
    n_q = 8 * n_groups
    queries, train = sparse_rows(rng, n_q), sparse_rows(rng, n_t)
    c_par = bracket(query_side(queries)) & 1
    taken, roles, places, want = set(), [], [], []
    for i in range(n_q):
        role = GROUP_ROLES[(i + i // 8) % 8]
        free = np.nonzero(queries[i] == 0)[0]
        at = rng.permutation(free)
        pert = np.zeros(128, dtype=np.float32)
        pert[at[:14]] = rng.integers(18, 34, 14)
        if (int((pert ** 2).sum()) & 1) != c_par[i]:       # D and D + 1 share P when D - c(query) is even
            pert[at[14]] = 1.0
        near = queries[i] + pert
        step = np.zeros((3, 128), dtype=np.float32)
        step[0, at[15]] = step[1, at[16]] = 1.0             # two different rows at D + 1
        step[2, at[0]], step[2, at[17]] = -pert[at[0]], pert[at[0]]   # another row at D
        rows = {"copies": [near, near, near], "third_below": [near + step[0], near + step[1], near],
                "later_closer": [near + step[0], near], "later_farther": [near, near + step[0]],
                "later_equal": [near, near + step[2]]}[role]
        while True:
            blks = np.sort(rng.choice(n_t // 32, len(rows), replace=False))      # whole blocks only
            spot = [(int(b), int(rng.choice(ROW_CHOICES))) for b in blks]
            if not taken & set(spot):
                break
        taken |= set(spot)
        for (b, r), row in zip(spot, rows):
            train[b * 32 + r] = row
        winner = {"copies": 0, "third_below": 2, "later_closer": 1, "later_farther": 0, "later_equal": 0}[role]
        roles.append(role)
        places.append(spot)
        want.append(spot[winner][0] * 32 + spot[winner][1])
    return queries, train, roles, places, np.array(want)


# ---- record edges of gms_bfmatch_device ----------------------------------------------------------------------------------------------
MIXED_FORMS = ["hamming_mfma", "hamming_valu1", "hamming_valu4", "l2_mfma", "l2_loop"]


def mixed_record_frames(form):
    """Frames for the launch of mixed records: 0 = 700 rows, 1 = no rows, 2 = 300 rows drawn from 40 distinct ones, 3 = 129 rows."""
    rng = np.random.default_rng(41 + MIXED_FORMS.index(form))
    if form.startswith("hamming"):
        make = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    elif form == "l2_mfma":
        make = lambda n: sparse_rows(rng, n)
    else:
        make = lambda n: (rng.uniform(size=(n, 128)) * 3.0).astype(np.float32)     # no frame is integer-valued: the loop kernel
    return [make(700), make(0), make(40)[rng.integers(0, 40, 300)].copy(), make(129)]


def mixed_records(repeat=1):
    """[(frame_a, frame_b, m)] of one launch over mixed_record_frames: every edge of a record, valid pairs between the invalid ones,
    the whole list `repeat` times over."""
    n_frames = 4
    recs = [(3, 2, 129),
            (0, 1, 700),                                                    # train frame of 0 rows
            (1, 0, 700), (0, 2, 0), (1, 1, 5),                              # query frame of 0 rows, m = 0
            (0, 2, 1), (0, 3, 255), (0, 2, 256), (0, 3, 257), (0, 2, 513),  # m < n(frame_a)
            (2, 0, 5000), (3, 0, 130),                                      # m > n(frame_a)
            (0, 0, 700), (2, 2, 300),                                       # a frame with itself
            (-1, 0, 10), (2, 3, 300), (0, n_frames, 10), (0, 2, -1), (n_frames, -1, 3),   # invalid records round a valid one
            (2, 3, 7)]
    return recs * repeat


def l2_edge_frames():
    """(frames, which of them must be flagged): integer-valued frames, and frames that are integer-valued but for ONE element --
    the last of the last row or the first of the first -- or, the last frame, hold nothing but NaN."""
    rng = np.random.default_rng(43)
    good0, good1 = sparse_rows(rng, 65), sparse_rows(rng, 100)
    good0[0, 0], good0[64, 127], good0[3, 5], good0[40, 0] = -0.0, 255.0, 255.0, -0.0      # legal values
    frames, flagged = [good0, good1], [False, False]
    for v in (255.5, 256.0, -1.0, 1e20, np.nan, np.inf):
        for at in ((-1, -1), (0, 0)):
            f = sparse_rows(rng, 40)
            f[at] = v
            frames.append(f)
            flagged.append(True)
    frames.append(np.full((5, 128), np.nan, dtype=np.float32))
    flagged.append(True)
    return frames, flagged


def l2_edge_pairs(n_frames):
    """Every frame with the two integer frames, both ways; the integer frames with each other; some flagged frames with each other."""
    ab = [(0, 1), (1, 0)]
    for f in range(2, n_frames):
        ab += [(f, 0), (0, f), (f, 1), (1, f)]
    return ab + [(f, f + 1) for f in range(2, n_frames - 1)] + [(n_frames - 1, n_frames - 1), (8, 8)]


def hamming_extreme_frames():
    """Frames of 129, 300, 1, 1 and 129 rows for the FP4 path: all zeros, all ones, one bit, 255 bits at rows 0, 31, 32, 63, 64, 127
    and at the last row; the same row in both lane halves of a block and in two blocks; frame 4 = frame 0's exact complements."""
    rng = np.random.default_rng(44)
    zeros, ones = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)

    def one_bit(k):
        r = zeros.copy()
        r[k >> 3] = 1 << (k & 7)
        return r

    x, y = rng.integers(0, 256, (129, 32), dtype=np.uint8), rng.integers(0, 256, (300, 32), dtype=np.uint8)
    for row, v in ((0, zeros), (31, ones), (32, one_bit(9)), (63, ~one_bit(9)), (64, zeros), (127, ones), (128, one_bit(255))):
        x[row] = v
    for row, v in ((0, ones), (31, zeros), (32, ~one_bit(0)), (63, one_bit(200)), (64, ~x[10]), (127, zeros), (299, ones)):
        y[row] = v
    y[3] = y[4] = x[5]          # rows 3 (lane half 0) and 4 (lane half 1) of one block: the lower wins
    y[36] = y[100] = x[6]       # blocks 1 and 3
    y[270] = y[45] = x[7]       # lane half 1 of block 1 against half 0 of block 8
    x[40] = x[12] = y[200]      # and with the 300-row frame as the query side
    return [x, y, ones[None, :].copy(), zeros[None, :].copy(), ~x]
