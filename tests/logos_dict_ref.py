"""A numpy statement of gms_logos_dict_train_device (include/gms.h, DESIGN.md §6b "Training the dictionary"): k-means of descriptor
rows with k-means++ seeding, every order-dependent step in integers, so that the GPU gives these bytes on every run.

Distances are those of the words call (tests/logos_words_ref.py): L2 is the fp32 squared distance in flann::L2's grouping, no fused
multiply-add; Hamming the popcount of the xor; nearest = lowest index on ties. Weights: a Hamming distance is its own weight, an L2
distance d weighs floor(d * 2**8) (uint64). Draws: u(seed, set, attempt, centre, trial) =
sm(sm(sm(sm(sm(seed) + set) + attempt) + centre) + trial) with sm = splitmix64's output function of (z + golden gamma), all mod 2**64;
mulhi64(u, n) = (u * n) >> 64.

Per attempt: centre 0 is row mulhi64(u(.., 0, 0), n). Centre c >= 1: with w_i the minimum weight of row i to the centres so far and
W their sum, trial t = 0, 1, 2 proposes the first row whose inclusive prefix sum of w exceeds mulhi64(u(.., c, t), W) -- row
mulhi64(u(.., c, t), n) when W = 0 -- and the candidate under which sum_i min(w_i, weight(i, candidate)) is smallest is kept (lowest t
on ties). Then at most max_iters assignments: label every row; stop if no label changed (the first assignment always counts as a
change); unless it was the last assignment allowed, move every centre: L2 to (float)((double)S / ((double)count * 2**20)) with S the
exact sum of rint(x * 2**20) over its rows, Hamming to the per-bit majority (1 iff 2 * ones > count); a centre without rows stays.
The attempt whose last assignment has the smallest sum of weights (compactness) wins, lowest index on ties. So the labels returned are
the words of the rows under the dictionary returned."""
import numpy as np

import logos_words_ref

M64 = (1 << 64) - 1
GMS_OK, GMS_ERR_BAD_ARG, GMS_ERR_DOMAIN = 0, -1, -2
HAMMING, L2 = 0, 1
MAX_SET_ROWS = 1 << 20
MAX_ABS = 4096.0
DICT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("attempt", "<i4"), ("iterations", "<i4"), ("empty_clusters", "<i4"),
                              ("compactness", "<u8")])


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, set_index, attempt, centre, trial):
    z = splitmix64(seed & M64)
    for v in (set_index, attempt, centre, trial):
        z = splitmix64((z + v) & M64)
    return z


def mulhi64(a, b):
    return (int(a) * int(b)) >> 64


def _rows(desc, kind):
    return (np.ascontiguousarray(desc, np.uint8).reshape(-1, 32) if kind == HAMMING
            else np.ascontiguousarray(desc, np.float32).reshape(-1, 128))


_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def hamming_distances(rows, centres, chunk=4096):
    """logos_words_ref.hamming_distances by a byte table (the same values, faster on large sets)."""
    a, b = _rows(rows, HAMMING), _rows(centres, HAMMING)
    out = np.empty((len(a), len(b)), np.float32)
    for s in range(0, len(a), chunk):
        out[s:s + chunk] = _POPCOUNT[a[s:s + chunk, None, :] ^ b[None, :, :]].sum(2, dtype=np.int32)
    return out


def distances(rows, centres, kind):
    """[n, k] float32 distances of the words call."""
    return logos_words_ref.l2_distances(rows, centres) if kind == L2 else hamming_distances(rows, centres)


def weights(d, kind):
    """uint64 weights of float32 distances."""
    d = np.asarray(d, np.float32)
    return np.floor(d * np.float32(256.0)).astype(np.uint64) if kind == L2 else d.astype(np.uint64)


def quantise(x):
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * 1048576.0).astype(np.int64)


def l2_mean(sum_q, count):
    return (np.asarray(sum_q, np.int64).astype(np.float64) / (np.float64(count) * 1048576.0)).astype(np.float32)


def seed_centres(rows, kind, n_words, seed, set_index, attempt, trace=None):
    """The row index of every centre of one attempt (k-means++, three trials per centre)."""
    n = len(rows)
    chosen = [mulhi64(draw(seed, set_index, attempt, 0, 0), n)]
    w = None
    for c in range(1, n_words):
        wc = weights(distances(rows, rows[chosen[-1]:chosen[-1] + 1], kind)[:, 0], kind)
        w = wc if w is None else np.minimum(w, wc)
        prefix = np.cumsum(w, dtype=np.uint64)
        total = int(prefix[-1])
        cands = []
        for t in range(3):
            u = draw(seed, set_index, attempt, c, t)
            if total == 0:
                cands.append(mulhi64(u, n))
            else:
                cands.append(int(np.searchsorted(prefix, np.uint64(mulhi64(u, total)), side="right")))
        wt = weights(distances(rows, rows[cands], kind), kind)
        pots = [int(np.minimum(w, wt[:, t]).sum(dtype=np.uint64)) for t in range(3)]
        best = int(np.argmin(pots))   # np.argmin keeps the first minimum
        if trace is not None:
            trace.append({"centre": c, "total": total, "candidates": cands, "potentials": pots, "kept": best})
        chosen.append(cands[best])
    return chosen


def assign(rows, centres, kind):
    d = distances(rows, centres, kind)
    labels = np.argmin(d, axis=1).astype(np.int32)
    w = weights(d[np.arange(len(rows)), labels], kind)
    return labels, w


def update(rows, labels, centres, kind):
    new = centres.copy()
    for c in range(len(centres)):
        members = rows[labels == c]
        if len(members) == 0:
            continue
        if kind == L2:
            new[c] = l2_mean(quantise(members).sum(axis=0, dtype=np.int64), len(members))
        else:
            ones = np.unpackbits(members, axis=1, bitorder="little").sum(axis=0, dtype=np.int64)
            new[c] = np.packbits(2 * ones > len(members), bitorder="little")
    return new


def run_attempt(rows, kind, n_words, max_iters, seed, set_index, attempt):
    """-> dict(centres, labels, iterations, compactness, seed_compactness, seed_rows)"""
    seed_rows = seed_centres(rows, kind, n_words, seed, set_index, attempt)
    centres = rows[seed_rows].copy()
    labels = None
    seed_comp = None
    for it in range(max_iters):
        new, w = assign(rows, centres, kind)
        comp = int(w.sum(dtype=np.uint64))
        if it == 0:
            seed_comp = comp
        changed = labels is None or bool(np.any(new != labels))
        labels = new
        if not changed:
            break
        if it + 1 < max_iters:
            centres = update(rows, labels, centres, kind)
    return {"centres": centres, "labels": labels, "iterations": it + 1, "compactness": comp, "seed_compactness": seed_comp,
            "seed_rows": seed_rows}


def set_status(rows, kind, n_words):
    if len(rows) < n_words or len(rows) > MAX_SET_ROWS:
        return GMS_ERR_BAD_ARG
    if kind == L2 and not bool(np.all(np.abs(rows) <= np.float32(MAX_ABS))):   # NaN and inf compare false
        return GMS_ERR_DOMAIN
    return GMS_OK


def train_set(rows, kind, n_words=50, attempts=3, max_iters=100, seed=0, set_index=0, detail=False):
    """One training set -> (dictionary, record, labels): what the call gives for set `set_index` of a batch."""
    rows = _rows(rows, kind)
    rec = np.zeros(1, DICT_RESULT_DTYPE)[0]
    status = set_status(rows, kind, n_words)
    if status != GMS_OK:
        rec["status"], rec["attempt"] = status, -1
        out = (np.zeros((n_words, rows.shape[1]), rows.dtype), rec, np.full(len(rows), -1, np.int32))
        return out + ([],) if detail else out
    runs = [run_attempt(rows, kind, n_words, max_iters, seed, set_index, a) for a in range(attempts)]
    win = int(np.argmin([r["compactness"] for r in runs]))
    r = runs[win]
    rec["status"], rec["attempt"], rec["iterations"], rec["compactness"] = GMS_OK, win, r["iterations"], r["compactness"]
    rec["empty_clusters"] = n_words - len(np.unique(r["labels"]))
    out = (r["centres"], rec, r["labels"])
    return out + (runs,) if detail else out


def train(desc, set_off, kind, n_words=50, attempts=3, max_iters=100, seed=0):
    """The batched call: rows [set_off[s], set_off[s + 1]) of desc are set s -> (dictionaries [n_sets, n_words, width], records,
    labels per row of desc; -1 where a set failed or a row belongs to no set). A set whose offsets are unusable -- negative, past
    the rows, end before start, or a start before the end of an earlier usable set -- gets GMS_ERR_BAD_ARG and touches no label."""
    desc = _rows(desc, kind)
    set_off = np.asarray(set_off, np.int64)
    n_sets = len(set_off) - 1
    dicts = np.zeros((n_sets, n_words, desc.shape[1]), desc.dtype)
    recs = np.zeros(n_sets, DICT_RESULT_DTYPE)
    labels = np.full(len(desc), -1, np.int32)
    end = 0   # of the sets with usable offsets so far: a set that starts before it is refused, so sets that run never overlap
    for s in range(n_sets):
        a, b = int(set_off[s]), int(set_off[s + 1])
        if a < 0 or b < a or b > len(desc) or a < end:
            recs[s]["status"], recs[s]["attempt"] = GMS_ERR_BAD_ARG, -1
            continue
        end = b
        dicts[s], recs[s], labels[a:b] = train_set(desc[a:b], kind, n_words, attempts, max_iters, seed, s)
    return dicts, recs, labels
