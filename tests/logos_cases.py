"""The named cases of the LOGOS tests at the edges of its domain (tests/test_logos_cases.py on the CPU, tests/test_gpu_logos_limits.py
on the GPU). A case is a dict: name, frames (float32 [n, 4] arrays of x, y, size, angle), words (int32 [n] arrays), n_words, and
pairs: (frame_a, frame_b) indices into frames. Everything is seeded and read-only; sizes are the smallest that reach the regime the
case is named for. expected() is the statement tests/logos_ref.py of a pair, computed once per session.

Every angle here lies inside the keypoint domain (|angle| <= 3600 degrees, include/gms.h) except in domain_refusals(), which holds
only values at which the unguarded wrap loop of logos_core.h rel_ori still ends within 11 rounds (or is skipped: NaN, inf). No case
holds a finite |angle| > 1e5: those are passed to the library by tests/test_logos_cases.py alone, without a device."""
import functools

import numpy as np


def _ro(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def _case(name, frames, words, n_words, pairs):
    frames = tuple(_ro(np.asarray(f, np.float32).reshape(-1, 4), np.float32) for f in frames)
    words = tuple(_ro(np.asarray(w).reshape(-1), np.int32) for w in words)
    assert len(frames) == len(words) and all(len(f) == len(w) for f, w in zip(frames, words))
    assert all(((w >= 0) & (w < n_words)).all() for w in words)
    return dict(name=name, frames=frames, words=words, n_words=int(n_words), pairs=tuple((int(a), int(b)) for a, b in pairs))


def moved(kp, theta, scale, t=(3.0, -2.0)):
    """kp under a similarity: rotated by theta, scaled, shifted; sizes scaled, angles turned back by theta (mod 360)."""
    kp = np.asarray(kp, np.float64).reshape(-1, 4)
    c, s = np.cos(theta), np.sin(theta)
    out = kp.copy()
    out[:, 0] = scale * (c * kp[:, 0] - s * kp[:, 1]) + t[0]
    out[:, 1] = scale * (s * kp[:, 0] + c * kp[:, 1]) + t[1]
    out[:, 2] = kp[:, 2] * scale
    out[:, 3] = np.mod(kp[:, 3] - np.degrees(theta), 360.0)
    return out.astype(np.float32)


def random_frame(rng, n, w=640.0, h=480.0, integer=False):
    if integer:   # distinct sites of the integer lattice: equal distances, no coincident points
        cell = rng.choice(int(w) * int(h), n, replace=False)
        xy = np.stack([cell % int(w), cell // int(w)], 1)
    else:
        xy = rng.uniform(0, (w, h), (n, 2))
    return np.concatenate([xy, rng.uniform(2, 20, (n, 1)), rng.uniform(0, 360, (n, 1))], 1).astype(np.float32)


def tiny():
    """Frames 2 k - 2 and 2 k - 1 (k = 1..8): a random frame of k keypoints and its copy moved by 0.3 rad and scale 1.2, words in
    {0, 1}; frame 16: 40 keypoints. Pairs (k, k) in both orders and (k, 40), (40, k). -1 neighbour pads, kk = n - 1 in the k-NN
    kernels, and at k = 7 and 8 neighbour lists of 6 and 7 records."""
    rng = np.random.default_rng(8101)
    frames, words, pairs = [], [], []
    for k in range(1, 9):
        a = random_frame(rng, k, 200.0, 150.0)
        w = np.arange(k) % 2
        frames += [a, moved(a, 0.3, 1.2)]
        words += [w, w]
        pairs += [(2 * k - 2, 2 * k - 1), (2 * k - 1, 2 * k - 2), (2 * k - 2, 16), (16, 2 * k - 2)]
    frames.append(random_frame(rng, 40, 200.0, 150.0))
    words.append(rng.integers(0, 2, 40))
    return _case("tiny", frames, words, 2, pairs)


EMPTY_TABLE_COUNTS = (0, 300, 0, 1, 5, 6, 7, 256, 257, 0)


def empty_in_table():
    """One table with empty frames first, in the middle and last; every (a, b) over its ten frames. Frames 7 and 8 are moved copies of
    frame 1's first 256 and 257 keypoints, so the large pairs have survivors."""
    rng = np.random.default_rng(8102)
    big = random_frame(rng, 300)
    wbig = rng.integers(0, 4, 300)
    frames, words = [], []
    for f, n in enumerate(EMPTY_TABLE_COUNTS):
        if n == 300:
            frames.append(big)
            words.append(wbig)
        elif n >= 256:
            frames.append(moved(big[:n], -0.25, 0.9))
            words.append(wbig[:n])
        else:
            frames.append(random_frame(rng, n))
            words.append(rng.integers(0, 4, n))
    return _case("empty_in_table", frames, words, 4, [(a, b) for a in range(10) for b in range(10)])


def coincident(n):
    """n copies of one keypoint, one word: every distance is 0. 6: no tie (five others); 7: a tie list sorted with m = 6; 40: the
    sort's partition on equal records; 300: two LDS tiles. Every candidate's geometry is 0 / 0."""
    f = np.tile(np.float32([[17.0, 23.0, 5.0, 30.0]]), (n, 1))
    return _case(f"coincident_{n}", [f], [np.zeros(n, np.int32)], 1, [(0, 0)])


def triples_on_lattice():
    """A 12 x 12 lattice of pitch 9 x 7 with three coincident keypoints per site (each with its own size and angle) and one word per
    site out of four, against its copy moved by 0.4 rad and scale 1.1: every point has two coincident neighbours (NaN geometry) and
    takes three of the six tied points of its two nearest sites."""
    rng = np.random.default_rng(8104)
    gy, gx = np.mgrid[0:12, 0:12]
    sx, sy = np.repeat(9.0 * gx.reshape(-1), 3), np.repeat(7.0 * gy.reshape(-1), 3)
    a = np.stack([sx, sy, rng.uniform(2, 20, 432), rng.uniform(0, 360, 432)], 1).astype(np.float32)
    w = np.repeat(rng.integers(0, 4, 144), 3)
    return _case("triples_on_lattice", [a, moved(a, 0.4, 1.1)], [w, w], 4, [(0, 1), (1, 0), (0, 0)])


LIMIT_ANGLES = (-1.0, 0.0, 360.0, 359.99997, 180.0, -180.0, 3600.0, -3600.0, 540.0, -539.5)
LIMIT_SIZES = (0.0, 1e-40, 3.4e38, -1.0, np.nan, np.inf)


def value_limits():
    """Frames 0, 1: 400 random keypoints and their moved copy, words in 0..5 (the clean pair). Frames 2, 3: the same with the angles of
    LIMIT_ANGLES on scattered keypoints of both frames (each frame its own), a run of 60 keypoints with angle -1 in both frames,
    and the sizes of LIMIT_SIZES on scattered keypoints of both."""
    rng = np.random.default_rng(8105)
    a = random_frame(rng, 400)
    b = moved(a, 0.5, 1.15)
    w = rng.integers(0, 6, 400)
    la, lb = a.copy(), b.copy()
    for f, fr in enumerate((la, lb)):
        spots = rng.choice(np.arange(60, 400), 4 * len(LIMIT_ANGLES), replace=False)
        fr[spots, 3] = np.tile(np.float32(LIMIT_ANGLES), 4)
        spots = rng.choice(np.arange(60, 400), 3 * len(LIMIT_SIZES), replace=False)
        with np.errstate(over="ignore"):
            fr[spots, 2] = np.tile(np.float32(LIMIT_SIZES), 3)
        fr[:60, 3] = -1.0
    return _case("value_limits", [a, b, la, lb], [w] * 4, 6, [(0, 1), (2, 3), (3, 2), (2, 2)])


WORD_EDGES = (1, 63, 64, 65, 128, 129, 300)


def word_edges(n_words):
    """prep_sort_kernel at the 64-lane chunk edges of n_words: a 300-keypoint pair (a frame and its moved copy) three times, with
    words drawn uniformly, all equal to n_words - 1, and only 0 and n_words - 1."""
    rng = np.random.default_rng(8200 + n_words)
    frames, words, pairs = [], [], []
    for v in range(3):
        a = random_frame(rng, 300)
        w = (rng.integers(0, n_words, 300), np.full(300, n_words - 1), rng.integers(0, 2, 300) * (n_words - 1))[v]
        frames += [a, moved(a, -0.35, 1.1)]
        words += [w, w]
        pairs += [(2 * v, 2 * v + 1), (2 * v + 1, 2 * v)]
    return _case(f"word_edges_{n_words}", frames, words, n_words, pairs)


def scan_edges():
    """n1 = 1023, 1024, 1025 queries against 300 keypoints, words in 0..3: the one-shot scan's `per` goes from 1 to 2 there. The
    train frame is the moved copy of the first 300 queries; the other queries lie apart, so those 300 keep their neighbours."""
    rng = np.random.default_rng(8107)
    big = random_frame(rng, 1025)
    big[300:, 0] += np.float32(2000.0)
    w = rng.integers(0, 4, 1025)
    frames = [big[:1023], big[:1024], big, moved(big[:300], 0.2, 1.05)]
    return _case("scan_edges", frames, [w[:1023], w[:1024], w, w[:300]], 4, [(0, 3), (1, 3), (2, 3)])


def tile_edges():
    """n = 256 (one full LDS tile of the k-NN kernels) and 257 (one more point), in either position. Frames 0..3: float coordinates
    and their moved copies, no ties. Frames 4..7: an integer lattice, with ties, and its moved copy, without: of the two tie
    launches of the one-shot only one runs."""
    rng = np.random.default_rng(8108)
    frames, words, pairs = [], [], []
    for integer in (False, True):
        for n in (256, 257):
            a = random_frame(rng, n, 40.0, 30.0, integer) if integer else random_frame(rng, n)
            w = rng.integers(0, 4, n)
            k = len(frames)
            b = moved(a, 0.3, 1.2)
            if integer:   # a turned lattice keeps some of its equal distances: a hundredth of a pixel of jitter leaves none
                b[:, :2] += rng.uniform(-0.01, 0.01, (n, 2)).astype(np.float32)
            frames += [a, b]
            words += [w, w]
            pairs += [(k, k + 1), (k + 1, k)]
    return _case("tile_edges", frames, words, 4, pairs)


@functools.lru_cache(maxsize=None)
def all_cases():
    return ((tiny(), empty_in_table()) + tuple(coincident(n) for n in (6, 7, 40, 300)) + (triples_on_lattice(), value_limits())
            + tuple(word_edges(n) for n in WORD_EDGES) + (scan_edges(), tile_edges()))


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected(name, a, b):
    """The statement's ((m, 2) int32 survivors, (n_candidates, n_supported, peak_bin)) of pair (a, b) of a named case; read-only."""
    import logos_ref
    c = case(name)
    with np.errstate(all="ignore"):   # sizes of 0, NaN and inf are part of the cases
        res, detail = logos_ref.match(c["frames"][a], c["frames"][b], c["words"][a], c["words"][b], detail=True)
    res.setflags(write=False)
    return res, detail


# the only out-of-domain values a GPU test may use: the unguarded wrap loop ends within 11 rounds at the finite ones
REFUSED = (("angle", 3600.5), ("angle", -3601.0), ("angle", np.nan), ("angle", np.inf), ("x", np.inf))


def domain_refusals():
    """Six frames of 50 keypoints: frame f < 5 holds REFUSED[f] on one keypoint; frame 5 is clean. Every (a, b) over them."""
    rng = np.random.default_rng(8109)
    base = random_frame(rng, 50)
    w = rng.integers(0, 3, 50)
    frames = []
    for f, (field, v) in enumerate(REFUSED):
        fr = moved(base, 0.1 * f, 1.0)
        fr[7 * f + 3, {"x": 0, "angle": 3}[field]] = v
        frames.append(fr)
    frames.append(base)
    return _case("domain_refusals", frames, [w] * 6, 3, [(a, b) for a in range(6) for b in range(6)])
