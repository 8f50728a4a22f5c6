"""CPU: the numpy restatement of gms_logos_words_device (tests/logos_words_ref.py) and the host-side surface of the batched LOGOS
path -- the built library exports its entry points and sizes its buffers without a device."""
import numpy as np
import pytest

import logos_words_ref

NEW_SYMBOLS = ["gms_logos_table_bytes", "gms_logos_workspace_bytes", "gms_logos_prepare_device", "gms_logos_filter_device",
               "gms_logos_words_device", "gms_logos_host_batch"]


@pytest.mark.parametrize("n_words", [1, 7, 50, 100])
def test_l2_restatement_agrees_with_float64_argmin(n_words):
    rng = np.random.default_rng(n_words)
    dic = rng.uniform(0, 255, (n_words, 128)).astype(np.float32)
    pick = rng.integers(0, n_words, 3000)
    desc = (dic[pick] + rng.normal(0, 2.0, (3000, 128))).astype(np.float32)     # well separated: words lie ~1000 apart
    d64 = ((desc.astype(np.float64)[:, None, :] - dic.astype(np.float64)[None]) ** 2).sum(2)
    got = logos_words_ref.words(desc, dic, 1)
    assert (got == np.argmin(d64, 1)).all()
    assert (got == pick).all() or n_words > 1 and (dic[got] == dic[pick]).all()


def test_l2_restatement_is_the_sequential_order():
    """The distance is the running fp32 sum of four-element groups, which is not numpy's pairwise sum."""
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, (200, 128)).astype(np.float32) * np.float32(1e3)
    b = rng.uniform(-1, 1, (5, 128)).astype(np.float32)
    d = logos_words_ref.l2_distances(a, b)
    for r in range(0, 200, 37):
        for w in range(5):
            diff = a[r] - b[w]
            acc = np.float32(0)
            for g in range(0, 128, 4):
                s = [np.float32(diff[g + k]) * np.float32(diff[g + k]) for k in range(4)]
                acc = np.float32(acc + np.float32(np.float32(np.float32(s[0] + s[1]) + s[2]) + s[3]))
            assert d[r, w] == acc


def test_ties_nan_and_duplicates():
    dic = np.zeros((4, 128), np.float32)
    dic[1] = 1.0
    dic[3] = 1.0                       # duplicate of row 1
    desc = np.ones((3, 128), np.float32)
    desc[1] = 0.5                       # equidistant from rows 0/2 and 1/3
    desc[2, 5] = np.nan                 # every distance NaN -> +inf -> word 0
    assert logos_words_ref.words(desc, dic, 1).tolist() == [1, 0, 0]


def test_hamming_restatement():
    rng = np.random.default_rng(5)
    dic = rng.integers(0, 256, (60, 32)).astype(np.uint8)
    desc = rng.integers(0, 256, (500, 32)).astype(np.uint8)
    pop = np.array([bin(v).count("1") for v in range(256)])
    want = np.array([np.argmin([pop[np.bitwise_xor(d, w)].sum() for w in dic]) for d in desc])
    assert (logos_words_ref.words(desc, dic, 0) == want).all()


def test_library_exports_and_sizes(pkg):
    for s in NEW_SYMBOLS:
        assert s in pkg.EXPORTED_SYMBOLS
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert lib.gms_logos_table_bytes(1000, 4, 50) > 1000 * (16 + 4 + 20 + 4 + 4) + 4 * 51 * 4
    assert lib.gms_logos_table_bytes(10, 1, 0) == 0 and lib.gms_logos_table_bytes(10, 1, 65536) == 0
    assert lib.gms_logos_table_bytes(-1, 1, 50) == 0
    assert lib.gms_logos_workspace_bytes(10000, 10, 10000) >= 10 * 10000 * 8
    assert lib.gms_logos_workspace_bytes(-1, 0, 0) == 0
    assert pkg.LOGOS_RESULT_DTYPE.itemsize == 32
    # argument checks come before any device work
    assert lib.gms_logos_words_device(None, 1, None, 0, None, 50, None) == -1
    assert lib.gms_logos_filter_device(None, None, None, 1, None, 0, None, None, None) == -1
