"""A numpy restatement of gms_logos_words_device (include/gms.h): the exact nearest dictionary row of every
descriptor row, lowest index on ties.

L2 (rows of 128 float32): the squared distance is accumulated in float32 in flann::L2<float>'s order -- per group of four
dimensions ((d0*d0 + d1*d1) + d2*d2) + d3*d3, the groups added to the running sum in order, no fused multiply-add. A NaN distance
counts as +inf. Hamming (rows of 32 bytes): popcount of the xor."""
import numpy as np


def l2_distances(desc, dictionary, chunk=2048):
    """[n, k] float32 squared distances in the definition's order."""
    desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
    dic = np.ascontiguousarray(dictionary, np.float32).reshape(-1, 128)
    out = np.empty((len(desc), len(dic)), np.float32)
    for s in range(0, len(desc), chunk):
        d = desc[s:s + chunk, None, :] - dic[None, :, :]          # float32
        sq = d * d                                                 # rounded per product
        grp = ((sq[..., 0::4] + sq[..., 1::4]) + sq[..., 2::4]) + sq[..., 3::4]
        acc = np.zeros(grp.shape[:2], np.float32)
        for g in range(32):
            acc = acc + grp[..., g]
        out[s:s + chunk] = acc
    return out


def hamming_distances(desc, dictionary):
    a = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(dictionary, np.uint8).reshape(-1, 32)
    x = np.bitwise_xor(a[:, None, :], b[None, :, :])
    return np.unpackbits(x, axis=2).sum(2).astype(np.float32)


def words(desc, dictionary, kind):
    """kind 1 = GMS_DESC_L2_F32X128, 0 = GMS_DESC_HAMMING256 -> int32 word per row (np.argmin keeps the first minimum)."""
    d = l2_distances(desc, dictionary) if kind == 1 else hamming_distances(desc, dictionary)
    d = np.where(np.isnan(d), np.float32(np.inf), d)
    return np.argmin(d, axis=1).astype(np.int32) if d.shape[1] else np.zeros(len(d), np.int32)
