"""The header-only C++ shim (sfm-gms_amd/include/mi355_gms.hpp) with the reference's matchGMS signature.
CPU: it compiles and links against libgms_hip.so and fails loudly without a device. GPU: same data
through the oracle, same survivors."""
import os

import numpy as np
import pytest

import hostbuild as hb


def _lcg_data():
    s = np.uint64(12345)
    def lcg():
        nonlocal s
        s = (s * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
        return int(s) >> 8
    w, h, n = 1280, 720, 4000
    xy1 = np.zeros((n, 2), dtype=np.float32)
    xy2 = np.zeros((n, 2), dtype=np.float32)
    q, t, img = (np.zeros(n, dtype=np.int32) for _ in range(3))
    dist = np.zeros(n, dtype=np.float32)
    for i in range(n):
        xy1[i, 0] = np.float32(lcg() % ((w - 1) * 16)) / np.float32(16.0)
        xy1[i, 1] = np.float32(lcg() % ((h - 1) * 16)) / np.float32(16.0)
        xy2[i, 0] = xy1[i, 0] * np.float32(0.98) + np.float32(7.25)
        xy2[i, 1] = xy1[i, 1] * np.float32(0.98) + np.float32(3.5)
        q[i] = i
        t[i] = i if (lcg() % 100 < 55) else lcg() % n
        img[i] = i % 3
        dist[i] = np.float32(lcg() % 1024) / np.float32(4.0)
    return (w, h), xy1, xy2, q, t, img, dist


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this box has a GPU")
def test_shim_compiles_links_and_fails_loudly_without_gpu():
    exe = hb.shim_exe("shim_main.cpp")
    res = hb.run(exe)
    assert res.returncode == 3 and "no usable HIP device" in res.stderr


@pytest.mark.gpu
def test_shim_matches_oracle(oracle, pkg, synth):
    exe = hb.shim_exe("shim_main.cpp")
    res = hb.run(exe, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split()
    size, xy1, xy2, q, t, img, dist = _lcg_data()
    m = np.zeros(len(q), dtype=pkg.DMATCH_DTYPE)
    m["queryIdx"], m["trainIdx"], m["imgIdx"], m["distance"] = q, t, img, dist
    for k, flags in enumerate(((False, False), (True, True))):
        rc, want, _, _ = oracle.match(size, size, synth.make_keypoints(xy1), synth.make_keypoints(xy2), m, *flags, 6.0)
        assert rc == 0 and len(want) > 500
        assert (int(lines[2 * k]), int(lines[2 * k + 1])) == (len(want), hb.fnv1a(want.tobytes(), words=True))
    # the batch form (matchGMSBatch -> gms_filter_host_batch): the pair, an empty pair, the first half of the pair's matches
    kp1, kp2 = synth.make_keypoints(xy1), synth.make_keypoints(xy2)
    for p, mm in enumerate((m, m[:0], m[: len(m) // 2])):
        rc, want, _, _ = oracle.match(size, size, kp1, kp2, mm, True, True, 6.0)
        assert rc == 0
        assert [int(x) for x in lines[4 + 3 * p: 7 + 3 * p]] == [len(want), hb.fnv1a(want.tobytes(), words=True), 1]
