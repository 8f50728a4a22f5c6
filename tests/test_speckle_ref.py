"""The two numpy statements of the speckle filter (tests/speckle_ref.py) against each other and against a g++ build of the header the
kernels compile (sfm-gms_amd/csrc/speckle_core.h through the stand-alone program tests/cpp/speckle_host.cpp), byte for byte, plain and
under sanitizers; that each case of tests/speckle_cases.py holds what it is named for; idempotence; the workspace's layout; and the
arguments that are refused. The host program never runs inside Python: cases go to it as files."""

import numpy as np
import pytest

import speckle_cases as sc
import speckle_ref as sr
import hostbuild as hb

SRC = "speckle_host.cpp"
NAMES = {"plus_on_lattice_131x67", "plus_on_lattice_135x71", "serpentine_70x40", "serpentine_259x131", "constant", "singletons", "ramp_exact",
         "ramp_one_more", "extremes", "diagonal_only", "new_val_inside", "thin_1x1", "thin_1x300", "thin_300x1", "thin_8192x1",
         "random_blobs_131x67", "random_blobs_259x131"}


def runs():
    return [(c, k) for c in sc.all_cases() for k in range(len(c["runs"]))]


def run_host(exe, disp, new_val, size, diff, tmp_path, tag):
    src, dst = tmp_path / (tag + ".in"), tmp_path / (tag + ".out")
    src.write_bytes(sc.case_bytes(disp, new_val, size, diff))
    res = hb.run(exe, src, dst)
    return res.returncode, (dst.read_bytes() if res.returncode == 0 else res.stderr)


@pytest.fixture(scope="module")
def host_exe():
    exe = hb.host_exe(SRC)
    return exe


def test_the_cases_are_all_there():
    assert {c["name"] for c in sc.all_cases()} == NAMES
    for c in sc.all_cases():
        w, h = c["disp"].shape[1], c["disp"].shape[0]
        if not c["name"].startswith("thin") and c["name"] != "serpentine_70x40":
            assert w > 2 * 64 and h > 2 * 32, c["name"]          # at least 3 x 3 tiles of 64 x 32
    assert sc.all_cases()[2]["disp"].shape == (40, 70)           # 2 x 2 tiles


def test_literal_equals_components_on_every_case():
    for c, k in runs():
        size, diff, _ = c["runs"][k]
        want, n_want = sc.expected(c["name"], k)
        got, n_got = sr.components(c["disp"], c["new_val"], size, diff)
        assert n_got == n_want and got.tobytes() == want.tobytes(), (c["name"], k)


def test_every_case_holds_what_it_is_named_for():
    for c, k in runs():
        size, diff, stated = c["runs"][k]
        out, removed = sc.expected(c["name"], k)
        changed = out != c["disp"]
        assert removed == int(changed.sum()) and (out[changed] == c["new_val"]).all(), (c["name"], k)
        assert (out[c["disp"] == c["new_val"]] == c["new_val"]).all(), (c["name"], k)      # new_val pixels never change
        if stated is not None:
            assert removed == stated, (c["name"], k, removed, stated)
    rb = next(c for c in sc.all_cases() if c["name"] == "random_blobs_131x67")
    assert 0 < sc.expected(rb["name"], 0)[1] < int((rb["disp"] != rb["new_val"]).sum())     # the seeded maps lose some pixels, not all
    assert 0 < sc.expected(rb["name"], 1)[1]


def test_component_structure_of_the_named_cases():
    by = {c["name"]: c for c in sc.all_cases()}

    def sizes(name, diff):
        lab = sr.component_labels(by[name]["disp"], by[name]["new_val"], diff)
        return sorted(np.bincount(lab[lab >= 0])[np.unique(lab[lab >= 0])].tolist())

    assert sizes("plus_on_lattice_135x71", 0) == [13] * 32 and sizes("plus_on_lattice_131x67", 0) == [13] * 21
    assert sizes("serpentine_259x131", 0) == [66 * 259 + 65] and sizes("constant", 0) == [131 * 67]
    assert sizes("singletons", 99) == [1] * (131 * 67) and sizes("singletons", 100) == [131 * 67]
    assert sizes("ramp_exact", 5) == [131] * 67 and sizes("ramp_exact", 4) == [1] * (131 * 67) and sizes("ramp_one_more", 5) == [1] * (131 * 67)
    assert sizes("extremes", 65535) == [131 * 67] and sizes("extremes", 65534) == [1] * (131 * 67)
    assert sizes("diagonal_only", 0) == [25] * 4
    assert sizes("new_val_inside", 2) == [8, 280, 300] and sizes("new_val_inside", 1) == [4, 4, 280, 300]
    d = by["ramp_exact"]["disp"]
    assert int(d[0, -1]) - int(d[0, 0]) == 650                # linked by transitivity although the ends differ by far more than 5


def test_idempotence():
    for c, k in runs():
        size, diff, _ = c["runs"][k]
        once, _ = sc.expected(c["name"], k)
        twice, n = sr.components(once, c["new_val"], size, diff)
        assert n == 0 and twice.tobytes() == once.tobytes(), (c["name"], k)


def test_host_build_equals_statement(host_exe, tmp_path):
    for c, k in runs():
        size, diff, _ = c["runs"][k]
        rc, got = run_host(host_exe, c["disp"], c["new_val"], size, diff, tmp_path, f"{c['name']}_{k}")
        assert rc == 0 and got == sc.result_bytes(*sc.expected(c["name"], k)), (c["name"], k)


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = hb.host_exe_sanitized(SRC)
    for c, k in runs():
        size, diff, _ = c["runs"][k]
        rc, got = run_host(exe, c["disp"], c["new_val"], size, diff, tmp_path, f"{c['name']}_{k}")
        assert rc == 0 and got == sc.result_bytes(*sc.expected(c["name"], k)), (c["name"], k, got if rc else "")


def test_layout():
    res = hb.run(hb.host_exe("speckle_layout_check.cpp"))
    assert res.returncode == 0 and res.stdout.strip() == "speckle_layout: ok", res.stdout


BAD = [dict(new_val=32768), dict(new_val=-32769), dict(size=-1), dict(diff=-1)]


def test_bad_arguments_are_refused(pkg, host_exe, tmp_path):
    """By the statements, by the host program (spk::args_ok: exit 2), and by the C ABI before anything touches a device."""
    d = np.zeros((3, 4), np.int16)
    for i, bad in enumerate(BAD):
        nv, size, diff = bad.get("new_val", 0), bad.get("size", 1), bad.get("diff", 1)
        for f in (sr.literal, sr.components):
            with pytest.raises(ValueError):
                f(d, nv, size, diff)
        assert run_host(host_exe, d, nv, size, diff, tmp_path, f"bad{i}")[0] == 2
        with pytest.raises(pkg.GmsError) as e:
            pkg.filterSpeckles(d, nv, size, diff)
        assert e.value.code == -1
    for f in (sr.literal, sr.components):
        with pytest.raises(ValueError):
            f(d.astype(np.int32), 0, 1, 1)
    for args in ((2 ** 32 + 1, 1, 1), (0, 2 ** 31, 1), (0, 1, 2 ** 31)):       # would wrap to acceptable values in 32 bits
        with pytest.raises(pkg.GmsError):
            pkg.filterSpeckles(d, *args)
    for shape in ((3,), (2, 3, 4), (0, 4)):
        with pytest.raises(ValueError):
            pkg.filterSpeckles(np.zeros(shape, np.int16), 0, 1, 1)
    with pytest.raises(ValueError):
        pkg.filterSpeckles(d.astype(np.uint8), 0, 1, 1)
    lib = pkg.load_library()
    assert lib.gms_filter_speckles_workspace_bytes(131, 67, 3) >= 8 * 131 * 67 * 3
    for w, h, n in ((0, 5, 1), (5, 0, 1), (8193, 5, 1), (5, 8193, 1), (5, 5, 0), (5, 5, 65536), (-1, 5, 1)):
        assert lib.gms_filter_speckles_workspace_bytes(w, h, n) == 0, (w, h, n)
    assert lib.gms_filter_speckles(None, 4, 3, 0, 1, 1, None) == -1
    assert lib.gms_filter_speckles(d.ctypes.data, 8193, 3, 0, 1, 1, None) == -1
    assert lib.gms_dense_pairs_filtered_workspace_bytes(96, 72, 1, 96, 72, 1, None) > lib.gms_dense_pairs_workspace_bytes(96, 72, 1, 96, 72, 1, None) > 0
    assert lib.gms_dense_pairs_filtered_workspace_bytes(96, 72, 2, 96, 72, 1, None) == 0
