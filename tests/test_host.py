"""CPU: host-side logic -- the C-ABI library loads and exports what include/gms.h declares, the product
path fails loudly without a GPU, PODs have the reference's layout, sharding tiles the pair list, the
synthetic recipe is deterministic, and the N>1 driver logic works under gloo with world_size 2."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported(pkg):
    hdr = open(os.path.join(ROOT, "include", "gms.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gms_[a-z_0-9]+)\s*\(", hdr)))
    assert sorted(pkg.EXPORTED_SYMBOLS) == declared
    lib = pkg.load_library()  # no compute call: loading and symbol lookup work without a GPU
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.gms_version()
    assert lib.gms_max_matches() >= 10000
    assert lib.gms_error_string(-2).decode().startswith("input outside")


_C_CLASSES = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
              "double": C.c_double, "void": None}


def _c_class(decl, name, is_return=False):
    """The ctypes class a C parameter or return declaration stands for: "pointer" for a pointer or array, else the scalar's."""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w != "const"]
    if not is_return and len(words) == 2:
        words = words[:1]   # (the parameter's name)
    assert len(words) == 1 and words[0] in _C_CLASSES, f"{name}: cannot read {decl!r}"
    return _C_CLASSES[words[0]]


def _ctypes_class(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)) else t


def test_signature_table_matches_the_header(pkg):
    """Every prototype of include/gms.h against capi.SIGNATURES: the return type and the class of each parameter (pointer, int, int64,
    uint64, size_t, double). A prototype the parser cannot read fails."""
    capi = importlib.import_module("sfm-gms_amd.capi")
    hdr = open(os.path.join(ROOT, "include", "gms.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"^\s*#.*$", "", hdr, flags=re.M)                       # preprocessor lines
    hdr = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", "", hdr, flags=re.S)   # struct bodies hold no prototypes
    seen = {}
    for stmt in hdr.split(";"):
        if "gms_" not in stmt or "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(gms_[a-z_0-9]+)\s*\((.*)\)\s*", stmt, flags=re.S)
        assert m, f"cannot read the prototype {' '.join(stmt.split())!r}"
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        seen[name] = (_c_class(ret, name, is_return=True), [_c_class(p, name) for p in params])
    assert sorted(seen) == sorted(capi.SIGNATURES) == sorted(pkg.EXPORTED_SYMBOLS)
    for name, (ret, params) in seen.items():
        restype, argtypes = capi.SIGNATURES[name]
        assert _ctypes_class(restype) == ret, f"{name}: returns {restype}, the header says {ret}"
        assert [_ctypes_class(t) for t in argtypes] == params, f"{name}: {argtypes} against the header's {params}"
    lib = pkg.load_library()
    for name, (restype, argtypes) in capi.SIGNATURES.items():            # and the table is what the loaded library carries
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes, name


def test_detect_workspace_size_is_not_truncated(pkg):
    """gms_detect_workspace_bytes returns size_t: 300 images of 1920 x 1080 need more than 2^31 bytes (host arithmetic, no device).
    The size restates detect_kernels.hip: detect_workspace_bytes."""
    lib = pkg.load_library()
    w, h, n, max_kp = 1920, 1080, 300, 10000
    up = lambda b: (b + 255) & ~255
    plane = w * h
    want = up(plane * n) * 2 + up(plane * n * 2) + n * 256 * 4 + n * 16 + up(n * h * 8) + up(n * max_kp * 8)
    got = lib.gms_detect_workspace_bytes(w, h, n, max_kp)
    assert got > 2**31
    assert got == want
    assert lib.gms_detect_pyramid_workspace_bytes(w, h, n, max_kp, 1) >= got


def test_pod_layouts_match_reference_strides(pkg):
    assert pkg.KEYPOINT_DTYPE.itemsize == 0x1C and pkg.DMATCH_DTYPE.itemsize == 0x10
    assert pkg.KEYPOINT_DTYPE.fields["y"][1] == 4 and pkg.DMATCH_DTYPE.fields["trainIdx"][1] == 4
    assert pkg.PAIR_DTYPE.itemsize == 24 and pkg.PAIR_DTYPE.fields["match_off"][1] == 16


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this box has a GPU")
def test_product_path_fails_loudly_without_gpu(pkg, synth):
    """No CPU fallback: without a device the compute entry points return an error / raise."""
    lib = pkg.load_library()
    h = C.c_void_p()
    assert lib.gms_ctx_create(0, C.byref(h)) == -4  # GMS_ERR_NO_DEVICE
    kp1, kp2, m = synth.make_pair(1, size1=(640, 480), n1=50)
    with pytest.raises(pkg.GmsError):
        pkg.matchGMS((640, 480), (640, 480), kp1, kp2, m)
    out = np.zeros(50, dtype=pkg.DMATCH_DTYPE)
    n_out = C.c_int(123)
    rc = lib.gms_match(kp1.ctypes.data, 50, 640, 480, kp2.ctypes.data, 50, 640, 480, m.ctypes.data, 50, 0, 0, 6.0,
                       out.ctypes.data, C.byref(n_out))
    assert rc == -4 and n_out.value == 0


def test_missing_library_is_an_import_error(pkg, monkeypatch):
    capi = sys.modules["sfm-gms_amd.capi"]
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "library_path", lambda: "/nonexistent/libgms_hip.so")
    with pytest.raises(ImportError):
        capi.load_library()


def test_product_sources_never_touch_the_oracle():
    pkg_dir = os.path.join(ROOT, "sfm-gms_amd")
    for dirpath, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp")) or f == "Makefile":
                text = open(os.path.join(dirpath, f)).read()
                assert "gms_ref" not in text and "gms_oracle" not in text and "oracle/" not in text, f


def test_pair_indexing_and_shards(pkg):
    for n in (2, 3, 7, 50):
        total = pkg.all_pairs_count(n)
        seen = [pkg.pair_from_index(k, n) for k in range(total)]
        assert seen == [(a, b) for a in range(n) for b in range(a + 1, n)]
    assert pkg.all_pairs_count(1000) == 499500 and pkg.pair_from_index(499499, 1000) == (998, 999)
    with pytest.raises(IndexError):
        pkg.pair_from_index(3, 3)
    for n_items in (0, 1, 7, 4096, 499500):
        for world in (1, 2, 3, 8):
            cuts = [pkg.shard_range(n_items, r, world) for r in range(world)]
            assert cuts[0][0] == 0 and cuts[-1][1] == n_items
            assert all(cuts[i][1] == cuts[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in cuts]
            assert max(sizes) - min(sizes) <= 1


def test_synthetic_recipe_is_deterministic(synth):
    a = synth.make_pair(3, size1=(640, 480), n1=200)
    b = synth.make_pair(3, size1=(640, 480), n1=200)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    kp1, kp2, m = a
    assert (m["queryIdx"] == np.arange(200)).all()  # BFMatcher without cross-check: M = N1, queryIdx = i
    assert kp1["x"].min() >= 0 and kp1["x"].max() < 639 and kp2["y"].max() < 479
    f1 = synth.make_sequence(9, 4, size=(640, 480), n_kp=100)
    f2 = synth.make_sequence(9, 4, size=(640, 480), n_kp=100)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(f1, f2))


_GLOO_WORKER = r'''
# The rank-side driver logic of bench.py (sfm-gms_amd/dist.py: RankPlan, synth_matches_device, parity_sample and the gloo
# rendezvous), on CPU tensors: everything except the filter launch itself.
import importlib, os, sys, json
sys.path.insert(0, sys.argv[1])
import numpy as np
pkg = importlib.import_module("sfm-gms_amd")
d = importlib.import_module("sfm-gms_amd.dist")
rank, local_rank, world = d.env_world()
dist = d.init_rendezvous(world)
assert dist is not None and dist.get_backend() == "gloo"
n_frames, n_kp, per_step, n_chunks = 40, 300, 64, 5
plan = d.RankPlan(n_frames, n_kp, per_step, n_chunks, rank, world)
assert plan.total_pairs == 780 and (plan.lo, plan.hi) == pkg.shard_range(780, rank, world)
seen = []
for c in range(n_chunks):
    t = plan.chunk_pairs(c)
    k0 = plan.starts[c]
    assert plan.lo <= k0 and k0 + plan.chunk <= plan.hi          # a chunk never leaves the rank's block
    assert [(int(a), int(b)) for a, b in zip(t["frame_a"], t["frame_b"])] == [pkg.pair_from_index(k0 + j, n_frames) for j in range(plan.chunk)]
    assert (t["match_off"] == np.arange(plan.chunk) * n_kp).all() and (t["m"] == n_kp).all()
    m = d.synth_matches_device(k0, plan.chunk, n_kp, 0.5, "cpu").numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
    for k, j in plan.chunk_sample(c):
        assert k % d.PARITY_EVERY == 0 and k == k0 + j
        seen.append(k)
    j = plan.chunk // 2                                           # any pair: device form == host form, whatever the rank
    assert m[j * n_kp:(j + 1) * n_kp].tobytes() == d.synth_matches_host(k0 + j, n_kp, 0.5).tobytes()
d.barrier(dist)
slow = d.max_over_ranks(1.0 + rank, dist)
tot = d.sum_over_ranks([plan.hi - plan.lo, len(set(seen))], dist)
counts = d.gather_counts(plan.hi - plan.lo, dist)
if rank == 0:
    print(json.dumps({"max": slow, "counts": counts, "sum": tot, "starts": plan.starts}))
d.barrier(dist)
dist.destroy_process_group()
'''


def test_two_rank_driver_logic_under_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_GLOO_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29731", str(script), ROOT]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    import json
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    got = json.loads(line)
    assert got["max"] == 2.0 and got["counts"] == [390, 390] and got["sum"][0] == 780
    assert got["starts"] == [0, 64, 128, 192, 256]   # rank 0 walks its block front to back
    assert got["sum"][1] == 1                         # pair 0 is the only multiple of 997 below 780 (rank 0 filtered it)


def test_bench_imports_the_driver_module_the_gloo_test_covers():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for name in ("RankPlan", "synth_matches_device", "init_rendezvous", "max_over_ranks", "sum_over_ranks", "barrier"):
        assert ("distmod." + name in src) or ("self.dist." + name in src) or ("wl.dist." + name in src), name
    assert '"nccl"' not in src and "init_process_group" not in src  # the rendezvous is dist.py's (gloo)


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True,
                         timeout=120, env=env)
    assert res.returncode != 0 and "--gpus 4" in res.stderr


def test_bench_refuses_zero_timed_steps():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "--steps" in res.stderr


def test_bench_full_is_off_by_default(monkeypatch):
    import importlib
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


def test_bench_dump_outputs_writes_what_the_step_returned(pkg, tmp_path):
    """bench.dump_outputs on a stand-in for a resident chunk (CPU tensors): every result record, the survivors of the seeded
    sample in order, float32 / float64 only, within 64 MB at 10k matches per pair, the same files from run to run."""
    import importlib
    import torch
    bench = importlib.import_module("bench")
    d = importlib.import_module("sfm-gms_amd.dist")
    n_pairs, n_kp = 300, 10000
    rng = np.random.default_rng(5)
    res = np.zeros(n_pairs, dtype=pkg.RESULT_DTYPE)
    res["n_inliers"] = rng.integers(0, n_kp + 1, n_pairs)
    res["n_inliers"][::7] = n_kp  # pairs that keep everything: the size bound holds for them too
    res["best_rot"], res["best_scale"] = rng.integers(0, 8, n_pairs), rng.integers(0, 5, n_pairs)
    out = np.zeros(n_pairs * n_kp, dtype=pkg.DMATCH_DTYPE)
    out["queryIdx"], out["trainIdx"] = np.tile(np.arange(n_kp), n_pairs), rng.integers(0, n_kp, n_pairs * n_kp)
    out["distance"] = rng.random(n_pairs * n_kp, dtype=np.float32)

    class Wl:
        chunks = [None, dict(pairs=d.pair_table(40, 100, 100 + n_pairs, n_kp),
                             d_out=torch.from_numpy(out.view(np.int32).reshape(-1, 4).copy()),
                             d_res=torch.from_numpy(res.view(np.int32).reshape(-1, 4).copy()))]
    Wl.n_kp = n_kp

    info = bench.dump_outputs(Wl, pkg, 1, str(tmp_path / "a"))
    bench.dump_outputs(Wl, pkg, 1, str(tmp_path / "b"))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["results.npy", "sample_matches.npy", "sample_pairs.npy"] == sorted(os.listdir(tmp_path / "b"))
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) == info["bytes"] <= 64 << 20
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    assert np.array_equal(got["results"], np.stack([res[f] for f in pkg.RESULT_DTYPE.names], axis=1))
    sp = got["sample_pairs"]
    assert len(sp) == info["sample_pairs"] > 0 and np.all(np.diff(sp[:, 0]) > 0)
    pt = Wl.chunks[1]["pairs"]
    want = []
    for j, fa, fb, k in sp.astype(np.int64):
        assert (fa, fb, k) == (pt["frame_a"][j], pt["frame_b"][j], res["n_inliers"][j])
        want.append(out[j * n_kp:j * n_kp + k])
    want = np.concatenate(want)
    assert np.array_equal(got["sample_matches"], np.stack([want[f].astype(np.float32) for f in pkg.DMATCH_DTYPE.names], axis=1))


def test_vectorised_pair_indexing_and_match_synthesis(pkg):
    import importlib
    d = importlib.import_module("sfm-gms_amd.dist")
    for n in (2, 3, 17, 1000):
        total = pkg.all_pairs_count(n)
        k = np.unique(np.concatenate([np.arange(min(total, 400)), np.arange(max(0, total - 400), total),
                                      np.linspace(0, total - 1, 300).astype(np.int64)]))
        a, b = d.pairs_from_indices(k, n)
        assert [pkg.pair_from_index(int(x), n) for x in k] == list(zip(a.tolist(), b.tolist()))
    with pytest.raises(IndexError):
        d.pairs_from_indices([3], 3)
    m = d.synth_matches_host(499499, 10000, 0.5)
    assert (m["queryIdx"] == np.arange(10000)).all() and m["trainIdx"].min() >= 0 and m["trainIdx"].max() < 10000
    assert 0.47 < (m["trainIdx"] == m["queryIdx"]).mean() < 0.53 and 0 <= m["distance"].min() and m["distance"].max() < 256
    dev = d.synth_matches_device(499498, 2, 10000, 0.5, "cpu").numpy().view(np.uint8).reshape(-1).view(pkg.DMATCH_DTYPE)
    assert dev[10000:].tobytes() == m.tobytes()
    assert d.parity_sample(0, 2000) == [0, 997, 1994] and d.parity_sample(998, 996) == [] and d.parity_sample(998, 997) == [1994]
    starts, chunk = d.chunk_starts(100, 1100, 300, 5)
    assert chunk == 300 and starts == [100, 400, 700, 100, 400]
    starts, chunk = d.chunk_starts(0, 50, 300, 2)
    assert chunk == 50 and starts == [0, 0]
