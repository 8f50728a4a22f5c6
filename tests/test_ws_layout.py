"""CPU: the layouts of nine device workspaces (sfm-gms_amd/csrc/ws_layout.h; the pyramid's in both its forms), compiled for the host by g++ into
tests/cpp/ws_layout_check.cpp -- a test build, the product includes the same header in its launchers. Over n in {1, 2, 3, 63, 64, 255,
257} pairs or images, odd image sizes, 0 and 1 keypoints, 1 and 16 levels, no backward rows, match capacities at both ends of
big_mcap's range and around a multiple of 4096, and sizes beyond 4 GiB: the regions follow each other in declaration order without
overlap, each holds what its kernel indexes and starts on the alignment its readers need, the cleared spans cover what they are
meant to, and a slice of n pairs fits n times the bytes per pair that plan_workspace reserves. The sizes equal those recorded from
the library before the layouts existed (tests/golden/ws_layout_sizes.txt, made by tests/golden/make_ws_layout_fixture.py) -- and so
do the public gms_*_workspace_bytes functions of the built library, refusals included."""
import ctypes as C
import os

import hostbuild as hb


SRC = "ws_layout_check.cpp"
FIXTURE = os.path.join(hb.ROOT, "tests", "golden", "ws_layout_sizes.txt")


def _run(exe, seed):
    res = hb.run_clean(exe, FIXTURE, seed)
    report = (res.stdout + res.stderr)[-4000:]
    with open(FIXTURE) as f:
        lines = sum(1 for _ in f)
    assert res.returncode == 0 and f"{lines} fixture lines: 0 bad" in res.stdout, report


def test_ws_layout():
    exe = hb.host_exe(SRC)
    _run(exe, 1)
    _run(exe, 2)


def test_ws_layout_under_sanitizers():
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = hb.host_exe_sanitized(SRC)
    _run(exe, 1)


def test_public_workspace_bytes_match_the_recorded_sizes(pkg):
    """The public size functions of the built library give the recorded value for every recorded tuple, the 0 of a refused input
    included (no device call: the functions are arithmetic). The gradient rows and the unrefined DoG detector add no region, so their
    functions are held to the `pyramid` lines; the refined DoG call to its own."""
    lib = pkg.load_library()
    fns = {"detect": ([lib.gms_detect_workspace_bytes], [C.c_int] * 4),
           "pyramid": ([lib.gms_detect_pyramid_workspace_bytes, lib.gms_detect_pyramid_grad_workspace_bytes, lib.gms_detect_dog_workspace_bytes],
                       [C.c_int] * 5),
           "refined": ([lib.gms_detect_dog_refined_workspace_bytes], [C.c_int] * 5),
           "stereo": ([lib.gms_stereo_bm_workspace_bytes], [C.c_int] * 3 + [C.c_void_p]),
           "portrait": ([lib.gms_portrait_workspace_bytes], [C.c_int] * 3 + [C.c_void_p]),
           "bfsel": ([lib.gms_bf_select_workspace_bytes], [C.c_int, C.c_int, C.c_int64])}
    seen = {name: 0 for name in fns}
    with open(FIXTURE) as f:
        for line in f:
            name, *args = line.split()
            if name not in fns:
                continue
            callees, argtypes = fns[name]
            *args, want = [int(a) for a in args]
            if name in ("stereo", "portrait"):
                args.append(None)  # the reference's parameters
            for fn in callees:
                got = C.CFUNCTYPE(C.c_size_t, *argtypes)(C.cast(fn, C.c_void_p).value)(*args)
                assert got == want, (fn.__name__, line)
            seen[name] += 1
    assert all(count >= 100 for count in seen.values()), seen
