"""How the tests compile and run C++ with g++, stated once: the paths, four kinds of build with one flag set each, a per-process
cache that builds each artefact once, the probe that tells a toolchain without a sanitizer from a source that does not compile,
running a program, and the FNV-1a digest that the stand-alone programs of tests/cpp print (tests/cpp/test_main_util.h). Everything
built here is host code: sanitized builds are stand-alone executables run as child processes, never loaded into python."""
import atexit
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
SHIM_INCLUDE = os.path.join(ROOT, "sfm-gms_amd", "include")
CPP = os.path.join(ROOT, "tests", "cpp")

STRICT = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
HOST = ["-ffp-contract=off", *STRICT, "-I" + CSRC, "-I" + INCLUDE]

compiles = 0          # g++ invocations so far (tests/test_hostbuild.py reads it)
_cache = {}
_probed = {}
_dir = None


def _compile(kind, src, flags, tail=()):
    """g++ flags src tail -o <artefact>, once per process for each (kind, src, flags, tail). src is a path, or a name in tests/cpp."""
    global _dir, compiles
    src = os.path.join(CPP, src)
    key = (kind, src, tuple(flags), tuple(tail))
    if key not in _cache:
        if _dir is None:
            _dir = tempfile.mkdtemp(prefix="hostbuild_")
            atexit.register(shutil.rmtree, _dir, ignore_errors=True)
        stem = os.path.splitext(os.path.basename(src))[0]
        out = os.path.join(_dir, f"{stem}_{len(_cache)}" + (".so" if kind == "lib" else ""))
        compiles += 1
        res = subprocess.run(["g++", *flags, src, *tail, "-o", out], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"g++ failed on {src} ({kind}):\n{res.stderr[-4000:]}")
        _cache[key] = out
    return _cache[key]


def _defines(defines):
    return ["-D" + d for d in defines]


def host_lib(src, defines=()):
    """A shared library of host code, for ctypes."""
    return _compile("lib", src, ["-O2", *HOST, "-shared", "-fPIC", *_defines(defines)])


def host_exe(src, defines=(), extra=()):
    """A stand-alone host program; extra carries things like -pthread."""
    return _compile("exe", src, ["-O2", *HOST, *_defines(defines), *extra])


def host_exe_sanitized(src, sanitizers="address,undefined", defines=(), extra=()):
    """The same program under sanitizers. Skips only where a trivial program does not build with them; a source that does not
    build where the trivial one does fails like any other."""
    san = ["-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"]
    if sanitizers not in _probed:
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "probe.cpp"), "w") as f:
                f.write("int main(){}\n")
            res = subprocess.run(["g++", *san, f.name, "-o", os.path.join(d, "probe")], capture_output=True, text=True)
        _probed[sanitizers] = None if res.returncode == 0 else (res.stderr.strip().splitlines() or ["?"])[-1][:200]
    if _probed[sanitizers] is not None:
        pytest.skip(f"this toolchain cannot build with -fsanitize={sanitizers}: " + _probed[sanitizers])
    return _compile("san", src, ["-O1", "-g", *san, *HOST, *_defines(defines), *extra])


def shim_exe(main_src):
    """A program on the public C++ header (sfm-gms_amd/include/mi355_gms.hpp), linked to libgms_hip.so: the only builds of that
    header by a compiler that is not hipcc."""
    return _compile("shim", main_src, ["-O1", *STRICT, "-I" + INCLUDE, "-I" + SHIM_INCLUDE],
                    ["-L", CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"])


def run(exe, *args, timeout=120, env=None):
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout,
                          env=None if env is None else dict(os.environ, **env))


def run_clean(exe, *args, timeout=120, env=None):
    """run(), and no sanitizer spoke and the exit status is 0."""
    res = run(exe, *args, timeout=timeout, env=env)
    report = (res.stdout + res.stderr)[-4000:]
    assert not any(s in res.stderr for s in ("runtime error", "AddressSanitizer", "ThreadSanitizer")), report
    assert res.returncode == 0, report
    return res


def fnv1a(data, words=False):
    """FNV-1a, 64 bits, over the bytes of anything with a (C-contiguous) buffer; words=True takes one step per 32-bit word, as
    fnv_words() of tests/cpp/test_main_util.h does for the match lists."""
    s = 14695981039346656037
    view = memoryview(data)
    for v in view.cast("B").cast("I" if words else "B") if view.nbytes else ():       # a view with a 0 in its shape does not cast
        s = ((s ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return s
