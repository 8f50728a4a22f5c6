"""CPU: the argument checks that the host ABI sources share (sfm-gms_amd/csrc/capi_checks.h: alignment, the caller's workspace, host
frame offsets, the walk over a host pair table, overlapping byte ranges, the registration's arrays), compiled for the host by g++ into
tests/cpp/capi_checks_check.cpp -- a test build, the product includes the same header in gms_capi.cpp and the capi_*.cpp beside it.
The program pins the edges that the entry points' own copies of these checks handled: a decreasing and a negative frame offset, match
ranges that end at and one past 2^40, a frame index equal to the number of frames, workspaces one byte off and one byte short, byte
ranges that abut and that share one byte."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "capi_checks_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "sfm-gms_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    report = (res.stdout + res.stderr)[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, report
    assert res.returncode == 0 and "capi_checks_check: 0 bad" in res.stdout, report


def test_capi_checks(tmp_path):
    exe = str(tmp_path / "capi_checks_check")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-o", exe, SRC])
    _run(exe)


def test_capi_checks_under_sanitizers(tmp_path):
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = str(tmp_path / "capi_checks_check_san")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS, "-o", exe, SRC],
                           capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("this toolchain cannot build with -fsanitize=address,undefined: " +
                    (build.stderr.strip().splitlines() or ["?"])[-1][:200])
    _run(exe)
