"""CPU: the offset arithmetic of the one-shot host entry points' device block (gms::BlockLayout, sfm-gms_amd/csrc/block_layout.h),
compiled for the host by g++ into tests/cpp/block_layout_check.cpp -- a test build, the product includes the same header in
capi_common.h, for the one-shot entry points of the capi_*.cpp. Over a few thousand seeded sequences of add(bytes, slack), with sizes 0, 1, 255, 256, 257 and above 4 GiB among them:
every offset is a multiple of 256, regions follow each other in call order without overlap, each is at least bytes + slack long, and
the block is less than 256 * (regions + 1) bytes larger than what it holds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "block_layout_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "sfm-gms_amd", "csrc")]


def _run(exe, sequences, seed):
    res = subprocess.run([exe, str(sequences), str(seed)], capture_output=True, text=True, timeout=120)
    report = (res.stdout + res.stderr)[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, report
    assert res.returncode == 0 and f"{sequences} sequences" in res.stdout and ": 0 bad" in res.stdout, report


def test_block_layout(tmp_path):
    exe = str(tmp_path / "block_layout_check")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-o", exe, SRC])
    _run(exe, 4000, 1)
    _run(exe, 4000, 2)


def test_block_layout_under_sanitizers(tmp_path):
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = str(tmp_path / "block_layout_check_san")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS, "-o", exe, SRC],
                           capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("this toolchain cannot build with -fsanitize=address,undefined: " +
                    (build.stderr.strip().splitlines() or ["?"])[-1][:200])
    _run(exe, 4000, 1)
