"""CPU: the half-cell rule behind the byte-matrix kernel's mark table (gms::dense_half_cell_owner, sfm-gms_amd/csrc/gms_kernel_dense.h),
compiled for the host by g++ into tests/cpp/mark_table_check.cpp -- a test build; the kernel's table builder calls the same function.
For all 1600 half cells x 4 grid types the owning cell agrees with what a match's code word yields (row = cell under grid type 1 +
(q & (gx + 20 gy)), nobody where an edge bit meets a shifted axis), every (cell, grid type) owns exactly the half cells that
dense_nleft_cm sums for it, and the table's place in the LDS is checked at compile time."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mark_table_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "sfm-gms_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    report = (res.stdout + res.stderr)[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, report
    assert res.returncode == 0 and "mark_table: ok" in res.stdout, report


def test_mark_table_layout(tmp_path):
    exe = str(tmp_path / "mark_table_check")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-o", exe, SRC])
    _run(exe)


def test_mark_table_layout_under_sanitizers(tmp_path):
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = str(tmp_path / "mark_table_check_san")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS, "-o", exe, SRC],
                           capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("this toolchain cannot build with -fsanitize=address,undefined: " +
                    (build.stderr.strip().splitlines() or ["?"])[-1][:200])
    _run(exe)
