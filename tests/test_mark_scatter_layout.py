"""CPU: who writes which field of the byte-matrix kernel's mark table (sfm-gms_amd/csrc/gms_kernel_dense.h: dense_cell_half_slot,
dense_mark_none_field), compiled for the host by g++ into tests/cpp/mark_scatter_check.cpp -- a test build; the kernel's scatter calls
the same functions. Over all kDenseMarkEntries x 4 fields: the verifying lanes and the none-writers hit every field exactly once
(clamped stores repeat one of their writer's own), an owned field's writer is dense_half_cell_owner()'s cell, and the none-writers'
fields are exactly the ones that function gives to nobody plus the entries from kFineN to the sink's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mark_scatter_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "sfm-gms_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    report = (res.stdout + res.stderr)[-4000:]
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, report
    assert res.returncode == 0 and "mark_scatter: ok" in res.stdout, report


def test_mark_scatter_layout(tmp_path):
    exe = str(tmp_path / "mark_scatter_check")
    subprocess.check_call(["g++", "-O2", *FLAGS, "-o", exe, SRC])
    _run(exe)


def test_mark_scatter_layout_under_sanitizers(tmp_path):
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = str(tmp_path / "mark_scatter_check_san")
    build = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *FLAGS, "-o", exe, SRC],
                           capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("this toolchain cannot build with -fsanitize=address,undefined: " +
                    (build.stderr.strip().splitlines() or ["?"])[-1][:200])
    _run(exe)
