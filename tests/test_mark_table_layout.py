"""CPU: the half-cell rule behind the byte-matrix kernel's mark table (gms::dense_half_cell_owner, sfm-gms_amd/csrc/gms_kernel_dense.h),
compiled for the host by g++ into tests/cpp/mark_table_check.cpp -- a test build; the kernel's table builder calls the same function.
For all 1600 half cells x 4 grid types the owning cell agrees with what a match's code word yields (row = cell under grid type 1 +
(q & (gx + 20 gy)), nobody where an edge bit meets a shifted axis), every (cell, grid type) owns exactly the half cells that
dense_nleft_cm sums for it, and the table's place in the LDS is checked at compile time."""
import hostbuild as hb


SRC = "mark_table_check.cpp"


def _run(exe):
    res = hb.run_clean(exe)
    report = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and "mark_table: ok" in res.stdout, report


def test_mark_table_layout():
    exe = hb.host_exe(SRC)
    _run(exe)


def test_mark_table_layout_under_sanitizers():
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = hb.host_exe_sanitized(SRC)
    _run(exe)
