"""CPU: who writes which field of the byte-matrix kernel's mark table (sfm-gms_amd/csrc/gms_kernel_dense.h: dense_cell_half_slot,
dense_mark_none_field), compiled for the host by g++ into tests/cpp/mark_scatter_check.cpp -- a test build; the kernel's scatter calls
the same functions. Over all kDenseMarkEntries x 4 fields: the verifying lanes and the none-writers hit every field exactly once
(clamped stores repeat one of their writer's own), an owned field's writer is dense_half_cell_owner()'s cell, and the none-writers'
fields are exactly the ones that function gives to nobody plus the entries from kFineN to the sink's."""
import hostbuild as hb


SRC = "mark_scatter_check.cpp"


def _run(exe):
    res = hb.run_clean(exe)
    report = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and "mark_scatter: ok" in res.stdout, report


def test_mark_scatter_layout():
    exe = hb.host_exe(SRC)
    _run(exe)


def test_mark_scatter_layout_under_sanitizers():
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = hb.host_exe_sanitized(SRC)
    _run(exe)
