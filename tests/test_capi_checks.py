"""CPU: the argument checks that the host ABI sources share (sfm-gms_amd/csrc/capi_checks.h: alignment, the caller's workspace, host
frame offsets, the walk over a host pair table, overlapping byte ranges, the registration's arrays), compiled for the host by g++ into
tests/cpp/capi_checks_check.cpp -- a test build, the product includes the same header in gms_capi.cpp and the capi_*.cpp beside it.
The program pins the edges that the entry points' own copies of these checks handled: a decreasing and a negative frame offset, match
ranges that end at and one past 2^40, a frame index equal to the number of frames, workspaces one byte off and one byte short, byte
ranges that abut and that share one byte."""
import hostbuild as hb


SRC = "capi_checks_check.cpp"


def _run(exe):
    res = hb.run_clean(exe)
    report = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and "capi_checks_check: 0 bad" in res.stdout, report


def test_capi_checks():
    exe = hb.host_exe(SRC)
    _run(exe)


def test_capi_checks_under_sanitizers():
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = hb.host_exe_sanitized(SRC)
    _run(exe)
