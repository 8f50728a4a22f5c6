"""CPU: the offset arithmetic of the one-shot host entry points' device block (gms::BlockLayout, sfm-gms_amd/csrc/block_layout.h),
compiled for the host by g++ into tests/cpp/block_layout_check.cpp -- a test build, the product includes the same header in
capi_common.h, for the one-shot entry points of the capi_*.cpp. Over a few thousand seeded sequences of add(bytes, slack), with sizes 0, 1, 255, 256, 257 and above 4 GiB among them:
every offset is a multiple of 256, regions follow each other in call order without overlap, each is at least bytes + slack long, and
the block is less than 256 * (regions + 1) bytes larger than what it holds."""
import hostbuild as hb


SRC = "block_layout_check.cpp"


def _run(exe, sequences, seed):
    res = hb.run_clean(exe, sequences, seed)
    report = (res.stdout + res.stderr)[-4000:]
    assert res.returncode == 0 and f"{sequences} sequences" in res.stdout and ": 0 bad" in res.stdout, report


def test_block_layout():
    exe = hb.host_exe(SRC)
    _run(exe, 4000, 1)
    _run(exe, 4000, 2)


def test_block_layout_under_sanitizers():
    """The same under AddressSanitizer and UndefinedBehaviorSanitizer (host code, a CPU build)."""
    exe = hb.host_exe_sanitized(SRC)
    _run(exe, 4000, 1)
