"""CPU: the host staging pool of gms_filter_host_batch (sfm-gms_amd/csrc/copy_pool.h), compiled for the host by g++ into the stress
driver tests/cpp/copy_pool_stress.cpp -- a test build, the product links the same header into libgms_hip.so. The driver's hook sleeps at
the pool's hand-off points (a worker "descheduled" between taking a generation and its first ticket, before it counts out, and the
caller between publishing a run and working along), with more workers than cores, over thousands of runs whose part counts grow and
shrink. A worker of one run that reached into the next one left that run waiting forever or returning before every byte had landed
(the watchdog's "HANG after N runs" / the byte check), and under ThreadSanitizer it is a data race on the run's offsets."""
import hostbuild as hb


SRC = "copy_pool_stress.cpp"


def _run(exe, args, env=None):
    res = hb.run(exe, *args, env=env)
    report = (res.stdout + res.stderr)[-4000:]
    assert "HANG" not in res.stdout, report
    assert "ThreadSanitizer" not in res.stderr, report
    assert res.returncode == 0 and ": 0 bad runs" in res.stdout, report
    return res.stdout


def test_copy_pool_stress():
    """2000 runs, 15 workers, hooks sleeping up to 3 ms."""
    exe = hb.host_exe(SRC, extra=("-pthread",))          # the pool's workers are std::threads
    out = _run(exe, [2000, 1, 15])
    assert "2000 runs" in out


def test_copy_pool_stress_under_thread_sanitizer():
    """The same under ThreadSanitizer: every copy and check is several times slower there, so the lists are shorter (4-8 parts) and
    the hooks sleep up to 100 ms -- a sleeping worker still outlasts the rest of its run, as it does in the plain build."""
    exe = hb.host_exe_sanitized(SRC, "thread", extra=("-pthread",))         # a race shows under ThreadSanitizer, not under the default set
    out = _run(exe, [120, 2, 15, 8, 100000], env={"TSAN_OPTIONS": "halt_on_error=1"})
    assert "120 runs" in out
