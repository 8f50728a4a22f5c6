"""tests/hostbuild.py itself: an artefact is built once per process, a source that does not compile raises with the compiler's
diagnostic, under sanitizers too (where only a toolchain without the sanitizer skips), and fnv1a gives the published FNV-1a 64
values."""
import numpy as np
import pytest

import hostbuild as hb


@pytest.fixture
def broken(tmp_path):
    path = tmp_path / "broken.cpp"
    path.write_text("int main() { return not_declared_anywhere; }\n")
    return str(path)


def test_a_second_request_compiles_nothing():
    first = hb.host_exe("block_layout_check.cpp")
    count = hb.compiles
    assert hb.host_exe("block_layout_check.cpp") == first and hb.compiles == count
    assert hb.host_exe("block_layout_check.cpp", defines=("HOSTBUILD_TEST_OTHER_KEY",)) != first and hb.compiles == count + 1


def test_a_source_that_does_not_compile_raises_with_the_diagnostic(broken):
    with pytest.raises(RuntimeError, match="not_declared_anywhere"):
        hb.host_exe(broken)
    with pytest.raises(RuntimeError, match="not_declared_anywhere"):
        hb.host_lib(broken)


def test_under_sanitizers_it_fails_and_does_not_skip(broken):
    hb.host_exe_sanitized("block_layout_check.cpp")         # skips here, and only here, where the toolchain lacks the sanitizers
    with pytest.raises(RuntimeError, match="not_declared_anywhere"):
        hb.host_exe_sanitized(broken)


def test_fnv1a_published_values():
    assert hb.fnv1a(b"") == 0xCBF29CE484222325 and hb.fnv1a(b"a") == 0xAF63DC4C8601EC8C
    assert hb.fnv1a(b"foobar") == 0x85944171F73967E8
    assert hb.fnv1a(b"\x01\x00\x00\x00", words=True) == hb.fnv1a(b"\x01")
    assert hb.fnv1a(np.zeros((0, 4), np.int32), words=True) == hb.fnv1a(b"") and hb.fnv1a(np.arange(3, dtype=np.uint8)) == hb.fnv1a(b"\0\1\2")
