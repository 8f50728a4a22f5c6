"""Generator of tests/golden/ws_layout_sizes.txt: the sizes the built library gives for its device workspaces -- six public
gms_*_workspace_bytes functions (the zero of a refused input included) and the four internal per-pair figures that plan_workspace
divides its budget by -- over a few hundred argument tuples, one text line each: `<name> <arguments ...> <bytes>`.

ws_layout_runner.cpp (beside this file) makes the tuples and asks the library; this script compiles it with hipcc (host code only: it
includes the library's internal header) against sfm-gms_amd/csrc/libgms_hip.so, runs it -- no device is needed -- and writes the
file. It reads nothing but this repository's own library.

The committed fixture was recorded at commit 063d3a7, whose size functions were hand-written sums apart from the launchers' pointer
walks; tests/test_ws_layout.py holds the layouts of ws_layout.h to it. Its `refined` lines (gms_detect_dog_refined_workspace_bytes on the
tuples of the `pyramid` lines, appended at the end) were recorded at commit e96d1ca, the last one whose refined layout was a struct
of its own beside the pyramid's. Regenerating it from a later library must not change a line.

usage (after the library is built): python tests/golden/make_ws_layout_fixture.py
"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "sfm-gms_amd", "csrc")


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ws_layout_runner")
        subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               os.path.join(HERE, "ws_layout_runner.cpp"), "-L" + CSRC, "-lgms_hip", "-Wl,-rpath," + CSRC, "-o", exe])
        text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    out = os.path.join(HERE, "ws_layout_sizes.txt")
    with open(out, "w") as f:
        f.write(text)
    print(f"{out}: {len(text.splitlines())} lines, {len(text)} bytes")


if __name__ == "__main__":
    main()
