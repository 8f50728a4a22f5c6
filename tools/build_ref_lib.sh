#!/bin/bash
# Diagnostic: build the library from the whole csrc/ of a git revision (for tools/ab_bench.py), in a temporary directory.
# tools/build_ref_lib.sh <rev> <name>  ->  sfm-gms_amd/csrc/libgms_hip_<name>.so
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd); C=$ROOT/sfm-gms_amd/csrc; T=$(mktemp -d)
git -C "$ROOT" archive "$1" sfm-gms_amd/csrc include | tar -x -C "$T"
make -C "$T/sfm-gms_amd/csrc" -s -j"${MAX_JOBS:-16}" libgms_hip.so
cp "$T/sfm-gms_amd/csrc/libgms_hip.so" "$C/libgms_hip_$2.so"
rm -rf "$T"; echo "$C/libgms_hip_$2.so"
