#!/usr/bin/env python3
"""Compare two builds' device assembly, function by function.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --offload-device-only -S x.hip -o before/x.s     (every filter source)
    ... the same for the other build into after/ ...
    tools/asm_compare.py before after

Takes two directories of .s files; a function may sit in differently named files on the two sides. For every function of
either side (kernels and non-inlined device functions) it compares the instruction stream, the .amdhsa_* descriptor block
with the function's resource symbols (.set NAME.num_vgpr, ...) and the .amdgpu_metadata entry, and prints equal / DIFFERENT
per function. The only normalisation: comments are dropped, and local labels (.LBB<n>_<m>, .Lfunc_end<n>, .Ltmp<n>, ...)
are renumbered by order of appearance within the function. Exit status 1 when anything differs or exists on one side only.
"""
import pathlib
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_$]+[0-9]+(?:_[0-9]+)?")


def clean(line):
    return line.split(";", 1)[0].rstrip()


def renumber(lines):
    names = {}
    return [LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln) for ln in lines]


def parse(directory):
    """{symbol: {"code": [...], "descriptor": [...], "metadata": [...]}} over all .s files of a directory"""
    out = {}
    for path in sorted(pathlib.Path(directory).glob("*.s")):
        lines = path.read_text().splitlines()
        i, n = 0, len(lines)
        while i < n:
            m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
            if not m:
                i += 1
                continue
            sym, code, desc, in_desc = m.group(1), [], [], False
            i += 1
            while i < n and not re.match(r"\s*\.size\s+" + re.escape(sym) + ",", lines[i]):
                ln = clean(lines[i])
                i += 1
                if ln.strip().startswith(".amdhsa_kernel"):
                    in_desc = True
                if in_desc:
                    desc.append(ln.strip())
                    in_desc = not ln.strip().startswith(".end_amdhsa_kernel")
                elif ln.strip() and not re.match(r"\s*\.(text|section|p2align)\b", ln):
                    code.append(ln.strip())
            while i < n and not re.match(r"\s*\.(type|section|protected|globl|text)\b", lines[i]):
                if lines[i].strip().startswith(".set " + sym + "."):
                    desc.append(lines[i].strip())
                i += 1
            out[sym] = {"code": renumber(code), "descriptor": desc, "metadata": []}
        # metadata: the list entries under amdhsa.kernels, each named by its .name line
        try:
            a = next(k for k, ln in enumerate(lines) if ln.startswith("amdhsa.kernels:"))
        except StopIteration:
            continue
        entry = []
        for ln in lines[a + 1:] + ["x"]:
            if ln.startswith("  - ") or not ln.startswith("  "):
                name = next((e.split(":", 1)[1].strip() for e in entry if e.strip().startswith(".name:")), None)
                if name in out:
                    out[name]["metadata"] = entry
                entry = []
                if not ln.startswith("  "):
                    break
            entry.append(ln)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for sym in sorted(set(before) | set(after)):
        if sym not in before or sym not in after:
            verdict = "only in " + (sys.argv[1] if sym in before else sys.argv[2])
        else:
            diff = [part for part in ("code", "descriptor", "metadata") if before[sym][part] != after[sym][part]]
            verdict = "DIFFERENT (" + ", ".join(diff) + ")" if diff else "equal"
        bad += verdict != "equal"
        print("%-12s %s" % (verdict if verdict == "equal" else verdict.split(" ")[0], sym) + ("" if verdict == "equal" else "   " + verdict))
    kernels = sum(1 for s in after.values() if s["descriptor"] and s["descriptor"][0].startswith(".amdhsa_kernel"))
    print("%d functions (%d kernels), %d not equal" % (len(set(before) | set(after)), kernels, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
