#!/usr/bin/env python3
"""Per-kernel ISA comparison of two trees' device code: `same`, `renumbered` (equal opcode sequence) or the number of
differing lines.   python tools/isa_diff.py <parent tree> <this tree> [--filter SUBSTR]
Each tree's calib_lm.hip is compiled with the Makefile's flags plus --cuda-device-only -S (about 30 s per tree)."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S"]


def kernels(tree, drop_args):
    """demangled kernel name -> its instructions and labels (comments, blank lines and directives dropped)"""
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-o", f.name, "calib_lm.hip"], check=True,
                       cwd=os.path.join(tree, "camera-calibration_amd", "csrc"))
        text = open(f.name).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(.*", "", name.replace("void calib::", ""))
        if drop_args:       # the parent's fused_kernel<MODEL, T, 32, 4, ...> is this tree's fused_kernel<MODEL, T, ...>
            name = re.sub(r"^(fused_kernel<\d+, \w+), 32, 4,", r"\1,", name)
        body = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
        out[name] = [ln for ln in body if ln and not (ln[0] == "." and ln[-1] != ":")]     # labels stay, directives go
    return out


def main():
    args = sys.argv[1:]
    flt = args[args.index("--filter") + 1] if "--filter" in args else ""
    a, b = kernels(args[0], True), kernels(args[1], False)
    for name in sorted(set(a) | set(b)):
        if flt not in name:
            continue
        if name not in a or name not in b:
            print(f"{name:90s} only in {'parent' if name in a else 'this'}")
            continue
        x, y = a[name], b[name]
        if x == y:
            verdict = "same"
        elif [ln.split()[0] for ln in x] == [ln.split()[0] for ln in y]:
            verdict = f"renumbered ({sum(p != q for p, q in zip(x, y))} lines)"
        else:
            d = sum(1 for ln in difflib.unified_diff(x, y, lineterm="", n=0) if ln[0] in "+-" and ln[:3] not in ("+++", "---"))
            verdict = f"{d} lines differ ({len(x)} -> {len(y)} lines)"
        print(f"{name:90s} {verdict}")


if __name__ == "__main__":
    main()
