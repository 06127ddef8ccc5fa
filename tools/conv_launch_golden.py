#!/usr/bin/env python3
"""Regenerate tests/golden/conv_launch_records.txt: the launch records of csrc/conv_host_check.cpp on the sources of ANOTHER revision.

Usage: tools/conv_launch_golden.py REV        (REV: the commit whose host code is the reference, e.g. the parent of a refactor)

The csrc/ and include/ of REV are extracted into a temporary directory, THIS tree's conv_host_check.cpp (the case table) is put beside
them, and the program is built for the host only with -ftrivial-auto-var-init=zero, so that an argument field REV's entries leave
unset reads as zero (the tree under test is built with =pattern: csrc/Makefile).  Its output, with the differences listed in
EXPECTED applied, becomes the golden file.  Needs hipcc; touches no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_launch_records.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ("--offload-host-only -O1 -std=c++17 -ffp-contract=off -Wno-unused-function -fsanitize=address,undefined "
         "-fno-sanitize-recover=undefined -ftrivial-auto-var-init=zero -Wl,--unresolved-symbols=ignore-all -x hip").split()

# Differences from REV's records that are meant: (entry prefix, pattern, replacement, why).
EXPECTED = [
    ("effi_conv3d_k3s1_bf16x3_f32", r" zcount=(\d+) hin=", r" zcount=\1 zin=\1 hin=",
     "the z-batched split 3-D entry left zin unset (no kernel of its launcher reads it); conv_volume sets zin = D for every volume"),
]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", sys.argv[1], "effi_mvs_plus_amd/csrc", "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
        csrc = os.path.join(tmp, "effi_mvs_plus_amd", "csrc")
        with open(os.path.join(ROOT, "effi_mvs_plus_amd", "csrc", "conv_host_check.cpp")) as f, open(os.path.join(csrc, "conv_host_check.cpp"), "w") as g:
            g.write(f.read())
        prog = os.path.join(tmp, "conv_host_check")
        subprocess.run([HIPCC, *FLAGS, "conv_host_check.cpp", "-o", prog], cwd=csrc, check=True)
        out = subprocess.run([prog], capture_output=True, text=True).stdout       # (exit status 1 where REV fails the refused-rows cases)
    lines, changed = [], [0] * len(EXPECTED)
    for line in out.splitlines():
        if line.startswith(("FAILED", "conv host check:")):                       # the direct assertions are not records
            continue
        for k, (entry, pat, rep, _) in enumerate(EXPECTED):
            if line.startswith(entry):
                line, n = re.subn(pat, rep, line)
                changed[k] += n
        lines.append(line)
    with open(GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{GOLDEN}: {len(lines)} lines from {sys.argv[1]}")
    for (entry, _, _, why), n in zip(EXPECTED, changed):
        print(f"  expected difference applied to {n} argument blocks of {entry}*: {why}")


if __name__ == "__main__":
    main()
