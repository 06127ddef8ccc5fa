#!/usr/bin/env python3
"""Regenerate a golden file of launch records: the output of a host check program on the sources of ANOTHER revision.

Usage: tools/conv_launch_golden.py CHECK REV
    CHECK   conv: csrc/conv_host_check.cpp -> tests/golden/conv_launch_records.txt
            warp: csrc/warp_host_check.cpp -> tests/golden/warp_launch_records.txt
            vol:  csrc/vol_host_check.cpp  -> tests/golden/vol_launch_records.txt
    REV     the commit whose host code is the reference, e.g. the parent of a refactor

The csrc/ and include/ of REV are extracted into a temporary directory, THIS tree's check program (the case table) and recorder
(host_check_record.hpp) are put beside them, and the program is built for the host only with -ftrivial-auto-var-init=zero, so that an
argument field REV's entries leave unset reads as zero (the tree under test is built with =pattern: csrc/Makefile).  Its output, with
the differences listed in the check's EXPECTED applied, becomes the golden file.  Needs hipcc; touches no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ("--offload-host-only -O1 -std=c++17 -ffp-contract=off -Wno-unused-function -fsanitize=address,undefined "
         "-fno-sanitize-recover=undefined -ftrivial-auto-var-init=zero -Wl,--unresolved-symbols=ignore-all -x hip").split()
RECORDER = "host_check_record.hpp"

# Per check: EXPECTED lists the differences from REV's records that are meant: (entry prefix, pattern, replacement, why).
CHECKS = {
    "conv": [
        ("effi_conv3d_k3s1_bf16x3_f32", r" zcount=(\d+) hin=", r" zcount=\1 zin=\1 hin=",
         "the z-batched split 3-D entry left zin unset (no kernel of its launcher reads it); conv_volume sets zin = D for every volume"),
    ],
    "warp": [],
    # effi_planar_to_nhwc_f32 left the slots past n of its two pointer lists and the view-table pointer of the first unset (the kernel
    # reads slot blockIdx.y < n only, and never the table); they are null now.  Null is what the zero-initialised build of REV
    # prints for them, so the records need no replacement.
    "vol": [],
}


def main():
    if len(sys.argv) != 3 or sys.argv[1] not in CHECKS:
        sys.exit(__doc__)
    check, rev = sys.argv[1:]
    expected = CHECKS[check]
    program = f"{check}_host_check"
    golden = os.path.join(ROOT, "tests", "golden", f"{check}_launch_records.txt")
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "effi_mvs_plus_amd/csrc", "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
        csrc = os.path.join(tmp, "effi_mvs_plus_amd", "csrc")
        for name in (program + ".cpp", RECORDER):
            with open(os.path.join(ROOT, "effi_mvs_plus_amd", "csrc", name)) as f, open(os.path.join(csrc, name), "w") as g:
                g.write(f.read())
        prog = os.path.join(tmp, program)
        subprocess.run([HIPCC, *FLAGS, program + ".cpp", "-o", prog], cwd=csrc, check=True)
        out = subprocess.run([prog], capture_output=True, text=True).stdout       # (exit status 1 where REV fails a direct assertion)
    lines, changed = [], [0] * len(expected)
    for line in out.splitlines():
        if line.startswith(("FAILED", f"{check} host check:")):                   # the direct assertions are not records
            continue
        for k, (entry, pat, rep, _) in enumerate(expected):
            if line.startswith(entry):
                line, n = re.subn(pat, rep, line)
                changed[k] += n
        lines.append(line)
    with open(golden, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{golden}: {len(lines)} lines from {rev}")
    for (entry, _, _, why), n in zip(expected, changed):
        print(f"  expected difference applied to {n} argument blocks of {entry}*: {why}")


if __name__ == "__main__":
    main()
