"""The launch records of the 3-D and volume entries (csrc/vol_host_check.cpp) against tests/golden/vol_launch_records.txt.

The program includes csrc/conv3d.hip and csrc/volume_ops.hip with the launch macro redefined to a recorder
(csrc/host_check_record.hpp), calls every extern "C" entry of the two files over a table of cases and prints, per case, the return
code and every launch: kernel instantiation, grid, block and each by-value argument field by field.  It is compiled for the host only
under the address / undefined-behaviour sanitizers and with pattern-initialised automatic variables, runs as a program of its own and
touches no GPU.  The GPU tests cannot see what this pins: the 4- and 8-planes forms of the 1 -> 8 / 8 -> 1 kernels, the planes per
thread and the dense / strided weight rows of the general 3-D kernel, and the register and generic soft-argmin kernels are bitwise
equal by design, and a sample stride in the wrong slot of a batch of one changes nothing.

The golden file is the program's output on the host code as it was before the entries took the filler-and-launcher form:
tools/conv_launch_golden.py vol REV.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "effi_mvs_plus_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vol_launch_records.txt")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vol_host_check"))
    r = subprocess.run(["make", "-C", CSRC, f"HOST_CHECK_DIR={out}", "vol_host_check"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return os.path.join(out, "vol_host_check")


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"line {i + 1}:\n  got  {g}\n  want {w}"
    return f"{len(got)} lines, want {len(want)}"


def test_launch_records_match_golden(program):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EFFI_")}      # (the program has its own option table anyway)
    r = subprocess.run([program], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = r.stdout.splitlines()
    want = open(GOLDEN).read().splitlines()
    assert len(want) > 900 and sum(" || " in line for line in want) > 400
    assert not any("0xaa" in line.lower() for line in got), "an argument field was left unset"
    assert got == want, first_difference(got, want)
