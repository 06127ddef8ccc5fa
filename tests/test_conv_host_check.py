"""The launch records of the convolution entries (csrc/conv_host_check.cpp) against tests/golden/conv_launch_records.txt.

The program includes csrc/conv2d.hip and csrc/conv2d_sr.hip with the launch macro redefined to a recorder, calls every extern "C"
convolution entry over a table of cases and prints, per case, the return code and every launch: kernel instantiation, grid, block
and each by-value argument field by field.  It is compiled for the host only under the address / undefined-behaviour sanitizers and
with pattern-initialised automatic variables, runs as a program of its own and touches no GPU.  The GPU tests cannot see what this
pins: every tile form of a layer is bitwise equal by design, so a wrong instantiation or grid passes them.

The golden file is the output of the full-precision build; the build with plain bf16 operands (-DEFFI_BF16_ONLY) has the
split-precision entries only, their names with _bf16 appended, and must print the same records for them.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "effi_mvs_plus_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_launch_records.txt")
MARK = "# split-precision entries"


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conv_host_check"))
    r = subprocess.run(["make", "-j2", "-C", CSRC, f"HOST_CHECK_DIR={out}", "conv_host_check"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return out


def run(path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EFFI_")}      # (the program has its own option table anyway)
    r = subprocess.run([path], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def first_difference(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"line {i + 1}:\n  got  {g}\n  want {w}"
    return f"{len(got)} lines, want {len(want)}"


def test_launch_records_match_golden(programs):
    got = run(os.path.join(programs, "conv_host_check_x3"))
    want = open(GOLDEN).read().splitlines()
    assert len(want) > 300 and any(line.startswith(MARK) for line in want)
    assert got == want, first_difference(got, want)


def test_launch_records_of_the_bf16_build(programs):
    got = [line.replace("_bf16 | ", " | ", 1) for line in run(os.path.join(programs, "conv_host_check_bf16"))]
    want = open(GOLDEN).read().splitlines()
    start = next(i for i, line in enumerate(want) if line.startswith(MARK))
    assert got == want[start:], first_difference(got, want[start:])
