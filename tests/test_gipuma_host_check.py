"""The stand-alone sanitizer program of the Gipuma fusion kernel (csrc/gipuma_host_check.cpp): built for the host only with
-fsanitize=address,undefined, it runs every thread of the launch grid -- the kernel's own body, csrc/gipuma_pixel.hpp -- as a loop over
exactly sized host arrays.  An out-of-bounds used[s][q] store, the one way this kernel could fault a GPU, is a heap overflow here.
It is a program of its own and touches no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "effi_mvs_plus_amd", "csrc")


def test_gipuma_host_check_builds_and_passes(tmp_path):
    out = str(tmp_path)
    r = subprocess.run(["make", "-C", CSRC, f"HOST_CHECK_DIR={out}", "gipuma_host_check"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    r = subprocess.run([os.path.join(out, "gipuma_host_check")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "gipuma host check: ok"
