"""omb_hypervolume / omb_hypervolume_contrib's argument checks (check_hypervolume in optimobo_amd/csrc/omb_host.cpp),
the work cap over hostile headers (check_hv_work: cell products that overflow 64 bits) and the launch sizes under
AddressSanitizer + UBSan: a stand-alone program (tests/asan/omb_hypervolume_check.cpp) built by
`make -C optimobo_amd/csrc asan` and run as it is (CPU, no GPU)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "optimobo_amd", "csrc")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_hypervolume_checks_under_asan_ubsan():
    if not os.path.exists(CLANGXX) or shutil.which("make") is None:
        pytest.skip("needs ROCm's clang++ and make (the build container)")
    r = subprocess.run(["make", "-C", CSRC, "build/asan/omb_hypervolume_check"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([os.path.join(CSRC, "build", "asan", "omb_hypervolume_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 mismatches" in r.stdout and "runtime error" not in r.stderr
