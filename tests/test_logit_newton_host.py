"""The host half of logit calibration (csrc/logit_newton.h), checked on the CPU.

tests/host/logit_newton_check.cpp is a stand-alone program (its own main, no HIP): the in-tree Cholesky on a known and on a singular
matrix, the identity damping, the three modes' reductions against hand-computed values, the frozen-class mask, and a whole fit on a
12-row problem whose sums it computes itself.  This test compiles it for the host with the ROCm clang++ and runs it.
"""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _clangxx():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cxx = Path(hipcc).resolve().parent.parent / "llvm" / "bin" / "clang++"
    return cxx if cxx.is_file() else None


def test_cholesky_reductions_mask_and_a_full_fit(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ next to hipcc")
    exe = tmp_path / "logit_newton_check"
    subprocess.run([str(cxx), "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "host" / "logit_newton_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "all checks passed" in run.stdout
