"""The weight layouts and the blob reader of csrc/backbone_pack.h, checked on the CPU.

tests/host/pack_check.cpp is a stand-alone program (its own main, no HIP): it walks every packed image in the order the kernel
reads it and feeds the blob reader well-formed and hostile blobs.  This test compiles it for the host with the ROCm clang++ (g++
does not take _Float16 in C++) and runs it.
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


def test_every_layout_and_the_blob_reader(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ next to hipcc")
    exe = tmp_path / "pack_check"
    subprocess.run([str(cxx), "-std=c++17", "-O1", "-o", str(exe), str(ROOT / "tests" / "host" / "pack_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "all checks passed" in run.stdout
