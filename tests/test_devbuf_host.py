"""The owned device buffer of csrc/device_mem.h (DevBuf), checked on the CPU.

tests/host/devbuf_check.cpp is a stand-alone program (its own main, no GPU): it instantiates DevBuf with a counting allocator on
malloc / free that can fail a chosen request, and checks the rules every owner of device memory in the library relies on: no
growth at or below the capacity, free-first growth, the slack, empty after a failure, build-then-replace, moves and vectors free
every block exactly once.  This test compiles it for the host with the ROCm clang++ and the address and undefined-behaviour
sanitizers, and runs it directly.
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


def test_devbuf_ownership_rules(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no ROCm clang++ next to hipcc")
    rocm_include = Path(cxx).parent.parent.parent / "include"
    exe = tmp_path / "devbuf_check"
    subprocess.run([str(cxx), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I", str(rocm_include), "-o", str(exe),
                    str(ROOT / "tests" / "host" / "devbuf_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "all checks passed" in run.stdout
