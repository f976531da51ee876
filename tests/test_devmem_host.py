"""The move-only owners of csrc/demc_devmem.hpp (DevBuf, PinnedBuf, Event, Module, Scratch) release what they hold exactly once,
and the end of a call (finish) and the pass timer of the diagnostic variant (PassTrace) do what they say: tests/devmem_host.cpp -- a
program of its own, HIP stubbed by counters over malloc / free -- is built with the address and undefined-behaviour sanitizers and
run.  No GPU, no HIP runtime."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_owners_release_exactly_once_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None or not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("needs g++ and the ROCm headers")
    exe = str(tmp_path / "devmem_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                            os.path.join(ROOT, "tests", "devmem_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "devmem owners ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr
    # the pass timer of the diagnostic variant: the line tools/quantile_bench.py and tools/cov_bench.py read
    assert run.stderr.splitlines() == ["devmem_host consecutive pass_ms 2.0000 3.0000 4.0000", "devmem_host pairs pass_ms 2.0000 4.0000"], run.stderr


def test_releases_are_written_in_one_place():
    """hipFree, hipHostFree and hipModuleUnload occur in demc_devmem.hpp alone; hipEventDestroy there and where the runtime empties
    its pool of recycled timing events; hiprtc compiles in one place"""
    seen = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cpp", ".hpp")):
            txt = open(os.path.join(CSRC, f)).read()
            for call in ("hipFree(", "hipHostFree(", "hipModuleUnload(", "hipEventDestroy(", "hiprtcCompileProgram("):
                if txt.count(call):
                    seen.setdefault(call, {})[f] = txt.count(call)
    for call in ("hipFree(", "hipHostFree(", "hipModuleUnload("):
        assert seen[call] == {"demc_devmem.hpp": 1}, (call, seen[call])
    assert seen["hipEventDestroy("] == {"demc_devmem.hpp": 1, "demc_hip.cpp": 1}, seen["hipEventDestroy("]
    assert seen["hiprtcCompileProgram("] == {"demc_hip.cpp": 1}, seen["hiprtcCompileProgram("]
