"""csrc/demc_geometry.hpp -- the arithmetic that turns (configuration, model shape, device facts) into kernel instance, grid,
workgroup size, LDS bytes, chunk counts and fuse flags -- is host-only code: tests/geometry_host.cpp, a program of its own, calls it
against the project's own statements (the rules' comments, the docstring of test_gpu_instance_selection.py) and
against brute force written by other means.  Built with the address and undefined-behaviour sanitizers and run once.  No GPU, no HIP
runtime, and no ROCm include path: that the program compiles is the proof that the header is host-only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")


def test_launch_geometry_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "geometry_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                            os.path.join(ROOT, "tests", "geometry_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "geometry ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr


def test_launch_geometry_is_written_in_the_host_only_header():
    """demc_geometry.hpp knows no HIP, no device allocation and no handle; the runtime keeps no rule of its own: the side channel
    of the tail flags is gone, the chunk and lane rules are defined in the header only, and each launch path plans exactly once."""
    geometry = open(os.path.join(CSRC, "demc_geometry.hpp")).read()
    for word in ("hip", "ALLOC", "demc_handle"):
        assert word not in geometry, word
    runtime = open(os.path.join(CSRC, "demc_hip.cpp")).read()
    assert "tf_cheap_obs" not in runtime
    for name in ("chunks_filling_rounds", "resident_lpp"):  # (defined in the header, not even named in the runtime)
        assert name not in runtime and ("inline int %s(" % name) in geometry, name
    for call in ("plan_phase(", "plan_loglike("):
        assert runtime.count(call) == 1, call
