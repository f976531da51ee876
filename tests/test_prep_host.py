"""csrc/demc_prep.hpp -- what the set-model, set-priors, set-bounds and set-blocks entry points work out before anything is
uploaded -- is host-only code: tests/prep_host.cpp, a program of its own, calls it against values formed by other means (integer
arithmetic, restated definitions, long double) and reads back every refusal's code and text.  Built with the address and
undefined-behaviour sanitizers and run once.  No GPU, no HIP runtime, and no ROCm include path: that the program compiles is the
proof that the header is host-only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")


def test_model_and_prior_preparation_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "prep_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                            os.path.join(ROOT, "tests", "prep_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)  # (the error of truncnormal_log_mass per case, and the largest)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "prep ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr


def test_preparation_is_written_in_the_host_only_header():
    """demc_prep.hpp knows no HIP, no device allocation and no handle; the arithmetic that moved there is not restated in the
    runtime.  (Two refusals of demc_set_model_sim quote the C-ABI's parameter `hip_source` by name: the messages are the parent's,
    byte for byte, so that word alone is taken out before the header is searched.)"""
    prep = open(os.path.join(CSRC, "demc_prep.hpp")).read()
    assert prep.count("hip_source") == 2
    prep = prep.replace("hip_source", "")
    for word in ("hip", "ALLOC", "demc_handle"):
        assert word not in prep, word
    runtime = open(os.path.join(CSRC, "demc_hip.cpp")).read()
    for call in ("std::lgamma(", "std::stable_sort(", "std::erfc("):
        assert call not in runtime, call
    for call in ("prepare_model(", "prepare_sim(", "prepare_priors(", "prepare_bounds(", "encode_segments(", "encode_mask("):
        assert runtime.count(call) == 1, call
