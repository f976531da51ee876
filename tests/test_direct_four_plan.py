"""plan_loglike's choice between k_direct_mvn<32> and its four-proposals-per-lane instance k_direct_mvn<32>x4
(csrc/demc_geometry.hpp) is host-only arithmetic: tests/direct_four_plan.cpp, a program of its own, holds it to the headline's
launch (64 x 48, four per lane), to populations that keep the thin workgroups, and -- over a sweep of shapes -- to the chunk
count of the two-per-lane rule, which fixes the sums whichever body runs.  Built with the address and undefined-behaviour
sanitizers and run once.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")


def test_four_per_lane_rule_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "direct_four_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                            os.path.join(ROOT, "tests", "direct_four_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "direct four plan ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr
