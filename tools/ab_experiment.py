#!/usr/bin/env python3
"""A/B runs of compile-time variants of the library, each built with make EXTRA=-DNAME=value OUT=../<name>.so:
    python3 tools/ab_experiment.py name1.so,name2.so,... -- <bench.py arguments>
(names are library files under differentialevolutionmcmc.jl_amd/) prints ms_per_step and the dominant kernel's launch_ms
for every library."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
libs = sys.argv[1].split(",")
args = sys.argv[sys.argv.index("--") + 1:]
def code_for(lib):
    return ("import sys, runpy; sys.path.insert(0, %r); import demc_amd; "
            "demc_amd._ffi.LIB_PATH = %r; sys.argv = ['bench.py', '--full'] + %r; runpy.run_path(%r, run_name='__main__')"
            % (ROOT, os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", lib), args, os.path.join(ROOT, "bench.py")))


for lib in libs:
    out = subprocess.run([sys.executable, "-c", code_for(lib)], capture_output=True, text=True, timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if not line:
        print(lib, "FAILED", out.stderr[-500:])
        continue
    r = json.loads(line[-1])  # (the compact line is the last one)
    rf = r.get("roofline") or {}
    print(f"{lib:>24}  ms_per_step {r['ms_per_step']:.4f}  launch_ms {rf.get('launch_ms', float('nan')):.4f}  frac {rf.get('frac', float('nan')):.3f}", flush=True)
