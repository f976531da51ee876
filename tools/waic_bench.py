#!/usr/bin/env python3
"""Times demc_waic (WAIC on the device) at two sizes: cfg5's share -- LBA with 3 accumulators, N = 50 000 trials, 4 096
chains, 100 history rows -- and a Gaussian with N = 100 000 observations on the same 4 096 x 100 draws.  The host route this call
replaces (the family's density rewritten in numpy, S x N evaluations, an S x N matrix of tens of gigabytes) cannot run at these
sizes; its cheapest part, demc_export_chains of the same rows, is timed beside the call for comparison.

    python3 tools/waic_bench.py [--rows 100] [--repeats 5] [--limit 400]

Each size runs in a process of its own under a time limit (`--limit` seconds), on the diagnostic variant of the library (`make
TRACE=1 OUT=../libdemc_hip_trace.so`; TRACE_PREBUILT=1: the variant is there already), which brackets the three passes of the call
-- k_pw_prepare, k_pw_accumulate, k_pw_final with k_pw_totals -- with events on the handle's stream and prints their device times
to stderr.  After one warm-up call the runs alternate: demc_waic, demc_export_chains, demc_waic, ...  Prints one JSON object per
size: the median / min / max over the repeats of the device time of the call (the sum of its passes, by the events) and of its wall
clock, the export's wall clock, density evaluations per second, and for the LBA the FP64 rate in executed flop per evaluation as
tools/count_lba_flop.py counted them (profiles/<round>/lba_inner_loop.json) against the FP64 vector peak."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"lba_cfg5_share": dict(N=50000, G=256, Np=16), "gaussian_1e5": dict(N=100000, G=256, Np=16)}
PEAK_FP64_TFLOPS = 78.6  # MI355X FP64 vector peak (bench.py)


def engine(name, rows):
    """a handle of the size `name` whose history holds `rows` rows of posterior-like draws (nothing is stepped)"""
    import demc_amd as D
    from demc_amd import families as F
    s = SIZES[name]
    N, G, Np = s["N"], s["G"], s["Np"]
    P = G * Np
    rng = np.random.default_rng(50514)
    if name == "lba_cfg5_share":
        nu, A, k, tau = np.array([3.0, 2.0, 1.0]), 0.8, 0.2, 0.3
        choice, rt = np.empty(N), np.empty(N)
        for i in range(N):  # Run_LBA.jl's simulator: drifts redrawn until one is positive
            while True:
                v = rng.normal(nu, 1.0)
                if (v > 0).any():
                    break
            t = (A + k - rng.uniform(0, A, 3)) / np.where(v > 0, v, np.nan)
            choice[i], rt[i] = np.nanargmin(t) + 1, np.nanmin(t) + tau
        e = D.HipEngine(n_groups=G, Np=Np, D=6, n_rows=rows, seed=2024, burnin=0, schedule=2)
        e.set_model(F.FAM_LBA, np.concatenate([choice, rt]), [N, 3])
        e.set_bounds([0.0] * 6, [np.inf] * 5 + [rt.min()])
        centre, spread = np.array([3.0, 2.0, 1.0, 0.8, 0.2, 0.3]), np.array([0.05, 0.05, 0.05, 0.02, 0.01, 0.005])
    else:
        x = rng.normal(0.3, 1.2, N)
        e = D.HipEngine(n_groups=G, Np=Np, D=2, n_rows=rows, seed=2024, burnin=0, schedule=2)
        e.set_model(F.FAM_GAUSSIAN, x, [N])
        e.set_bounds([-np.inf, 0.0], [np.inf, np.inf])
        centre, spread = np.array([x.mean(), x.std()]), np.array([0.004, 0.003])
    for r in range(rows):
        e.set_history_rows(r, centre + spread * rng.normal(0, 1, (1, P, len(centre))))
    return e


def one(name, rows, repeats):
    csrc = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
    if os.environ.get("TRACE_PREBUILT") != "1":  # (build here and ship the library to the GPU box: TRACE_PREBUILT=1 skips the make)
        subprocess.check_call(["make", "-B", "-j8", "-C", csrc, "-s", "TRACE=1", "OUT=../libdemc_hip_trace.so"], stdout=sys.stderr)
    import demc_amd
    demc_amd._ffi.LIB_PATH = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "libdemc_hip_trace.so")
    e = engine(name, rows)
    wall, exp = [], []
    try:
        tot, _ = e.waic(0, rows)  # warm-up: the first launch of each kernel
        e.export_chains(0, min(rows, 2))
        sys.stderr.write("timed runs\n")
        for _ in range(repeats):  # alternating
            t0 = time.perf_counter()
            tot, _ = e.waic(0, rows)
            wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            value = e.export_chains(0, rows)
            exp.append((time.perf_counter() - t0) * 1e3)
    finally:
        e.close()
    s = SIZES[name]
    S = rows * s["G"] * s["Np"]
    return dict(size=name, N=s["N"], chains=s["G"] * s["Np"], rows=rows, draws=S, evaluations=S * s["N"], repeats=repeats,
                waic_wall_ms_median=float(np.median(wall)), waic_wall_ms_min=float(min(wall)), waic_wall_ms_max=float(max(wall)),
                export_ms_median=float(np.median(exp)), export_bytes=int(value.nbytes), matrix_bytes_host_route=int(8 * S * s["N"]),
                totals=dict(zip(demc_amd.chains.WAIC_TOTALS, (float(v) for v in tot))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=400.0, help="seconds each size may take")
    ap.add_argument("--size", choices=sorted(SIZES), help="(internal) run this size in this process")
    o = ap.parse_args()
    if o.size:
        print(json.dumps(one(o.size, o.rows, o.repeats)))
        return 0
    flop = None
    try:
        import bench
        flop = json.load(open(os.path.join(ROOT, "profiles", bench.PROFILE_ROUND, "lba_inner_loop.json")))["fp64_flop_per_eval"]
    except (OSError, ValueError, KeyError, ImportError):
        pass
    for name in SIZES:  # a fresh process per size, each under its own limit; a GPU fault or a time-out ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", name, "--rows", str(o.rows), "--repeats", str(o.repeats)],
                               timeout=o.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(size=name, error=f"time limit of {o.limit} s")))
            return 124
        if r.returncode != 0:
            print(json.dumps(dict(size=name, error=f"exit status {r.returncode}", stderr=r.stderr[-2000:])))
            return r.returncode
        res = json.loads(r.stdout.strip().splitlines()[-1])
        err = r.stderr.splitlines()
        timed = err[err.index("timed runs") + 1:] if "timed runs" in err else err
        passes = [[float(x) for x in ln.split()[2:]] for ln in timed if ln.startswith("demc_waic pass_ms")]
        if passes:
            dev = [sum(p) for p in passes]
            med = float(np.median(dev))
            res.update(waic_device_ms_median=med, waic_device_ms_min=float(min(dev)), waic_device_ms_max=float(max(dev)),
                       pass_ms_median=dict(zip(("prepare", "accumulate", "final_totals"), (float(v) for v in np.median(np.array(passes), axis=0)))),
                       evaluations_per_second=res["evaluations"] / (med * 1e-3), export_over_waic=res["export_ms_median"] / med,
                       method="events on the handle's stream around the three passes (the diagnostic variant), median of runs alternating with the export")
            if name == "lba_cfg5_share" and flop:
                tf = res["evaluations"] * flop / (med * 1e-3) / 1e12
                res.update(fp64_flop_per_eval=flop, fp64_TFLOPs=tf, fp64_peak_fraction=tf / PEAK_FP64_TFLOPS)
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
