#!/usr/bin/env python3
"""Times demc_hpd (highest-density intervals on the device) against the only route there was before it --
demc_export_chains of the same rows, then Chains.hpd() on the host -- and against one demc_rank_series (one sort of one series) on
the same window, on the same handle, at the two sizes of DESIGN.md 5.5's table: the Gaussian example's (4 groups x 6 particles,
D = 2) and 64 x 64 chains with D = 32 (MvNormal, full covariance), 1000 kept rows each.

    python3 tools/hpd_bench.py [--rows 1000] [--repeats 5] [--limit 600] [--alphas 0.05,0.5]

Each size runs in a process of its own under a time limit (`--limit` seconds).  Prints one JSON object per size: wall-clock ms of
demc_hpd (median / min / max over the repeats, after one warm-up call), of one demc_rank_series, of the export, of Chains.hpd() on
the exported array, the bytes either route moves to the host, whether the two tables are equal bit for bit, and the split between
the sort and the window pass: one further call in a process of its own on the diagnostic variant of the library
(`make TRACE=1 OUT=../libdemc_hip_trace.so`; TRACE_PREBUILT=1: the variant is there already), which brackets the three stages of
every batch with events -- keys, sort, window and final -- and prints the times to stderr."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"gaussian_example": dict(G=4, Np=6, D=2), "mvn_64x64_d32": dict(G=64, Np=64, D=32)}


def engine(name, rows):
    import demc_amd as D
    from demc_amd import families as F
    s = SIZES[name]
    G, Np, d = s["G"], s["Np"], s["D"]
    P = G * Np
    rng = np.random.default_rng(50514)
    e = D.HipEngine(n_groups=G, Np=Np, D=d, n_rows=rows, seed=2024, burnin=0, schedule=2)
    if name == "gaussian_example":
        e.set_model(F.FAM_GAUSSIAN, rng.normal(0.0, 1.0, 50), [50])
        e.set_priors([F.PRIOR_NORMAL, 2], [0.0, 0.0], [1.0, 1.0])
        e.set_bounds([-np.inf, 0.0], [np.inf, np.inf])
        e.set_state(np.stack([rng.normal(0, 0.3, P), rng.uniform(0.8, 1.3, P)], 1))
    else:
        A = rng.normal(0, 1, (d, d))
        Sigma = A @ A.T / d + 0.5 * np.eye(d)
        X = rng.multivariate_normal(rng.normal(0, 1, d), Sigma, 400)
        e.set_model(F.FAM_MVN_FULL, X, [400, d], Sigma)
        e.set_priors([F.PRIOR_NORMAL] * d, [0.0] * d, [1.0] * d)
        e.set_bounds([-np.inf] * d, [np.inf] * d)
        e.set_state(rng.normal(0, 1, (P, d)))
    e.step(1, rows)
    return e


def one(name, rows, repeats, alphas):
    import demc_amd as D
    s = SIZES[name]
    d, P = s["D"], s["G"] * s["Np"]
    e = engine(name, rows)
    try:
        e.hpd(0, rows, alphas)  # warm-up: the first launch of each kernel
        dev = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = e.hpd(0, rows, alphas)
            dev.append((time.perf_counter() - t0) * 1e3)
        e.rank_series(0, rows, 0, 0)
        t0 = time.perf_counter()
        ranks = e.rank_series(0, rows, 0, 0)
        t_series = (time.perf_counter() - t0) * 1e3
        e.export_chains(0, min(rows, 2))
        exp = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            value = e.export_chains(0, rows)
            exp.append((time.perf_counter() - t0) * 1e3)
    finally:
        e.close()
    t0 = time.perf_counter()
    host = np.stack([D.chains.series_hpd(value[:, j, :], alphas) for j in range(d + 2)])
    t_host = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(np.isnan(out), np.isnan(host)) and np.array_equal(out[~np.isnan(out)].view(np.uint64), host[~np.isnan(host)].view(np.uint64)))
    med = float(np.median(dev))
    return dict(size=name, chains=P, D=d, rows=rows, repeats=repeats, alphas=list(alphas), hpd_ms_median=med, hpd_ms_min=float(min(dev)),
                hpd_ms_max=float(max(dev)), rank_series_ms=t_series, export_ms_median=float(np.median(exp)), host_hpd_ms=t_host,
                parent_path_ms=float(np.median(exp)) + t_host, speedup=(float(np.median(exp)) + t_host) / med,
                bytes_to_host_device_path=int(out.nbytes), bytes_to_host_rank_series=int(ranks.nbytes), bytes_to_host_export=int(value.nbytes),
                tables_equal_bit_for_bit=same,
                method="wall clock around each call (the calls drain the stream), one handle, same rows")


def traced(name, rows, alphas):
    """one call on the diagnostic variant of the library: its stage times go to stderr, where the parent reads them"""
    csrc = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
    if os.environ.get("TRACE_PREBUILT") != "1":  # (build here and ship the library to the GPU box: TRACE_PREBUILT=1 skips the make)
        subprocess.check_call(["make", "-B", "-j8", "-C", csrc, "-s", "TRACE=1", "OUT=../libdemc_hip_trace.so"], stdout=sys.stderr)
    import demc_amd
    demc_amd._ffi.LIB_PATH = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "libdemc_hip_trace.so")
    e = engine(name, rows)
    try:
        e.hpd(0, rows, alphas)
        e.hpd(0, rows, alphas)
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=600.0, help="seconds each size may take")
    ap.add_argument("--alphas", default="0.05", help="comma-separated alphas of every call")
    ap.add_argument("--size", choices=sorted(SIZES), help="(internal) run this size in this process")
    ap.add_argument("--traced", choices=sorted(SIZES), help="(internal) two calls of this size on the diagnostic variant, in this process")
    o = ap.parse_args()
    alphas = tuple(float(a) for a in o.alphas.split(","))
    if o.size:
        print(json.dumps(one(o.size, o.rows, o.repeats, alphas)))
        return 0
    if o.traced:
        traced(o.traced, o.rows, alphas)
        return 0
    for name in SIZES:  # a fresh process per step, each under its own limit; a GPU fault or a time-out ends the run
        steps = [["--size", name, "--repeats", str(o.repeats)], ["--traced", name]]
        res = None
        for extra in steps:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(o.rows), "--alphas", o.alphas] + extra, timeout=o.limit,
                                   capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(size=name, error=f"time limit of {o.limit} s ({extra[0]})")))
                return 124
            if r.returncode != 0:
                print(json.dumps(dict(size=name, error=f"exit status {r.returncode} ({extra[0]})", stderr=r.stderr[-2000:])))
                return r.returncode
            if extra[0] == "--size":
                res = json.loads(r.stdout.strip().splitlines()[-1])
            else:
                lines = [ln for ln in r.stderr.splitlines() if ln.startswith("demc_hpd pass_ms")]
                ms = [float(x) for x in lines[-1].split()[2:]] if lines else []
                res["stage_ms"] = dict(keys=sum(ms[0::3]), sort=sum(ms[1::3]), window_final=sum(ms[2::3])) if ms else None
                res["window_share"] = sum(ms[2::3]) / sum(ms) if ms else None
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
