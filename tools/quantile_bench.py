#!/usr/bin/env python3
"""Times demc_quantiles (posterior quantiles on the device) against the path it replaces -- demc_export_chains of
the same rows and np.quantile per series, chains pooled -- on the same handle, at two sizes: the Gaussian example's (4 groups x 6
particles, D = 2) and 64 x 64 chains with D = 32 (MvNormal, full covariance), 1000 kept rows each, the default five probs.

    python3 tools/quantile_bench.py [--rows 1000] [--repeats 5] [--limit 300]

Each size runs in a process of its own under a time limit (`--limit` seconds); a size that runs into it is reported as such and the
other still runs.  Prints one JSON object per size: wall-clock ms of demc_quantiles (median / min / max over the repeats, after one
warm-up call), of the export alone and of np.quantile on the exported array, the device time of each of the eight histogram passes
(one further call in a process of its own on the diagnostic variant of the library, `make TRACE=1 OUT=../libdemc_hip_trace.so`,
which brackets every k_q_hist launch with events and prints the times to stderr; TRACE_PREBUILT=1: the variant is there already),
the bytes either path moves to the host, and whether the device's table equals chains.series_quantiles bit for bit."""
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
    """a handle of the size `name` with `rows` rows of history"""
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


def one(name, rows, repeats):
    from demc_amd.chains import DEFAULT_QUANTILES, series_quantiles
    d, P = SIZES[name]["D"], SIZES[name]["G"] * SIZES[name]["Np"]
    e = engine(name, rows)
    try:
        e.quantiles(0, rows, DEFAULT_QUANTILES)  # warm-up: the first launch of each kernel
        dev = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = e.quantiles(0, rows, DEFAULT_QUANTILES)
            dev.append((time.perf_counter() - t0) * 1e3)
        e.export_chains(0, min(rows, 2))
        exp = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            value = e.export_chains(0, rows)
            exp.append((time.perf_counter() - t0) * 1e3)
    finally:
        e.close()
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        host_np = np.stack([np.quantile(value[:, j, :].reshape(-1), DEFAULT_QUANTILES, method="linear") for j in range(d + 2)])
    t_np = (time.perf_counter() - t0) * 1e3
    ref = np.stack([series_quantiles(value[:, j, :], DEFAULT_QUANTILES) for j in range(d + 2)])
    same = bool(np.array_equal(np.isnan(out), np.isnan(ref)) and np.array_equal(out[~np.isnan(out)].view(np.uint64), ref[~np.isnan(ref)].view(np.uint64)))
    fin = np.isfinite(host_np) & np.isfinite(out)
    med = float(np.median(dev))
    return dict(size=name, chains=P, D=d, rows=rows, repeats=repeats, quantiles_ms_median=med, quantiles_ms_min=float(min(dev)),
                quantiles_ms_max=float(max(dev)), export_ms_median=float(np.median(exp)), np_quantile_ms=t_np,
                parent_path_ms=float(np.median(exp)) + t_np, speedup=(float(np.median(exp)) + t_np) / med,
                bytes_to_host_device_path=int(out.nbytes), bytes_to_host_export=int(value.nbytes), bits_equal_host_definition=same,
                max_abs_diff_np_quantile=float(np.abs(out[fin] - host_np[fin]).max()) if fin.any() else None,
                method="wall clock around each call (the calls drain the stream), one handle, same rows")


def traced(name, rows):
    """one call on the diagnostic variant of the library: its pass times go to stderr, where the parent reads them"""
    csrc = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
    if os.environ.get("TRACE_PREBUILT") != "1":  # (build here and ship the library to the GPU box: TRACE_PREBUILT=1 skips the make)
        subprocess.check_call(["make", "-B", "-j8", "-C", csrc, "-s", "TRACE=1", "OUT=../libdemc_hip_trace.so"], stdout=sys.stderr)
    import demc_amd
    demc_amd._ffi.LIB_PATH = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "libdemc_hip_trace.so")
    from demc_amd.chains import DEFAULT_QUANTILES
    e = engine(name, rows)
    try:
        e.quantiles(0, rows, DEFAULT_QUANTILES)
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds each size may take")
    ap.add_argument("--size", choices=sorted(SIZES), help="(internal) run this size in this process")
    ap.add_argument("--traced", choices=sorted(SIZES), help="(internal) one call of this size on the diagnostic variant, in this process")
    o = ap.parse_args()
    if o.size:
        print(json.dumps(one(o.size, o.rows, o.repeats)))
        return 0
    if o.traced:
        traced(o.traced, o.rows)
        return 0
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
        try:  # the timed calls above ran on the product library; the variant serves this one call
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--traced", name, "--rows", str(o.rows)], timeout=o.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(size=name, error=f"time limit of {o.limit} s (traced call)")))
            return 124
        if r.returncode != 0:
            print(json.dumps(dict(size=name, error=f"exit status {r.returncode} (traced call)", stderr=r.stderr[-2000:])))
            return r.returncode
        passes = [ln for ln in r.stderr.splitlines() if ln.startswith("demc_quantiles pass_ms")]
        res["hist_pass_ms"] = [float(x) for x in passes[-1].split()[2:]] if passes else None
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
