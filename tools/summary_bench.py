#!/usr/bin/env python3
"""Times demc_summarize (chain summaries on the device) against the path it replaces -- demc_export_chains of the
same rows, Chains.describe() and the host's Chains.summarystats() -- on the same handle, at two sizes: the Gaussian example's
(4 groups x 6 particles, D = 2) and 64 x 64 chains with D = 32 (MvNormal, full covariance), 1000 kept rows each.

    python3 tools/summary_bench.py [--rows 1000] [--repeats 5] [--limit 300]

Each size runs in a process of its own under a time limit (`--limit` seconds); a size that runs into it is reported as such and the
other still runs.  Prints one JSON object per size: wall-clock ms of demc_summarize (median / min / max over the repeats, after one
warm-up call), of the export alone, of describe() and of summarystats() on the exported array, the bytes either path moves to the
host, and the largest relative difference between the device's and the host's columns."""
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


def one(name, rows, repeats):
    import demc_amd as D
    from demc_amd import families as F
    s = SIZES[name]
    G, Np, d = s["G"], s["Np"], s["D"]
    P = G * Np
    rng = np.random.default_rng(50514)
    e = D.HipEngine(n_groups=G, Np=Np, D=d, n_rows=rows, seed=2024, burnin=0, schedule=2)
    try:
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
        e.summarize(0, rows)  # warm-up: the first launch of each kernel
        dev = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out, _ = e.summarize(0, rows)
            dev.append((time.perf_counter() - t0) * 1e3)
        e.export_chains(0, min(rows, 2))
        exp = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            value = e.export_chains(0, rows)
            exp.append((time.perf_counter() - t0) * 1e3)
    finally:
        e.close()
    names = [f"p{j}" for j in range(d)] + ["acceptance", "lp"]
    ch = D.Chains(value, names, names[:-2])
    t0 = time.perf_counter()
    ch.describe()
    t_desc = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = ch.summarystats()
    t_stats = (time.perf_counter() - t0) * 1e3
    with np.errstate(all="ignore"):
        rel = np.abs(out[:, :5] - host.values[:, :5]) / np.abs(host.values[:, :5])
    med = float(np.median(dev))
    return dict(size=name, chains=P, D=d, rows=rows, repeats=repeats, summarize_ms_median=med, summarize_ms_min=float(min(dev)),
                summarize_ms_max=float(max(dev)), export_ms_median=float(np.median(exp)), describe_ms=t_desc, summarystats_ms=t_stats,
                parent_path_ms=float(np.median(exp)) + t_desc + t_stats, speedup=(float(np.median(exp)) + t_desc + t_stats) / med,
                bytes_to_host_device_path=int(out.nbytes), bytes_to_host_export=int(value.nbytes),
                max_rel_diff=float(np.nanmax(rel)), pairs_equal=bool(np.array_equal(out[:, 5], host.values[:, 5])),
                method="wall clock around each call (the calls drain the stream), one handle, same rows")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds each size may take")
    ap.add_argument("--size", choices=sorted(SIZES), help="(internal) run this size in this process")
    o = ap.parse_args()
    if o.size:
        print(json.dumps(one(o.size, o.rows, o.repeats)))
        return 0
    rc = 0
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
        print(r.stdout.strip().splitlines()[-1])
    return rc


if __name__ == "__main__":
    sys.exit(main())
