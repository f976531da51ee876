#!/usr/bin/env python3
"""Times demc_covariance (posterior covariance and correlation on the device) against the path it replaces --
demc_export_chains of the same rows and chains.series_cov on the host -- on the same handle, at two sizes: the Gaussian example's
(4 groups x 6 particles, D = 2) and 64 x 64 chains with D = 32 (MvNormal, full covariance), 1000 kept rows each, all D + 2 series.

    python3 tools/cov_bench.py [--rows 1000] [--repeats 5] [--limit 300]

Each size runs in a process of its own under a time limit (`--limit` seconds); a size that runs into it is reported as such and the
other still runs.  Prints one JSON object per size: wall-clock ms of demc_covariance (median / min / max over the repeats, after one
warm-up call), of the export alone and of series_cov on the exported array, the device time of the three stages (one further call
in a process of its own on the diagnostic variant of the library, `make TRACE=1 OUT=../libdemc_hip_trace.so`, which brackets pass 1,
pass 2 and the final kernel with events and prints the times to stderr; TRACE_PREBUILT=1: the variant is there already), the
history bytes per second and the FP64 rate of pass 2, the bytes either path moves to the host, and the largest scaled difference
between the device's matrices and the host function's."""
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
    from demc_amd.chains import series_cov
    d, P = SIZES[name]["D"], SIZES[name]["G"] * SIZES[name]["Np"]
    e = engine(name, rows)
    try:
        e.covariance(0, rows)  # warm-up: the first launch of each kernel
        dev = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = e.covariance(0, rows)
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
    ref = series_cov(value)
    t_host = (time.perf_counter() - t0) * 1e3
    N = rows * P
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.diag(ref[1]))
        scale = sd[:, None] * sd[None, :]
        ok = np.isfinite(ref[1]) & (scale > 0)
        d_cov = float(np.max(np.abs(out[1] - ref[1])[ok] / scale[ok])) if ok.any() else None
        okr = np.isfinite(ref[2])
        d_cor = float(np.max(np.abs(out[2] - ref[2])[okr])) if okr.any() else None
    med = float(np.median(dev))
    return dict(size=name, chains=P, D=d, K=d + 2, rows=rows, cells=N, repeats=repeats, covariance_ms_median=med, covariance_ms_min=float(min(dev)),
                covariance_ms_max=float(max(dev)), export_ms_median=float(np.median(exp)), series_cov_ms=t_host,
                parent_path_ms=float(np.median(exp)) + t_host, speedup=(float(np.median(exp)) + t_host) / med,
                bytes_to_host_device_path=int(sum(a.nbytes for a in out)), bytes_to_host_export=int(value.nbytes),
                history_bytes_per_pass=int(N * (8 * d + 1 + 8)), same_nan_pattern=bool(all(np.array_equal(np.isnan(a), np.isnan(b)) for a, b in zip(out, ref))),
                max_scaled_cov_diff_host=d_cov, max_cor_diff_host=d_cor,
                method="wall clock around each call (the calls drain the stream), one handle, same rows")


def traced(name, rows):
    """one call on the diagnostic variant of the library: its stage times go to stderr, where the parent reads them"""
    csrc = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
    if os.environ.get("TRACE_PREBUILT") != "1":  # (build here and ship the library to the GPU box: TRACE_PREBUILT=1 skips the make)
        subprocess.check_call(["make", "-B", "-j8", "-C", csrc, "-s", "TRACE=1", "OUT=../libdemc_hip_trace.so"], stdout=sys.stderr)
    import demc_amd
    demc_amd._ffi.LIB_PATH = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "libdemc_hip_trace.so")
    e = engine(name, rows)
    try:
        e.covariance(0, rows)
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
        stages = [ln for ln in r.stderr.splitlines() if ln.startswith("demc_covariance pass_ms")]
        if stages:
            ms = [float(x) for x in stages[-1].split()[2:]]
            res["stage_ms"] = dict(mean=ms[0], syrk=ms[1], final=ms[2])
            nb = -(-res["K"] // 16)
            flop = 2.0 * 16 * 16 * 4 * (nb * (nb + 1) // 2) * -(-res["cells"] // 4)  # every MFMA of pass 2: 2 * 16 * 16 * 4 each
            res["syrk_history_GBps"] = res["history_bytes_per_pass"] / (ms[1] * 1e-3) / 1e9 if ms[1] > 0 else None
            res["syrk_matrix_TFLOPs"] = flop / (ms[1] * 1e-3) / 1e12 if ms[1] > 0 else None
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
