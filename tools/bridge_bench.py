#!/usr/bin/env python3
"""Times demc_bridge (the marginal likelihood by bridge sampling on the device) at two sizes -- cfg5's share (LBA, 3
accumulators, N = 50 000 trials, 4 096 chains, 100 history rows = 409 600 draws: the shape of tools/loo_bench.py) and a hierarchical
Gaussian (60 subjects of 100 observations, D = 63, the same 4 096 x 100 draws) -- next to the host route on the same handle:
export_chains of the window, logpost of the same proposal rows P at a time, and the numpy twins of chains.py.

    python3 tools/bridge_bench.py [--rows 100] [--repeats 3] [--limit 500]

Each size runs in a process of its own under a time limit (`--limit` seconds), on the diagnostic variant of the library (`make TRACE=1
OUT=../libdemc_hip_trace.so`; TRACE_PREBUILT=1: the variant is there already), which brackets the stages of the call with events on the
handle's stream and prints their device times to stderr: the transform and the fit (with the host's Cholesky factorisation between
them), the draws and the triangular solve, the two evaluations, the iteration with the error terms.  Prints one JSON object per size:
the median / min / max over the repeats of the wall clock of the call and of the sum of its stages, the median of each stage, and the
wall clock of the host route with its three parts."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import waic_bench as WB  # noqa: E402

SIZES = {"lba_cfg5_share": dict(N=50000, G=256, Np=16, D=6), "hier_gaussian_60x100": dict(N=6000, G=256, Np=16, D=63)}


def engine(name, rows):
    """-> (handle whose history holds `rows` rows of posterior-like draws, lo, hi)"""
    import demc_amd as D
    from demc_amd import families as F
    if name == "lba_cfg5_share":
        e = WB.engine(name, rows)
        lo, hi = [0.0] * 6, [np.inf] * 5 + [0.33]  # (tau of the rows is 0.3 +- 0.005: every draw is inside)
        e.set_bounds(lo, hi)
        return e, lo, hi
    s = SIZES[name]
    S, n, P = 60, 100, s["G"] * s["Np"]
    rng = np.random.default_rng(50515)
    b0 = rng.normal(0, 1, S)
    Y = 1.0 + b0[:, None] + rng.normal(0, 0.5, (S, n))
    Dm = S + 3
    e = D.HipEngine(n_groups=s["G"], Np=s["Np"], D=Dm, n_rows=rows, seed=2024, burnin=0, schedule=2)
    e.set_model(F.FAM_HIER_GAUSSIAN, Y, [S, n])
    e.set_priors([1, 2] + [5] * S + [2], [1, 0] + [0] * S + [0], [1, 1] + [1] * S + [1], [0, 0] + [1] * S + [0])
    lo, hi = [-np.inf, 0] + [-np.inf] * S + [0], [np.inf] * Dm
    e.set_bounds(lo, hi)
    centre = np.concatenate([[1.0, 1.0], Y.mean(axis=1) - 1.0, [0.5]])
    spread = np.concatenate([[0.1, 0.08], np.full(S, 0.05), [0.005]])
    for r in range(rows):
        e.set_history_rows(r, centre + spread * rng.normal(0, 1, (1, P, Dm)))
    return e, lo, hi


def host_route(D, e, rows, lo, hi, prop_theta, lp1):
    """the same estimate without demc_bridge -> (Bridge, dict of the seconds of its parts).  set_history_rows leaves no lp in the history, so
    the lp of the estimate half is handed over (lp1, the device's own): after a real run the export carries it, at no further cost"""
    t = {}
    t0 = time.perf_counter()
    full = e.export_chains(0, rows)  # [rows][D + 2][P]
    t["export_chains"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lp2 = e.logpost(prop_theta)
    t["logpost_of_the_proposal_rows"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    Dm = e.D
    th = np.ascontiguousarray(np.transpose(full[:, :Dm, :], (0, 2, 1)))
    rmid = rows // 2
    m, L = D.bridge_fit(D.bridge_transform(th[:rmid].reshape(-1, Dm), lo, hi)[0])
    xi, lj = D.bridge_transform(th[rmid:].reshape(-1, Dm), lo, hi)
    l1 = lp1 + lj - D.chains.bridge_logg(xi, m, L)
    xi2, lj2 = D.bridge_transform(prop_theta, lo, hi)
    l2 = lp2 + lj2 - D.chains.bridge_logg(xi2, m, L)
    b = D.bridge_from_logs(l1, l2, lp2=lp2)
    t["numpy_twins"] = time.perf_counter() - t0
    return b, t


def one(name, rows, repeats):
    csrc = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
    if os.environ.get("TRACE_PREBUILT") != "1":  # (build here and ship the library to the GPU box: TRACE_PREBUILT=1 skips the make)
        subprocess.check_call(["make", "-B", "-j8", "-C", csrc, "-s", "TRACE=1", "OUT=../libdemc_hip_trace.so"], stdout=sys.stderr)
    import demc_amd as D
    D._ffi.LIB_PATH = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "libdemc_hip_trace.so")
    e, lo, hi = engine(name, rows)
    wall = []
    try:
        out, prop, post, fit = e.bridge(0, rows, 0, 1, diagnostics=True)  # warm-up: the first launch of each kernel
        sys.stderr.write("timed runs\n")
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = e.bridge(0, rows, 0, 1)
            wall.append((time.perf_counter() - t0) * 1e3)
        sys.stderr.write("host route\n")
        t0 = time.perf_counter()
        hb, parts = host_route(D, e, rows, lo, hi, np.ascontiguousarray(prop[:, :e.D]), post[:, 0].copy())
        host_wall = (time.perf_counter() - t0) * 1e3
    finally:
        e.close()
    s = SIZES[name]
    b = D.Bridge(out)
    return dict(size=name, N=s["N"], D=s["D"], chains=s["G"] * s["Np"], rows=rows, draws=rows * s["G"] * s["Np"], n_fit=b.n_fit, n1=b.n1, n2=b.n2, repeats=repeats,
                wall_ms_median=float(np.median(wall)), wall_ms_min=float(min(wall)), wall_ms_max=float(max(wall)),
                logml=b.logml, se=b.se(1.0), n_iter=b.n_iter, converged=b.converged,
                host_route_ms=host_wall, host_route_parts_ms={k: v * 1e3 for k, v in parts.items()}, host_route_logml=hb.logml,
                host_over_device=host_wall / float(np.median(wall)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=float, default=500.0, help="seconds each size may take")
    ap.add_argument("--size", choices=sorted(SIZES), help="(internal) run this size in this process")
    ap.add_argument("--only", choices=sorted(SIZES), help="time this size alone")
    o = ap.parse_args()
    if o.size:
        print(json.dumps(one(o.size, o.rows, o.repeats)))
        return 0
    for name in ([o.only] if o.only else list(SIZES)):  # a fresh process per size, each under its own limit; a GPU fault or a time-out ends the run
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
        timed = err[err.index("timed runs") + 1:err.index("host route")] if "timed runs" in err and "host route" in err else []
        st = [[float(x) for x in ln.split()[2:]] for ln in timed if ln.startswith("demc_bridge pass_ms")]
        if st:
            a = np.array(st)  # [repeat][transform and fit, draws, evaluations, iteration]
            dev = a.sum(axis=1)
            res.update(device_ms_median=float(np.median(dev)), device_ms_min=float(dev.min()), device_ms_max=float(dev.max()),
                       stage_ms_median=dict(transform_and_fit=float(np.median(a[:, 0])), draws_and_solve=float(np.median(a[:, 1])),
                                            evaluations=float(np.median(a[:, 2])), iteration_and_errors=float(np.median(a[:, 3]))),
                       method="events on the handle's stream around the stages (the diagnostic variant); the wall clock is the whole call, host work included")
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
