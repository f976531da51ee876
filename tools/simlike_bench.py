#!/usr/bin/env python3
"""Times the simulation-based likelihood path (demc_set_model_sim, k_sim_loglike) on the GPU, beside the same estimator in numpy on
the host's threads: the KDE example (Examples/KDE_Example.jl) scaled to 64 groups x 64 particles, N = 50 observations,
n_sim = 10 000 simulated values per proposal.  `--model lnr`: the pair path instead (k_sim_choice) -- a two-accumulator log-normal
race under the per-choice defective KDE, N = 50 (choice, response time) observations, the same population and n_sim.

    python3 tools/simlike_bench.py [--model normal|lnr] [--steps 50] [--warmup 10] [--repeats 5] [--cpu-rows 64]

Per repeat: `steps` iterations of demc_step with demc_timing_enable (HIP events in the dispatch packets) after `warmup`
iterations; prints one JSON object with the median and the spread over the repeats of the wall-clock ms per step, the likelihood
kernel's share of the device time, simulated values per second and kernel evaluations per second (n_sim x N per proposal), and
the numpy figure: the same estimator (Philox draws, Box-Muller, two-pass bandwidth, exact Epanechnikov sum) for `cpu-rows`
proposals spread over the host's threads."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M32 = np.uint64(0xFFFFFFFF)


def philox(blocks, entity, seed):
    c = [blocks.astype(np.uint64), np.full(blocks.size, entity, np.uint64), np.zeros(blocks.size, np.uint64),
         np.full(blocks.size, 7 << 24, np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def numpy_row(theta, x, n, entity, seed):
    w = [(v.astype(np.float64) + 0.5) / 4294967296.0 for v in philox(np.arange((n + 3) // 4), entity, seed)]
    r0, r1 = np.sqrt(-2.0 * np.log(1.0 - w[0])), np.sqrt(-2.0 * np.log(1.0 - w[2]))
    z = np.stack([r0 * np.cos(2 * np.pi * w[1]), r0 * np.sin(2 * np.pi * w[1]), r1 * np.cos(2 * np.pi * w[3]),
                  r1 * np.sin(2 * np.pi * w[3])], 1).ravel()[:n]
    s = theta[0] + theta[1] * z
    h = 0.9 * s.std(ddof=1) * n ** -0.2
    u = (x[:, None] - s[None, :]) / h
    return float(np.log(np.maximum(1e-10, 0.75 * np.maximum(0.0, 1.0 - u * u).sum(1) / (n * h))).sum())


def numpy_row_lnr(theta, oc, ox, n, entity, seed):
    """the pair path's CPU side: the race (K = 2: one Philox block a value), per-choice rule-of-thumb bandwidths, the defective densities"""
    w = [(v.astype(np.float64) + 0.5) / 4294967296.0 for v in philox(np.arange(n), entity, seed)]
    r0 = np.sqrt(-2.0 * np.log(1.0 - w[0]))
    T = np.exp(theta[None, :2] + np.stack([r0 * np.cos(2 * np.pi * w[1]), r0 * np.sin(2 * np.pi * w[1])], 1))
    c, t = np.where(T[:, 1] < T[:, 0], 2, 1), theta[2] + T.min(1)
    ll = 0.0
    for k in (1, 2):
        s, x = t[c == k], ox[oc == k]
        h = 0.9 * s.std(ddof=1) * s.size ** -0.2
        u = (x[:, None] - s[None, :]) / h
        ll += float(np.log(np.maximum(1e-10, 0.75 * np.maximum(0.0, 1.0 - u * u).sum(1) / (n * h))).sum())
    return ll


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", choices=("normal", "lnr"), default="normal")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--np", type=int, default=64, dest="Np")
    ap.add_argument("--n-sim", type=int, default=10_000)
    ap.add_argument("--n-obs", type=int, default=50)
    ap.add_argument("--cpu-rows", type=int, default=64)
    ap.add_argument("--cpu-threads", type=int, default=min(16, os.cpu_count() or 1))
    o = ap.parse_args()
    import demc_amd as D
    rng = np.random.default_rng(50514)
    x = rng.normal(0.0, 1.0, o.n_obs)
    P = o.groups * o.Np
    th0 = np.stack([rng.normal(0, 0.3, P), rng.uniform(0.8, 1.3, P)], 1)
    lnr = o.model == "lnr"
    if lnr:
        T = np.exp(rng.normal([-1.0, -0.7], 1.0, (o.n_obs, 2)))
        oc, ox = T.argmin(1) + 1, T.min(1) + 0.2
        th0 = np.stack([rng.normal(-1.0, 0.2, P), rng.normal(-0.7, 0.2, P), rng.uniform(0.05, 0.9, P) * ox.min()], 1)
    n_it = o.warmup + o.repeats * o.steps
    e = D.HipEngine(n_groups=o.groups, Np=o.Np, D=3 if lnr else 2, n_rows=n_it, seed=2024, burnin=n_it, schedule=2)
    try:
        if lnr:
            e.set_model_sim(2, 2, o.n_sim, np.concatenate([oc.astype(np.float64), ox]), hyper=[0.0, 1.0])
            e.set_priors([1, 1, 0], [0.0, 0.0, 0.0], [3.0, 3.0, 1.0])
            e.set_bounds([-np.inf, -np.inf, 0.0], [np.inf, np.inf, float(ox.min())])
        else:
            e.set_model_sim(0, 0, o.n_sim, x)
            e.set_priors([1, 2], [0.0, 0.0], [1.0, 1.0])
            e.set_bounds([-np.inf, 0.0], [np.inf, np.inf])
        e.set_state(th0)
        e.step(1, o.warmup)
        e.timing_enable(True)
        e.timing_read(reset=True)
        ms, share, ll_ms = [], [], []
        it = 1 + o.warmup
        for _ in range(o.repeats):
            t0 = time.perf_counter()
            e.step(it, o.steps)
            ms.append((time.perf_counter() - t0) * 1e3 / o.steps)
            t = e.timing_read(reset=True)
            dev = sum(v["ms"] for v in t.values())
            share.append(t["loglike"]["ms"] / dev)
            ll_ms.append(t["loglike"]["ms"] / o.steps)
            it += o.steps
        kernels = e.last_kernels()
        acc = float(e.get_history(o.warmup, n_it)[1].mean())
    finally:
        e.close()
    # the same estimator in numpy, `cpu-rows` proposals over the host's threads (numpy releases the GIL in its loops)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(o.cpu_threads) as pool:
        if lnr:
            list(pool.map(lambda r: numpy_row_lnr(th0[r], oc, ox, o.n_sim, r, 2024), range(o.cpu_rows)))
        else:
            list(pool.map(lambda r: numpy_row(th0[r], x, o.n_sim, r, 2024), range(o.cpu_rows)))
    cpu_ms_per_prop = (time.perf_counter() - t0) * 1e3 / o.cpu_rows
    med = float(np.median(ms))
    what = "log-normal race (K = 2) under the per-choice KDE" if lnr else "KDE example"
    out = dict(workload=f"{what}, {o.groups} groups x {o.Np} particles, N = {o.n_obs}, n_sim = {o.n_sim}", kernels=kernels,
               steps=o.steps, warmup=o.warmup, repeats=o.repeats, ms_per_step_median=med, ms_per_step_min=float(min(ms)),
               ms_per_step_max=float(max(ms)), loglike_kernel_ms_per_step_median=float(np.median(ll_ms)),
               loglike_share_of_device_time_median=float(np.median(share)), simulated_values_per_s=P * o.n_sim / (med * 1e-3),
               kernel_evaluations_per_s=P * o.n_sim * o.n_obs / (med * 1e-3), accept_rate=acc,
               numpy_ms_per_proposal=cpu_ms_per_prop, numpy_threads=o.cpu_threads, numpy_ms_per_step_equivalent=cpu_ms_per_prop * P,
               speedup_vs_numpy=cpu_ms_per_prop * P / med,
               method="wall clock around demc_step (drained), median / min / max over the repeats; kernel share from HIP events carried by the dispatch packets (demc_timing_enable)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
