#!/usr/bin/env python3
"""Times demc_loo (PSIS-LOO on the device) at the two sizes of tools/waic_bench.py -- cfg5's share (LBA, 3 accumulators,
N = 50 000 trials, 4 096 chains, 100 history rows) and a Gaussian with N = 100 000 observations on the same 4 096 x 100 draws -- next
to demc_waic of the same window on the same handle.

    python3 tools/loo_bench.py [--rows 100] [--repeats 3] [--limit 500]

Each size runs in a process of its own under a time limit (`--limit` seconds), on the diagnostic variant of the library (`make TRACE=1
OUT=../libdemc_hip_trace.so`; TRACE_PREBUILT=1: the variant is there already), which brackets the passes of both calls with events on
the handle's stream and prints their device times to stderr: for demc_loo the preparation, then k_loo_terms and k_loo_column of every
observation block, then the totals.  After one warm-up call of each the runs alternate: demc_loo, demc_waic, ...  Prints one JSON
object per size: the median / min / max over the repeats of the device time of each call (the sum of its passes, by the events), the
medians of the term passes and the column passes summed over the blocks, the wall clock, and the ratio of the two calls."""
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


def one(name, rows, repeats):
    csrc = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
    if os.environ.get("TRACE_PREBUILT") != "1":
        subprocess.check_call(["make", "-B", "-j8", "-C", csrc, "-s", "TRACE=1", "OUT=../libdemc_hip_trace.so"], stdout=sys.stderr)
    import demc_amd
    demc_amd._ffi.LIB_PATH = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "libdemc_hip_trace.so")
    e = WB.engine(name, rows)
    loo_wall, waic_wall = [], []
    try:
        tot, _ = e.loo(0, rows)  # warm-up: the first launch of each kernel
        e.waic(0, rows)
        sys.stderr.write("timed runs\n")
        for _ in range(repeats):  # alternating
            t0 = time.perf_counter()
            tot, _ = e.loo(0, rows)
            loo_wall.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            wtot, _ = e.waic(0, rows)
            waic_wall.append((time.perf_counter() - t0) * 1e3)
    finally:
        e.close()
    s = WB.SIZES[name]
    S = rows * s["G"] * s["Np"]
    return dict(size=name, N=s["N"], chains=s["G"] * s["Np"], rows=rows, draws=S, evaluations=S * s["N"], repeats=repeats,
                loo_wall_ms_median=float(np.median(loo_wall)), waic_wall_ms_median=float(np.median(waic_wall)),
                totals=dict(zip(demc_amd.chains.LOO_TOTALS, (float(v) for v in tot))),
                waic_totals=dict(zip(demc_amd.chains.WAIC_TOTALS, (float(v) for v in wtot))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=float, default=500.0, help="seconds each size may take")
    ap.add_argument("--size", choices=sorted(WB.SIZES), help="(internal) run this size in this process")
    ap.add_argument("--only", choices=sorted(WB.SIZES), help="time this size alone")
    o = ap.parse_args()
    if o.size:
        print(json.dumps(one(o.size, o.rows, o.repeats)))
        return 0
    for name in ([o.only] if o.only else list(WB.SIZES)):  # a fresh process per size, each under its own limit; a GPU fault or a time-out ends the run
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
        loo = [[float(x) for x in ln.split()[2:]] for ln in timed if ln.startswith("demc_loo pass_ms")]
        waic = [sum(float(x) for x in ln.split()[2:]) for ln in timed if ln.startswith("demc_waic pass_ms")]
        if loo and waic:
            a = np.array(loo)  # [repeat][prepare, (terms, column) per block ..., totals]
            dev = a.sum(axis=1)
            med, wmed = float(np.median(dev)), float(np.median(waic))
            res.update(loo_device_ms_median=med, loo_device_ms_min=float(dev.min()), loo_device_ms_max=float(dev.max()), blocks=(a.shape[1] - 2) // 2,
                       pass_ms_median=dict(prepare=float(np.median(a[:, 0])), terms=float(np.median(a[:, 1:-1:2].sum(axis=1))),
                                           column=float(np.median(a[:, 2:-1:2].sum(axis=1))), totals=float(np.median(a[:, -1]))),
                       waic_device_ms_median=wmed, loo_over_waic=med / wmed, evaluations_per_second=res["evaluations"] / (med * 1e-3),
                       column_bytes_per_second=8.0 * res["evaluations"] / (float(np.median(a[:, 2:-1:2].sum(axis=1))) * 1e-3),
                       method="events on the handle's stream around the passes (the diagnostic variant), median of runs alternating with demc_waic")
        print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
