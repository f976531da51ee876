"""What the bridge-sampling tests share (demc_bridge): the plan program of csrc/demc_bridgeplan.hpp, the definition
restated with mpmath at 40 digits, the closed-form marginal likelihoods with their exact-posterior draws, the inputs the edge rules
are checked on, the geometry of the device code restated, and the split windows of the iteration with their conditions.  No GPU."""
import atexit
import functools
import math
import os
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np

from conftest import make_problem
from loo_cases import BAR  # the project's bar: 1e-9 relative to max(1, |ref|)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
DIGITS = 40
CLOSED_ROWS, CLOSED_P = 64, 32  # the closed forms: 2048 draws, half of them fit the proposal


def err_in_bars(got, ref):
    """the worst |got - ref| / max(1, |ref|) over the finite entries in units of BAR; the non-finite pattern must be equal exactly"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()) / BAR


# ---- the plan program -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def program():
    """tests/bridgeplan_host.cpp under the address and undefined-behaviour sanitizers, built once per session"""
    tmp = tempfile.mkdtemp(prefix="bridgeplan_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "bridgeplan_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "bridgeplan_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


# ---- the definition at 40 digits ------------------------------------------------------------------------------------------------------
def mp_transform(theta, lo, hi):
    """one scalar -> (xi, logJ) as floats"""
    with mpmath.workdps(DIGITS):
        t, inf = mpmath.mpf(float(theta)), float("inf")
        if lo > -inf and hi < inf:
            a, b = mpmath.mpf(float(lo)), mpmath.mpf(float(hi))
            # u is the FP64 quotient as written (it IS the definition: next to hi, 1 - u has no more digits than u has); the rest is mpmath
            u = mpmath.mpf(float((np.float64(theta) - np.float64(lo)) / (np.float64(hi) - np.float64(lo))))
            xi = mpmath.log(u) - mpmath.log1p(-u)
            return float(xi), float(mpmath.log(b - a) - abs(xi) - 2 * mpmath.log1p(mpmath.exp(-abs(xi))))
        if lo > -inf:
            xi = mpmath.log(t - mpmath.mpf(float(lo)))
            return float(xi), float(xi)
        if hi < inf:
            xi = mpmath.log(mpmath.mpf(float(hi)) - t)
            return float(xi), float(xi)
        return float(t), 0.0


def mp_logjac_both(xi, lo, hi):
    """logJ of the two-sided transform at a GIVEN xi: log((hi - lo) s (1 - s)), s = 1 / (1 + exp(-xi))"""
    with mpmath.workdps(DIGITS):
        x = mpmath.mpf(float(xi))
        s = 1 / (1 + mpmath.exp(-x))
        return float(mpmath.log(mpmath.mpf(float(hi)) - mpmath.mpf(float(lo))) + mpmath.log(s) + mpmath.log1p(-s) if abs(x) < 30 else
                     mpmath.log(mpmath.mpf(float(hi)) - mpmath.mpf(float(lo))) - abs(x) - 2 * mpmath.log1p(mpmath.exp(-abs(x))))


def mp_logg(xi, m, L):
    """log of the Normal density with mean m and covariance L L' at xi, by the inverse of L L' in mpmath"""
    with mpmath.workdps(DIGITS):
        D = len(m)
        Lm = mpmath.matrix([[mpmath.mpf(float(L[i][j])) if j <= i else 0 for j in range(D)] for i in range(D)])
        d = mpmath.matrix([mpmath.mpf(float(xi[k])) - mpmath.mpf(float(m[k])) for k in range(D)])
        y = mpmath.lu_solve(Lm, d)
        q = mpmath.fsum(v * v for v in y)
        return float(-q / 2 - mpmath.fsum(mpmath.log(Lm[k, k]) for k in range(D)) - mpmath.mpf(D) / 2 * mpmath.log(2 * mpmath.pi))


def mp_bridge(l1, l2):
    """DESIGN.md 5.10 steps 5 and 6 in mpmath on the shifted logs, never forming exp of a large number: -> (logml, re2_prop, re2_post_iid,
    n_iter).  A term of the numerator is 1 / (s1 + s2 r exp(-x2)), a -Inf among l2 contributing 0."""
    with mpmath.workdps(DIGITS):
        mpf = mpmath.mpf
        N1, N2 = len(l1), len(l2)
        s1, s2 = mpf(N1) / (N1 + N2), mpf(N2) / (N1 + N2)
        lstar = max(float(v) for v in l1)
        e1 = [mpmath.exp(mpf(float(v)) - mpf(lstar)) if v != -math.inf else mpf(0) for v in l1]
        e2 = [None if v == -math.inf else mpmath.exp(mpf(lstar) - mpf(float(v))) for v in l2]  # (formed once: the iteration may run to its limit)
        f1_of = lambda r: [mpf(0) if e is None else 1 / (s1 + s2 * r * e) for e in e2]  # noqa: E731
        r, n_iter = mpf(1), 0
        while n_iter < 1000:
            rn = (mpmath.fsum(f1_of(r)) / N2) / (mpmath.fsum(1 / (s1 * e + s2 * r) for e in e1) / N1)
            n_iter += 1
            done = abs(rn - r) <= mpf("1e-10") * abs(rn)
            r = rn
            if done:
                break
        f1, f2 = f1_of(r), [1 / (s1 * e / r + s2) for e in e1]
        m1, m2 = mpmath.fsum(f1) / N2, mpmath.fsum(f2) / N1
        re1 = mpmath.fsum((f - m1) ** 2 for f in f1) / (N2 - 1) / m1 ** 2 / N2 if N2 > 1 else mpmath.nan
        re2 = mpmath.fsum((f - m2) ** 2 for f in f2) / (N1 - 1) / m2 ** 2 / N1 if N1 > 1 else mpmath.nan
        return float(mpmath.log(r) + lstar), float(re1), float(re2), n_iter


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def closed_problem(family, seed=20250):
    """-> (prob, exact log marginal likelihood, rows[CLOSED_ROWS][CLOSED_P][D] of iid draws from the exact posterior, (theta_hat, log
    posterior density at theta_hat)): Binomial with the Beta(1,1) prior of make_problem, mvn_full with d = 3 and Normal(0,1) priors"""
    rng = np.random.default_rng(seed)
    n_draws = CLOSED_ROWS * CLOSED_P
    if family == "binomial":
        prob = make_problem("binomial", rng, N=5)
        n, k = np.asarray(prob["data"][:5]), np.asarray(prob["data"][5:])
        a, b = k.sum() + 1.0, (n - k).sum() + 1.0
        lbeta = lambda p, q: math.lgamma(p) + math.lgamma(q) - math.lgamma(p + q)  # noqa: E731
        exact = sum(math.lgamma(x + 1) - math.lgamma(y + 1) - math.lgamma(x - y + 1) for x, y in zip(n, k)) + lbeta(a, b)
        rows = rng.beta(a, b, (CLOSED_ROWS, CLOSED_P, 1))
        th = a / (a + b)
        return prob, exact, rows, (np.array([th]), (a - 1) * math.log(th) + (b - 1) * math.log1p(-th) - lbeta(a, b))
    assert family == "mvn_full"
    d, N = 3, 20
    prob = make_problem("mvn_full", rng, N=N, d=d)
    X, Sigma = np.asarray(prob["data"]).reshape(N, d), np.asarray(prob["Sigma"])
    Si = np.linalg.inv(Sigma)
    Vn = np.linalg.inv(np.eye(d) + N * Si)
    mn = Vn @ (N * Si @ X.mean(axis=0))
    K = np.kron(np.eye(N), Sigma) + np.kron(np.ones((N, N)), np.eye(d))  # vec(X) ~ Normal(0, K) with mu ~ Normal(0, I) integrated out
    x = X.ravel()
    exact = -0.5 * (x @ np.linalg.solve(K, x)) - 0.5 * np.linalg.slogdet(K)[1] - 0.5 * N * d * math.log(2 * math.pi)
    rows = rng.multivariate_normal(mn, Vn, CLOSED_ROWS * CLOSED_P).reshape(CLOSED_ROWS, CLOSED_P, d)
    assert rows.shape[0] * rows.shape[1] == n_draws
    return prob, float(exact), rows, (mn, -0.5 * np.linalg.slogdet(Vn)[1] - 0.5 * d * math.log(2 * math.pi))


def twin_bridge(D, rows, lo, hi, logpost, n_prop=0, seed=0, trace=None):
    """the whole call on the twins: rows[R][P][D], logpost(theta[n][D]) -> lp[n] -> (Bridge, l1, l2); trace as in bridge_from_logs"""
    R, P, dim = rows.shape
    rmid = R // 2
    fit, est = rows[:rmid].reshape(-1, dim), rows[rmid:].reshape(-1, dim)
    m, L = D.bridge_fit(D.bridge_transform(fit, lo, hi)[0])
    xi, lj = D.bridge_transform(est, lo, hi)
    l1 = logpost(est) + lj - D.chains.bridge_logg(xi, m, L)
    n2 = n_prop or est.shape[0]
    th2, lj2, lg2 = D.bridge_draws(m, L, n2, seed, lo, hi)
    lp2 = logpost(th2)
    l2 = lp2 + lj2 - lg2
    return D.bridge_from_logs(l1, l2, n_fit=fit.shape[0], lp2=lp2, trace=trace), l1, l2


# ---- the geometry of the device code, restated (csrc/demc_bridgeplan.hpp; tests/test_bridge_host.py holds it to the plan program) ------
BRIDGE_WG, BRIDGE_LANE, BRIDGE_MAX_W, BRIDGE_PER_THREAD, BRIDGE_BATCH, COV_CHUNK, COV_MAX_WORKERS = 256, 64, 256, 4, 8, 512, 512
GEOMETRY_KEYS = ("n_fit", "N1", "N2", "W1", "W2", "chunks1", "chunks2", "pad2", "last2", "draw_blocks", "solve_blocks", "lds_bytes", "cov_chunks", "cov_workers")


def geometry(R, P, D, n_prop=0):
    """what demc_bridge launches for a window of R rows of P draws of D scalars and n_prop proposal draws (0: N1) -> dict of GEOMETRY_KEYS
    (plan_bridge's numbers; cov_chunks and cov_workers are plan_cov's for the fit half) and logs_blocks, the grid of k_bridge_logs and
    k_bridge_exp (blocks_of(max(N1, N2)) in csrc/demc_bridge.cpp)"""
    n_fit, N1 = (R // 2) * P, (R - R // 2) * P
    N2 = n_prop or N1
    workers = lambda n: max(1, min(-(-n // (BRIDGE_WG * BRIDGE_PER_THREAD)), BRIDGE_MAX_W))  # noqa: E731
    chunks2 = -(-N2 // P)
    cov_chunks = -(-n_fit // COV_CHUNK)
    return dict(n_fit=n_fit, N1=N1, N2=N2, W1=workers(N1), W2=workers(N2), chunks1=N1 // P, chunks2=chunks2, pad2=chunks2 * P, last2=N2 - (chunks2 - 1) * P,
                draw_blocks=-(-(chunks2 * P) // BRIDGE_LANE), solve_blocks=-(-N1 // BRIDGE_LANE), lds_bytes=max(D, 1) * BRIDGE_LANE * 8, cov_chunks=cov_chunks,
                cov_workers=min(cov_chunks, COV_MAX_WORKERS), logs_blocks=-(-max(N1, N2) // BRIDGE_WG))


def plan_geometry(shapes):
    """plan_bridge's own answer for each (R, P, D, n_prop), through the plan program's G request -> list of dicts of GEOMETRY_KEYS"""
    run = subprocess.run([program(), "--dump"], input="".join(f"G {R} {P} {D} {n_prop}\n" for R, P, D, n_prop in shapes), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr
    out = [{k: int(v) for k, v in (tok.split("=", 1) for tok in line.split())} for line in run.stdout.splitlines()]
    assert len(out) == len(shapes)
    return out


def asserted_geometry(label, R, P, D, n_prop=0, **want):
    """the geometry of a GPU case, the numbers the case exists for asserted and printed"""
    g = geometry(R, P, D, n_prop)
    for k, v in want.items():
        assert g[k] == v, (label, k, g[k], v)
    print(f"{label}: plan " + " ".join(f"{k}={g[k]}" for k in want))
    return g


WIN_R, WIN_P = 130, 16  # the window of two reduction workgroups a side: N_fit = N1 = 1040
CAP_P, CAP_N2 = 512, 262145  # the first N2 at which kBridgeMaxW binds and a thread takes a fifth element: 256 * 256 * 4 + 1
# the (R, P, D, n_prop) of the GPU cases of tests/test_gpu_bridge.py; the host test holds geometry() to the planner on these and on a grid
GPU_SHAPES = ([(WIN_R, WIN_P, 2, n) for n in (0, 2049, 257)] + [(6, 13, 2, n) for n in (63, 64, 65, 128)] + [(64, 16, 2, 0), (54, 19, 2, 0)] +
              [(R, D + 1, D, 0) for D in (63, 64) for R in (2, 8)] + [(2, CAP_P, 2, CAP_N2), (20, WIN_P, 2, 0), (6, 13, 3, 0), (6, 13, 2, 0)])


# ---- the inputs of the GPU cases past one workgroup and of the iteration's windows ------------------------------------------------------
def spread_rows(rng, prob, n, P, sd=0.05):
    """posterior_like's sibling with the centre at the data's own mean and standard deviation (Gaussian): rows the log posterior is
    smooth over, all strictly inside the bounds"""
    data = np.asarray(prob["data"], dtype=np.float64)
    return np.array([data.mean(), data.std()]) + sd * rng.normal(0, 1, (n, P, 2))


WIDE_BOUNDS = ((-math.inf, math.inf), (-1.0, math.inf), (-math.inf, 2.0), (-3.0, 0.25))  # the four kinds, assigned cyclically
WIDE_CENTRE = (0.1, 0.1, 0.1, -1.0)


def wide_problem(D):
    """Rastrigin at D scalars (no data; the density is not normalised, which a stage-by-stage check does not need) under Normal(0, 3)
    priors, the four kinds of bounds assigned cyclically over the scalars -> (prob, centre[D])"""
    from demc_amd import families as F
    lo, hi = [WIDE_BOUNDS[k % 4][0] for k in range(D)], [WIDE_BOUNDS[k % 4][1] for k in range(D)]
    centre = np.array([WIDE_CENTRE[k % 4] for k in range(D)])
    return dict(fam=F.FAM_RASTRIGIN, data=None, dims=[], hyper=None, D=D, pk=[F.PRIOR_NORMAL] * D, pa=[0.0] * D, pb=[3.0] * D, pref=[0] * D, lo=lo, hi=hi), centre


# The split windows of the iteration (Gaussian, N = 50, mu unbounded, sigma > 0): the fit half is centre + fit_sd N(0,1), the estimate
# half centre + (shift, 0) + est_sd N(0,1), centre = (mean, sd) of the data.  Each carries the CONDITION its case exists for, checked on
# the twins with the oracle's log posterior in tests/test_bridge_host.py and again on the device's own logs in tests/test_gpu_bridge.py;
# a window that misses its condition asks for another seed.
WINDOWS = {
    "slow, a few batches": dict(seed=52001, R=WIN_R, P=WIN_P, fit_sd=0.05, est_sd=0.05, shift=0.2, n_prop=0, kind="slow", lo=8, hi=64),
    "slow, many batches": dict(seed=52059, R=WIN_R, P=WIN_P, fit_sd=0.05, est_sd=0.05, shift=0.36, n_prop=0, kind="slow", lo=64, hi=999),
    "iteration limit": dict(seed=52003, R=20, P=WIN_P, fit_sd=0.04, est_sd=0.05, shift=0.4, n_prop=0, kind="limit"),
    "r stops": dict(seed=52004, R=WIN_R, P=WIN_P, fit_sd=0.01, est_sd=0.15, shift=0.0, n_prop=2049, kind="stops"),
}
WINDOW_DRAW_SEED = 11


@functools.lru_cache(maxsize=None)
def split_window(name):
    """-> (prob, rows[R][P][2]) of WINDOWS[name]"""
    w = WINDOWS[name]
    rng = np.random.default_rng(w["seed"])
    prob = make_problem("gaussian", rng, N=50)
    rmid = w["R"] // 2
    data = np.asarray(prob["data"], dtype=np.float64)
    centre = np.array([data.mean(), data.std()])
    z = rng.normal(0, 1, (w["R"], w["P"], 2))
    rows = np.empty_like(z)
    rows[:rmid] = centre + w["fit_sd"] * z[:rmid]
    rows[rmid:] = centre + np.array([w["shift"], 0.0]) + w["est_sd"] * z[rmid:]
    rows.setflags(write=False)
    return prob, rows


STOP_MARGIN = 0.1  # see window_condition


def window_condition(name, b, trace):
    """the condition of WINDOWS[name] on a twin's record b and its trace [(r, relative change)]: raises AssertionError with the figures.

    slow: converged after more than lo and at most hi iterations, and rounding cannot move the stop by more than one step.  For the
    window of a few batches that is the plain form: the change that stopped the iteration is at most half the tolerance, or the one
    before is at least twice it.  A sequence that needs more than 64 iterations to come from a change of order 1 to 1e-10 shrinks its
    change by a factor rho > 0.69 a step, and the plain form needs rho <= 0.5: no window of many batches can meet it (85 of 85 tried
    did not).  What it is there for is then asked directly.  Two evaluations of one mean over N <= 2080 terms in different orders
    differ by at most N 2^-53 = 2.3e-13 of it; the map is a contraction of rate rho, so two sequences stay within
    2 * 2.3e-13 / (1 - rho) of each other, 1.9e-12 of r at rho <= 0.75 (asserted); the change is a difference of two iterates, so the
    relative change moves by at most 2 * 1.9e-12 / 1e-10 < STOP_MARGIN of itself near the tolerance.  With t the stop of the
    reference: every change before t - 1 is at least (1 + STOP_MARGIN) 1e-10, so nothing stops before t - 1, and the change
    extrapolated to t + 1, rho times the last, is at most 1e-10 / (1 + STOP_MARGIN), so everything has stopped by t + 1.
    Both forms also ask that t is not 0 or 7 mod the batch of eight: a device that ran its batch to the end would otherwise pass the
    comparison of the counts within one."""
    w = WINDOWS[name]
    n = int(b.n_iter)
    what = (name, n, b.converged, trace[-3:])
    tol = 1e-10
    if w["kind"] == "slow":
        assert b.converged == 1 and w["lo"] < n <= w["hi"] and n == len(trace), what
        if n <= 64:
            assert trace[-1][1] <= 0.5 * tol or trace[-2][1] >= 2.0 * tol, what
        else:
            rho = trace[-1][1] / trace[-2][1]
            assert rho <= 0.75 and min(t[1] for t in trace[:-2]) >= (1.0 + STOP_MARGIN) * tol and rho * trace[-1][1] <= tol / (1.0 + STOP_MARGIN), what
        assert 1 <= n % BRIDGE_BATCH <= BRIDGE_BATCH - 2, what
    elif w["kind"] == "limit":
        assert b.converged == 0 and n == 1000 and n == len(trace) and math.isfinite(b.logml) and min(t[1] for t in trace) >= 2.0 * tol, what
    else:
        assert w["kind"] == "stops"
        assert b.converged == 0 and 1 <= n < 1000 and n == len(trace) and not (math.isfinite(trace[-1][0]) and trace[-1][0] > 0.0) and b.n_nonfinite == 0, what
