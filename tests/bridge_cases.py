"""What the bridge-sampling tests share (demc_bridge): the plan program of csrc/demc_bridgeplan.hpp, the definition
restated with mpmath at 40 digits, the closed-form marginal likelihoods with their exact-posterior draws, and the inputs the edge rules
are checked on.  No GPU."""
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
        f1_of = lambda r: [mpf(0) if v == -math.inf else 1 / (s1 + s2 * r * mpmath.exp(mpf(lstar) - mpf(float(v)))) for v in l2]  # noqa: E731
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


def twin_bridge(D, rows, lo, hi, logpost, n_prop=0, seed=0):
    """the whole call on the twins: rows[R][P][D], logpost(theta[n][D]) -> lp[n] -> (Bridge, l1, l2)"""
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
    return D.bridge_from_logs(l1, l2, n_fit=fit.shape[0], lp2=lp2), l1, l2
