"""What the PSIS-LOO tests share (demc_loo): the plan program of csrc/demc_looplan.hpp and its Python restatement, the
definition restated in plain loops with mpmath at 40 digits, and the inputs the edge rules are checked on.  No GPU."""
import atexit
import functools
import math
import os
import shutil
import subprocess
import tempfile

import mpmath
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")

LOO_OBS, LOO_TILE, LOO_TARGET_WG, LOO_WG, LOO_CAP, LOO_MAX_TAIL = 64, 16, 2048, 512, 8192, 6144
LOO_MAX_DRAWS, LOO_MAX_CELLS = 1 << 22, 1 << 27
LOG_MIN = -708.3964185322641  # log(DBL_MIN) rounded to FP64
DIGITS = 40
BAR = 1e-9


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def tail_len(S):
    return int(math.ceil(min(0.2 * float(S), 3.0 * math.sqrt(float(S)))))


def plan(N, S):
    """what demc_loo launches for N observations and S draws -> dict(M, Nb, blocks, cuts, tiles, chunks, chunk_len)"""
    Nb = min(N, LOO_MAX_CELLS // S)
    blocks = -(-N // Nb)
    tiles = -(-Nb // LOO_OBS)
    want = max(1, min(LOO_TARGET_WG // tiles, -(-S // LOO_TILE)))
    chunk_len = -(-(-(-S // want)) // LOO_TILE) * LOO_TILE
    return dict(M=0 if S <= 20 else tail_len(S), Nb=Nb, blocks=blocks, cuts=[(b * Nb, min(N, (b + 1) * Nb)) for b in range(blocks)], tiles=tiles,
                chunks=-(-S // chunk_len), chunk_len=chunk_len)


@functools.lru_cache(maxsize=None)
def program():
    """tests/looplan_host.cpp under the address and undefined-behaviour sanitizers, built once per session"""
    tmp = tempfile.mkdtemp(prefix="looplan_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "looplan_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "looplan_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def plans(requests):
    """one dict per request line (tests/looplan_host.cpp says what a line is): the fields of the plan, or refused and message"""
    run = subprocess.run([program(), "--dump"], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(requests), (len(lines), len(requests))
    out = []
    for line in lines:
        head, _, message = line.partition(" message=")
        d = {k: int(v) for k, v in (tok.split("=", 1) for tok in head.split()[1:])}
        if message:
            d["message"] = message
        out.append(d)
    return out


# ---- the definition at 40 digits --------------------------------------------------------------------------------------------------
def _key(x):
    b = int(np.float64(x).view(np.uint64))
    return b ^ (0xFFFFFFFFFFFFFFFF if b >> 63 else 1 << 63)


def ref_column(l):
    """DESIGN.md 5.9 for one observation in plain loops: l[S] float64 -> (elpd_loo, p_loo, khat, lppd, n_tail, l_cut) as floats.  The
    selection is Python's sorted on the integer keys; x_s = fl(lmin - l_s) and the comparison with x_cut are FP64 (they ARE the
    definition of the tail); everything after that is mpmath."""
    l = [float(v) for v in l]
    S = len(l)
    nan, inf = float("nan"), float("inf")
    if any(v != v or v == inf for v in l):
        return (nan,) * 6
    with mpmath.workdps(DIGITS):
        mpf = mpmath.mpf
        fin = [v for v in l if v != -inf]
        if fin:
            mx = max(fin)
            lppd = float(mpf(mx) + mpmath.log(mpmath.fsum(mpmath.exp(mpf(v) - mpf(mx)) for v in fin)) - mpmath.log(S))
        else:
            lppd = -inf
        if len(fin) < S:
            return (-inf, float(np.float64(lppd) - np.float64(-inf)), inf, lppd, 0.0, -inf)
        ls = sorted(l, key=_key)
        lmin = ls[0]
        n2, l_cut, khat = 0, nan, inf
        xs_tail, ls_tail = [], []
        x_cut = None
        if S > 20:
            M = tail_len(S)
            l_cut = ls[M]
            x_cut = max(float(np.float64(lmin) - np.float64(l_cut)), LOG_MIN)
            tail = [v for v in ls if float(np.float64(lmin) - np.float64(v)) > x_cut]
            n2 = len(tail)
            ls_tail = tail[::-1]  # x ascending = l descending
            xs_tail = [mpf(float(np.float64(lmin) - np.float64(v))) for v in ls_tail]
            if n2 > 4:
                exc = mpmath.exp(mpf(x_cut))
                e = [mpmath.exp(x) - exc for x in xs_tail]
                n = n2
                q = int(math.floor(n / 4.0 + 0.5))
                if e[q - 1] > 0:
                    m = 30 + int(math.floor(math.sqrt(float(n))))
                    b = [(1 - mpmath.sqrt(mpf(m) / (mpf(j) - mpf("0.5")))) / (3 * e[q - 1]) + 1 / e[n - 1] for j in range(1, m + 1)]
                    k = [mpmath.fsum(mpmath.log1p(-bj * et) for et in e) / n for bj in b]
                    L = [n * (mpmath.log(-bj / kj) - kj - 1) for bj, kj in zip(b, k)]
                    w = [1 / mpmath.fsum(mpmath.exp(Li - Lj) for Li in L) for Lj in L]
                    bhat = mpmath.fsum(bj * wj for bj, wj in zip(b, w))
                    kk = mpmath.fsum(mpmath.log1p(-bhat * et) for et in e) / n
                    sigma = -kk / bhat
                    kh = (n * kk + 5) / (mpf(n) + 10)
                    khat = float(kh)
                    xs_tail = []
                    for t in range(1, n + 1):
                        p = (mpf(t) - mpf("0.5")) / n
                        g = -sigma * mpmath.log1p(-p) if kh == 0 else sigma * mpmath.expm1(-kh * mpmath.log1p(-p)) / kh
                        xs_tail.append(min(mpmath.log(g + exc), mpf(0)))
        outside = ls[n2:]
        num = [mpf(float(np.float64(lmin) - np.float64(v))) + mpf(v) for v in outside] + [x + mpf(v) for x, v in zip(xs_tail, ls_tail)]
        den = [mpf(float(np.float64(lmin) - np.float64(v))) for v in outside] + list(xs_tail)
        lse = lambda a: max(a) + mpmath.log(mpmath.fsum(mpmath.exp(v - max(a)) for v in a))  # noqa: E731
        elpd = lse(num) - lse(den)
        return (float(elpd), float(mpf(lppd) - elpd), khat, lppd, float(n2), l_cut)


def ref_table(ll):
    return np.array([ref_column(ll[:, i]) for i in range(ll.shape[1])])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
Y_FLOOR = np.array([0.1, -0.7, 1.3, 3.5, 50.0])  # 50.0 beside ordinary points: ratios span more than 708 log units, the floor is active


def gaussian_draws(rng, S):
    """posterior-like draws (mu, sigma) whose sigma varies enough for y = 50 to push part of its tail below the floor"""
    sd = 0.15 if S < 100 else 0.12 if S < 1000 else 0.08  # (a longer window reaches further into sigma's lower tail)
    return np.stack([rng.normal(0.3, 0.1, S), np.maximum(rng.normal(1.0, sd, S), 0.3)], axis=1)


def gaussian_terms(y, th):
    y, th = np.asarray(y, dtype=np.float64), np.asarray(th, dtype=np.float64)
    return -0.5 * ((y[None, :] - th[:, :1]) / th[:, 1:2]) ** 2 - np.log(th[:, 1:2]) - 0.5 * math.log(2 * math.pi)


def cutoff_gap_ok(ll, rel=BAR):
    """True where a reference column has no other term within rel |l| of its cutoff, and none of x within rel of the floor: another
    evaluation of the same terms (a few ulps apart) then selects the same tail"""
    S, N = ll.shape
    ok = np.ones(N, dtype=bool)
    if S <= 20:
        return ok
    M = tail_len(S)
    for i in range(N):
        ls = np.sort(ll[:, i])
        lc = ls[M]
        gap = rel * max(1.0, abs(lc))
        ok[i] = ls[M] - ls[M - 1] > gap and (M + 1 >= S or ls[M + 1] - ls[M] > gap)
        x = ls[0] - ls
        x_cut = max(ls[0] - lc, LOG_MIN)
        if x_cut == LOG_MIN:
            ok[i] = ok[i] and (np.abs(x - LOG_MIN) > rel * 709).all()
    return ok


def check_table(pt, ref, label, exact_tail=True):
    """a device (or numpy) table against a reference table: the non-finite pattern exactly, n_tail and l_cut exactly, the other columns at
    BAR of max(1, |ref|) (khat: of max(1, |khat|)) -> the worst error of each compared column, in units of BAR"""
    pt, ref = np.asarray(pt, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert pt.shape == ref.shape and pt.shape[1] == 6, (label, pt.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(pt), np.isnan(ref)), (label, np.argwhere(np.isnan(pt) != np.isnan(ref))[:5])
    assert np.array_equal(np.isfinite(pt), fin), label
    inf = ~fin & ~np.isnan(ref)
    assert np.array_equal(pt[inf], ref[inf]), label
    if exact_tail:
        assert np.array_equal(pt[:, 4][fin[:, 4]], ref[:, 4][fin[:, 4]]), (label, "n_tail", np.argwhere(pt[:, 4] != ref[:, 4])[:5].ravel())
        assert np.array_equal(pt[:, 5][fin[:, 5]], ref[:, 5][fin[:, 5]]), (label, "l_cut")
    worst = {}
    for c, name in ((0, "elpd_loo"), (1, "p_loo"), (2, "khat"), (3, "lppd")):
        f = fin[:, c]
        with np.errstate(all="ignore"):
            err = np.abs(pt[f, c] - ref[f, c]) / np.maximum(1.0, np.abs(ref[f, c]))
        worst[name] = float(err.max()) / BAR if err.size else 0.0
    return worst
