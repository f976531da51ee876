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


# ---- the path of the select in k_loo_column, restated ---------------------------------------------------------------------------
# Used only to prove that a test's input reaches the branch it is there for (as geometry() is in the rank tests); never a reference
# for a result.
LOO_BITS, LOO_DIGITS = 11, 6
_ALL, _SIGN = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63)


def keys_of(col):
    """the integer keys of section 5.6, as uint64"""
    b = np.ascontiguousarray(col, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, _ALL, _SIGN)


def _digit(d):
    """digit d is bits [dsh, top): 11 bits each, the last one the nine bits [0, 9)"""
    return (64 - LOO_BITS * (d + 1) if d < LOO_DIGITS - 1 else 0), 64 - LOO_BITS * d


def select_path(col, M):
    """step (2) of k_loo_column as the kernel text walks it -> dict(early, stop_digit (None: unresolved), counted, skipped (digits
    counted and skipped up to the stop), nc (the keys step (3) compacts))"""
    k = keys_of(col)
    kmin, kmax = int(k.min()), int(k.max())
    prefix, rank, below = 0, int(M), 0
    counted = skipped = 0
    for d in range(LOO_DIGITS):
        dsh, top = _digit(d)
        if kmin >> dsh == kmax >> dsh:
            prefix = (kmin >> dsh) << dsh
            skipped += 1
            continue
        counted += 1
        mask = (1 << (top - dsh)) - 1
        sel = k if d == 0 else k[(k >> np.uint64(top)) == np.uint64(prefix >> top)]
        hist = np.bincount(((sel >> np.uint64(dsh)) & np.uint64(mask)).astype(np.int64), minlength=1 << LOO_BITS)
        part = hist.reshape(256, 8).sum(axis=1)
        acc, g = 0, 0
        while g < 255 and rank >= acc + part[g]:  # eight bins at a time, then bin by bin
            acc += int(part[g])
            g += 1
        b = 8 * g
        while b < 8 * g + 7 and rank >= acc + hist[b]:
            acc += int(hist[b])
            b += 1
        cnt = int(hist[b])
        below += acc
        rank -= acc
        prefix |= b << dsh
        if below + cnt <= LOO_CAP:
            return dict(early=True, stop_digit=d, counted=counted, skipped=skipped, nc=below + cnt)
    return dict(early=False, stop_digit=None, counted=counted, skipped=skipped, nc=below)  # lim = key_c - 1: the keys below the cutoff


def select_path_direct(col, M):
    """the same answer without a walk: k_M is the (M + 1)-th smallest key; the stop is the first digit on which the keys differ whose
    bins up to k_M's hold at most 8192 keys"""
    k = keys_of(col)
    kM = np.sort(k)[M]
    lo, hi = k.min(), k.max()
    counted = skipped = 0
    for d in range(LOO_DIGITS):
        dsh = np.uint64(_digit(d)[0])
        if lo >> dsh == hi >> dsh:
            skipped += 1
            continue
        counted += 1
        n = int(((k >> dsh) <= (kM >> dsh)).sum())
        if n <= LOO_CAP:
            return dict(early=True, stop_digit=d, counted=counted, skipped=skipped, nc=n)
    return dict(early=False, stop_digit=None, counted=counted, skipped=skipped, nc=int((k < kM).sum()))


def select_paths(ll):
    """select_path of every column of ll[S][N], checked on the way against the closed form and against what each outcome means"""
    S, N = ll.shape
    M = plan(N, S)["M"]
    assert M > 0
    out = []
    for i in range(N):
        col = np.ascontiguousarray(ll[:, i])
        p, q = select_path(col, M), select_path_direct(col, M)
        assert p == q, (i, p, q)
        k = keys_of(col)
        n_le = int((k <= np.sort(k)[M]).sum())
        if p["early"]:
            assert M < p["nc"] <= LOO_CAP, (i, p)
        elif p["counted"]:
            assert p["nc"] <= M and n_le > LOO_CAP, (i, p, n_le)
        else:  # no digit differs: a constant column, whatever its length (the keys up to the cutoff are all of them)
            assert p["nc"] == 0 and n_le == S and p["skipped"] == LOO_DIGITS, (i, p, n_le)
        out.append(p)
    return out


def reach(paths):
    """how many columns stop at each digit ('u': unresolved) -> dict"""
    out = {}
    for p in paths:
        key = p["stop_digit"] if p["early"] else "u"
        out[key] = out.get(key, 0) + 1
    return out


# ---- column families with ties, crowds and narrow ranges --------------------------------------------------------------------------
# Gaussian (D = 2), N = 65.  Ties are repeated draws -- equal theta gives equal terms bit for bit in every column -- and the repeats
# sit at random cells of the window.
N_FAMILY = 65
CROWD_K = (12, 24, 34, 45, 51, 52)  # (52: the crowd's terms tie in more columns than at 51 -- a second, wider reach of the unresolved branch)
CROWD_SEED = {51: 9907, 52: 9906}  # seeds at which the DEVICE's terms of the three draws tie (all 9000 equal) in at least four columns


def family_data(rng, N=N_FAMILY):
    y = rng.normal(0.3, 1.2, N)
    y[0] = 50.0  # beside ordinary points: the floor is active in this column
    return y


def tied_draws(rng, distinct, repeated):
    """distinct[n][2] and the draws of repeated = [((mu, sigma), copies), ...], shuffled over the window"""
    th = np.concatenate([np.asarray(distinct, dtype=np.float64).reshape(-1, 2)] + [np.tile(np.array(t, dtype=np.float64), (c, 1)) for t, c in repeated])
    return th[rng.permutation(th.shape[0])]


def crowd(k, S=9216, copies=3000, seed=None):
    """three draws 2^-k apart in sigma, `copies` times each, beside S - 3 copies well-spread draws (fewer than M): the cutoff falls
    in the crowd, and the crowd's terms part only at a digit that deepens with k"""
    rng = np.random.default_rng((CROWD_SEED.get(k, 9900) if seed is None else seed) + k)
    y = family_data(rng)
    rep = [((0.55, 0.8 * (1.0 + j * 2.0 ** -k)), copies) for j in range(3)]
    return y, tied_draws(rng, gaussian_draws(rng, S - 3 * copies), rep)


def one_draw(S=9216, copies=8500, at=(0.55, 0.8), seed=9910):
    """one draw `copies` times: more than 8192 equal keys, which no bin can separate"""
    rng = np.random.default_rng(seed)
    y = family_data(rng)
    return y, tied_draws(rng, gaussian_draws(rng, S - copies), [(at, copies)])


def four_times(S=2000, seed=9920):
    """every draw four times: the cutoff falls inside a run"""
    rng = np.random.default_rng(seed)
    y = family_data(rng)
    d = gaussian_draws(rng, S // 4)
    return y, tied_draws(rng, np.empty((0, 2)), [(tuple(t), 4) for t in d])


def two_values(seed=9930):
    """S = 130: one draw 100 times, another 30 times -- either way the M + 1 = 27 smallest terms tie, the cutoff is the minimum"""
    rng = np.random.default_rng(seed)
    y = family_data(rng)
    return y, tied_draws(rng, np.empty((0, 2)), [((0.25, 1.1), 100), ((0.4, 0.9), 30)])


def constant(S, seed=9940):
    rng = np.random.default_rng(seed)
    return family_data(rng), np.tile(np.array([0.25, 1.1]), (S, 1))


def mixed_sign(S=9216, seed=9950):
    """narrow sigma about 0.3: the term of a point 0.226 from mu changes sign across the draws"""
    rng = np.random.default_rng(seed)
    h = N_FAMILY // 2
    y = np.concatenate([0.3 + rng.choice([-0.226, 0.226], h) + rng.normal(0.0, 0.02, h), rng.normal(0.3, 0.3, N_FAMILY - h)])
    th = np.stack([rng.normal(0.3, 0.1, S), np.maximum(rng.normal(0.3, 0.03, S), 0.1)], axis=1)
    return y, th


def narrow(S=2000, jitter=1e-12, seed=9960):
    """draws 1e-12 apart: every key of a column shares its leading two or three digits.  (At 1e-13 the quartile excess of some
    columns falls to 3e-13, under the 2^-40 the tests ask of it; at 1e-12 the smallest is 3e-12.)"""
    rng = np.random.default_rng(seed)
    y = family_data(rng)
    i, j = rng.integers(0, 1000, S), rng.integers(0, 1000, S)
    return y, np.stack([0.3 * (1.0 + jitter * i), 1.0 + jitter * j], axis=1)


def quartile_excess(ll):
    """e_q of the definition for every column of ll[S][N] in FP64 (NaN where no fit is tried)"""
    S, N = ll.shape
    M = tail_len(S)
    out = np.full(N, np.nan)
    for i in range(N):
        ls = np.sort(ll[:, i])
        x = ls[0] - ls
        x_cut = max(ls[0] - ls[M], LOG_MIN)
        xt = x[x > x_cut][::-1]
        if xt.size > 4:
            out[i] = (np.exp(xt) - np.exp(x_cut))[int(math.floor(xt.size / 4.0 + 0.5)) - 1]
    return out


HOST_FAMILIES = {  # name -> (y, theta): what tests/test_loo_host.py walks with gaussian_terms, and tests/test_gpu_loo.py on the device
    **{f"crowd k={k}": (lambda k=k: crowd(k)) for k in CROWD_K},
    "one draw 8500 times": one_draw, "every draw four times": four_times, "two values": two_values,
    "constant S=130": lambda: constant(130), "constant S=26": lambda: constant(26), "mixed sign": mixed_sign, "narrow": narrow,
}
