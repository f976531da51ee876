"""What demc_pointwise_loglik and demc_waic are held to beyond the oracle, written once more by other means.  Nothing
here needs a GPU: tests/test_pointwise_cases_host.py runs it on the CPU, tests/test_gpu_pointwise_edges.py against the device.

1. Plain references.  ref_terms: l_is = log p(y_i | theta_s) of Gaussian, Binomial, MVN_ISO and MVN_FULL in mpmath at 40 digits on
   the RAW data (no centring, no whitened rows, no prepared constants) -- for S N up to about 2 000.  closed_terms: the same four
   families in numpy, for large N; the host test holds it to ref_terms at 1e-13 max(1, |ref|).  The race models keep the oracle's
   per-trial densities (orc_lba_logpdf, orc_lnr_logpdf).  ref_waic: the definition of 5.8 in mpmath, with its -Inf and NaN rules;
   chains.waic_from_loglik is held to it once, and so are the device's lppd of columns that span more than exp can hold.

2. kernel_walk: the arithmetic of k_pw_accumulate and k_pw_final in float64 numpy, operation by operation in the order the kernels
   write it (the library is built with -ffp-contract=off: the expressions are the ones written).  A chunk of chunk_len draws keeps
   l0 (its first term), a1 = sum (l - l0), a2 = sum (l - l0)^2 and the online (M, E); its partial is mean_c = l0 + a1 / n,
   M2_c = a2 - a1^2 / n; the chunks merge in index order by the pairwise rule of Chan, Golub and LeVeque.  shift=False is the same
   walk with the shift lost (l0 = 0); unshifted() is the textbook one-pass form (sum l^2 - (sum l)^2 / S) / (S - 1), sums in index
   order.

3. The conditioning cases and their tolerance.  For a column l[S] walked in chunks of L draws, u = 2^-53, in np.longdouble:
       var  the sample variance,   msh = sum_c n_c (mean_c - l0_c)^2 / (S - 1),   D = max_c |mean_c - mean|,
       tol = 4 u [ L (var + msh) + 2 D (max|l| + L sqrt(var + msh)) + chunks var ].
   Derivation (first order in u).  Inside a chunk the shifted terms d = l - l0 are exact or rounded once (u |d|); a1 and a2 are
   recursive sums of n <= L terms, so |err a2| <= L u sum d^2 and |err (a1^2 / n)| <= 2 L u (sum |d|)^2 / n <= 2 L u sum d^2 (Cauchy-
   Schwarz); sum_c sum d^2 = sum_c [M2_c + n_c (mean_c - l0_c)^2] <= (S - 1)(var + msh): the first term, with the factor 4 taking the
   two sums, the squares and the division.  A chunk mean mean_c = l0 + a1 / n is wrong by u |mean_c| + L u rms_c(d) <= u (max|l| +
   L sqrt(var + msh) sqrt(S / n_c)); it enters the merge through delta^2 n nb / tot, whose derivative is 2 |delta| n nb / tot, and
   sum_c 2 |delta_c| w_c <= 2 D (S - 1) with D the largest distance of a chunk mean from the pooled one: the second term.  Every merge
   adds two numbers that are at most the final M2 = (S - 1) var and rounds the product once: chunks roundings of u (S - 1) var: the
   third.  Dividing by S - 1 gives tol.  A host simulation of this arithmetic on fifteen columns (the issue that asked for these
   cases) stayed at <= 0.07 tol; test_pointwise_cases_host asserts 0.25 tol on the committed cases and that the walk without its
   shift misses tol by more than a factor of 100.

   The cases are realised through a real model, so that the device can run them: Gaussian data that holds x = 50 beside ordinary
   points, draws (mu_s, sigma_s = 1).  "concentrated": mu_s = 1e-6 z_s, so the column of x = 50 is -1250.9 +- 5e-5 and those of
   the ordinary points -1.4 +- 1e-6: |l| / sd = 1e6 to 2.5e7, the case the shift exists for.  "+outlier": draw 0 moved so that the
   column of x = 50 holds -3 000.  "bulk": mu_s = 0.3 z_s, columns -1.4 +- 0.3, with one draw at mu = 141 (l = -1e4) or 1 414
   (l = -1e6) at s = 0, at the first draw of chunk 2, or in the middle of chunk 1.  "far_apart": mu_s = 10 (c mod 2) + 1e-6 z_s for
   the draws of chunk c: the chunk means of the x = 50 column are 450 apart and the D term is the largest of the three.  Sizes: S =
   130 (L = 44, three chunks, the last ragged), 65 536 (1 024 chunks of exactly 64) and 65 792 (1 013 chunks of 65, the last 12) --
   the windows a handle of 13 or 256 particles can hold; 65 537, which the host simulation also walked, is a prime and no window."""
import math

import mpmath
import numpy as np

import test_pwplan_host as PL

U = 2.0 ** -53
ld = np.longdouble
DIGITS = 40


# ---- 1. plain references ---------------------------------------------------------------------------------------------------------
def _family(prob):
    from demc_amd import families as F
    return {F.FAM_GAUSSIAN: "gaussian", F.FAM_BINOMIAL: "binomial", F.FAM_MVN_ISO: "mvn_iso", F.FAM_MVN_FULL: "mvn_full"}[prob["fam"]]


def ref_terms(prob, theta):
    """ref[s][i] = log p(y_i | theta_s) at 40 digits on the raw data, rounded to float64 at the end"""
    fam = _family(prob)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, prob["D"])
    N = prob["dims"][0]
    out = np.empty((theta.shape[0], N))
    with mpmath.workdps(DIGITS):
        mpf, log, l2pi = mpmath.mpf, mpmath.log, mpmath.log(2 * mpmath.pi)
        data = np.asarray(prob["data"], dtype=np.float64)
        if fam == "gaussian":
            for s, (mu, sg) in enumerate(theta):
                for i in range(N):
                    z = (mpf(data[i]) - mpf(mu)) / mpf(sg)
                    out[s, i] = float(-z * z / 2 - log(mpf(sg)) - l2pi / 2)
        elif fam == "binomial":
            n, k = data[:N], data[N:]
            lgc = [mpmath.loggamma(mpf(a) + 1) - mpmath.loggamma(mpf(b) + 1) - mpmath.loggamma(mpf(a) - mpf(b) + 1) for a, b in zip(n, k)]
            for s, (p,) in enumerate(theta):
                for i in range(N):
                    out[s, i] = float(lgc[i] + mpf(k[i]) * log(mpf(p)) + (mpf(n[i]) - mpf(k[i])) * mpmath.log1p(-mpf(p)))
        elif fam == "mvn_iso":
            d = prob["dims"][1]
            X = data.reshape(N, d)
            for s, th in enumerate(theta):
                sg = mpf(th[d])
                for i in range(N):
                    q = mpmath.fsum((mpf(X[i, k]) - mpf(th[k])) ** 2 for k in range(d))
                    out[s, i] = float(-d * l2pi / 2 - d * log(sg) - q / (2 * sg * sg))
        else:
            d = prob["dims"][1]
            X = data.reshape(N, d)
            Lc = mpmath.cholesky(mpmath.matrix(np.asarray(prob["Sigma"], dtype=np.float64).tolist()))
            logdet = 2 * mpmath.fsum(log(Lc[k, k]) for k in range(d))
            for s, th in enumerate(theta):
                for i in range(N):
                    z = []  # L z = x - mu by forward substitution
                    for r in range(d):
                        z.append((mpf(X[i, r]) - mpf(th[r]) - mpmath.fsum(Lc[r, k] * z[k] for k in range(r))) / Lc[r, r])
                    out[s, i] = float(-mpmath.fsum(v * v for v in z) / 2 - (d * l2pi + logdet) / 2)
    return out


def closed_terms(prob, theta, cols=None):
    """the same four families in float64 numpy on the raw data; cols: the observations wanted (all of them when None)"""
    fam = _family(prob)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, prob["D"])
    N = prob["dims"][0]
    cols = np.arange(N) if cols is None else np.asarray(cols)
    data = np.asarray(prob["data"], dtype=np.float64)
    if fam == "gaussian":
        x = data[cols]
        return -0.5 * ((x[None, :] - theta[:, :1]) / theta[:, 1:2]) ** 2 - np.log(theta[:, 1:2]) - 0.5 * math.log(2 * math.pi)
    if fam == "binomial":
        n, k = data[:N][cols], data[N:][cols]
        lgc = np.array([math.lgamma(a + 1) - math.lgamma(b + 1) - math.lgamma(a - b + 1) for a, b in zip(n, k)])
        return lgc[None, :] + k[None, :] * np.log(theta) + (n - k)[None, :] * np.log1p(-theta)
    d = prob["dims"][1]
    X = data.reshape(N, d)[cols]
    r = X[None, :, :] - theta[:, None, :d]
    if fam == "mvn_iso":
        sg = theta[:, d][:, None]
        return -0.5 * d * math.log(2 * math.pi) - d * np.log(sg) - (r ** 2).sum(axis=2) / (2 * sg * sg)
    Lc = np.linalg.cholesky(np.asarray(prob["Sigma"], dtype=np.float64))
    z = np.linalg.solve(Lc, r.reshape(-1, d).T).T.reshape(r.shape)
    return -0.5 * (z ** 2).sum(axis=2) - 0.5 * (d * math.log(2 * math.pi) + 2 * np.log(np.diag(Lc)).sum())


def ref_waic(ll):
    """DESIGN.md 5.8 in mpmath at 40 digits: ll[S][N] -> (totals[8], pointwise[N][4]) rounded to float64.  A NaN term makes all four
    values of its observation NaN; a -Inf term makes mean and p_waic (and so elpd) NaN and leaves lppd to the finite draws, -Inf when
    there is none; S = 1 has p_waic NaN, N = 1 has se_elpd NaN; the totals follow by ordinary arithmetic."""
    ll = np.asarray(ll, dtype=np.float64)
    S, N = ll.shape
    nan, inf = float("nan"), float("inf")
    pt = np.empty((N, 4))
    with mpmath.workdps(DIGITS):
        for i in range(N):
            col = ll[:, i]
            if np.isnan(col).any():
                pt[i] = nan
                continue
            fin = [mpmath.mpf(v) for v in col if v != -inf]
            assert all(math.isfinite(v) for v in fin), "+Inf is no log-density"
            if not fin:
                lppd = -inf
            else:
                M = max(fin)
                lppd = M + mpmath.log(mpmath.fsum(mpmath.exp(v - M) for v in fin)) - mpmath.log(S)
            if len(fin) < S or S == 1:
                mean = nan if len(fin) < S else fin[0]
                pw = nan
            else:
                mean = mpmath.fsum(fin) / S
                pw = mpmath.fsum((v - mean) ** 2 for v in fin) / (S - 1)
            pt[i, 0], pt[i, 1], pt[i, 2] = float(lppd), float(pw), float(mean)
            pt[i, 3] = nan if (pw != pw) else (-inf if lppd == -inf else float(lppd - pw))
        # the totals, from the 40-digit values where they are finite (float64 values re-read: their rounding is 1e-16 of each term)
        def total(j):
            c = pt[:, j]
            if np.isnan(c).any():
                return nan
            if (c == -inf).any():
                return -inf
            return mpmath.fsum(mpmath.mpf(v) for v in c)
        elpd, pw, lppd, mean = total(3), total(1), total(0), total(2)
        if N > 1 and elpd == elpd and elpd != -inf:
            ebar = elpd / N
            se = mpmath.sqrt(N * mpmath.fsum((mpmath.mpf(v) - ebar) ** 2 for v in pt[:, 3]) / (N - 1))
        else:
            se = nan
        tot = np.array([float(elpd), float(se), float(pw), float(lppd), float(-2 * elpd), float(-2 * mean), float((pt[:, 1] > 0.4).sum()),
                        float((~(np.isfinite(pt[:, 0]) & np.isfinite(pt[:, 1]))).sum())])
    return tot, pt


# ---- 2. the arithmetic of k_pw_accumulate and k_pw_final --------------------------------------------------------------------------
def _chunked(ll, chunk_len):
    ll = np.asarray(ll)
    if ll.ndim == 1:
        ll = ll[:, None]
    S, N = ll.shape
    L = int(chunk_len)
    C = -(-S // L)
    pad = np.full((C * L, N), np.nan, dtype=ll.dtype)
    pad[:S] = ll
    n_c = np.minimum(L, S - L * np.arange(C))
    return pad.reshape(C, L, N), n_c, S, N, L, C


def kernel_walk(ll, chunk_len, shift=True):
    """ll[S] or ll[S][N], chunk_len -> (lppd, p_waic, mean) as k_pw_accumulate and k_pw_final form them, in float64"""
    pad, n_c, S, N, L, C = _chunked(np.asarray(ll, dtype=np.float64), chunk_len)
    with np.errstate(all="ignore"):
        # k_pw_accumulate: one pass over the draws of a chunk (all chunks and observations side by side, the draws in order)
        l0 = pad[:, 0, :].copy() if shift else np.zeros((C, N))
        a1, a2, E = np.zeros((C, N)), np.zeros((C, N)), np.zeros((C, N))
        M = np.full((C, N), -np.inf)
        flags = np.zeros((C, N), dtype=np.int64)
        for j in range(L):
            act = (j < n_c)[:, None] & np.ones((1, N), dtype=bool)
            l = pad[:, j, :]
            dl = l - l0
            a1 = np.where(act, a1 + dl, a1)
            a2 = np.where(act, a2 + dl * dl, a2)
            isn = act & (l != l)
            ninf = act & (l == -np.inf)
            flags |= np.where(isn, 3, 0) | np.where(ninf, 1, 0)
            fin = act & ~isn & ~ninf
            up = fin & (l > M)
            E = np.where(up, E * np.exp(M - l) + 1.0, np.where(fin, E + np.exp(l - M), E))
            M = np.where(up, l, M)
        n = n_c.astype(np.float64)[:, None]
        mean_c = l0 + a1 / n
        M2_c = a2 - (a1 * a1) / n
        # k_pw_final: the chunks in index order
        Mx = M[0].copy()
        for c in range(1, C):
            Mx = np.where(M[c] > Mx, M[c], Mx)
        Et = np.zeros(N)
        for c in range(C):
            Et = np.where(E[c] != 0.0, Et + E[c] * np.exp(M[c] - Mx), Et)
        Sd = float(S)
        lppd = Mx + np.log(Et) - math.log(Sd)
        nn, mean, M2, fl = float(min(L, S)), mean_c[0].copy(), M2_c[0].copy(), flags[0].copy()
        for c in range(1, C):
            nb = float(n_c[c])
            tot = nn + nb
            delta = mean_c[c] - mean
            mean = mean + delta * (nb / tot)
            M2 = (M2 + M2_c[c]) + (delta * delta) * (nn * nb / tot)
            nn = tot
            fl |= flags[c]
        p_waic = M2 / (Sd - 1.0)
        mean = np.where(fl & 1, np.nan, mean)
        p_waic = np.where(fl & 1, np.nan, p_waic)
        lppd = np.where(fl & 2, np.nan, lppd)
    return lppd, p_waic, mean


def unshifted(ll):
    """(sum l^2 - (sum l)^2 / S) / (S - 1) in float64, the sums in index order (np.cumsum adds one term at a time)"""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim == 1:
        ll = ll[:, None]
    S = ll.shape[0]
    s1, s2 = np.cumsum(ll, axis=0)[-1], np.cumsum(ll * ll, axis=0)[-1]
    return (s2 - (s1 * s1) / S) / (S - 1.0)


# ---- 3. the tolerance and the cases -------------------------------------------------------------------------------------------------
def tolerance(ll, chunk_len):
    """tol of p_waic per column (the formula of the module's docstring), with the column's var, in float64 -> (tol[N], var[N])"""
    pad, n_c, S, N, L, C = _chunked(np.asarray(ll, dtype=np.float64).astype(ld), chunk_len)
    live = (np.arange(L)[None, :] < n_c[:, None])[:, :, None]
    full = np.where(live, pad, ld(0))
    mean = full.sum(axis=(0, 1)) / S
    var = (np.where(live, full - mean, ld(0)) ** 2).sum(axis=(0, 1)) / ld(S - 1)
    mean_c = full.sum(axis=1) / n_c[:, None].astype(ld)
    msh = (n_c[:, None] * (mean_c - pad[:, 0, :]) ** 2).sum(axis=0) / ld(S - 1)
    delta = np.abs(mean_c - mean).max(axis=0)
    amax = np.abs(np.where(live, full, ld(0))).max(axis=(0, 1))
    tol = 4 * ld(U) * (L * (var + msh) + 2 * delta * (amax + L * np.sqrt(var + msh)) + C * var)
    return tol.astype(np.float64), var.astype(np.float64)


X_COND = np.array([50.0, 0.3, -1.1, 1.7, 2.4])  # x = 50 beside ordinary points, none so close to 0 that its column has no spread
# S: the handle that holds the window (n_groups x Np particles, rows) and what geometry() must say about it
COND_SHAPES = {
    130: dict(n_groups=1, Np=13, rows=10, chunks=3, chunk_len=44, last_chunk=42),
    65536: dict(n_groups=16, Np=16, rows=256, chunks=1024, chunk_len=64, last_chunk=64),
    65792: dict(n_groups=16, Np=16, rows=257, chunks=1013, chunk_len=65, last_chunk=12),
}
COND_KINDS = ("concentrated", "concentrated_outlier_s0", "bulk_1e4_s0", "bulk_1e6_chunk2", "bulk_1e4_inside", "far_apart")


def _mu_for(x, l):
    """the mu below x at which the Gaussian term of x with sigma = 1 is l"""
    return x - math.sqrt(2.0 * (-l - 0.5 * math.log(2 * math.pi)))


def conditioning_cases():
    """[dict(name, kind, S, shape, chunk_len, x[N], theta[S][2], concentrated)]: the draws in the order the device walks them (row by
    row of the window, the particles of a row in index order)"""
    out = []
    for S, shape in COND_SHAPES.items():
        g = PL.geometry(len(X_COND), S)
        for k in ("chunks", "chunk_len", "last_chunk"):
            assert g[k] == shape[k], f"S={S}: {k} is {g[k]}, the case was chosen for {shape[k]} -- the constants of csrc/demc_pwplan.hpp moved"
        assert shape["n_groups"] * shape["Np"] * shape["rows"] == S
        L = g["chunk_len"]
        for j, kind in enumerate(COND_KINDS):
            z = np.random.default_rng(7000 + 10 * j + S % 97).standard_normal(S)
            if kind.startswith("concentrated"):
                mu = 1e-6 * z
                if kind.endswith("outlier_s0"):
                    mu[0] = _mu_for(50.0, -3000.0)
            elif kind.startswith("bulk"):
                mu = 0.3 * z
                at = dict(bulk_1e4_s0=0, bulk_1e6_chunk2=2 * L, bulk_1e4_inside=L + L // 2)[kind]
                assert at % L == (L // 2 if kind.endswith("inside") else 0) and at < S
                mu[at] = -_mu_for(0.0, -1e6 if "1e6" in kind else -1e4)  # above every ordinary point: l = -1e4 (-1e6) to within 5 %
            else:
                mu = 10.0 * ((np.arange(S) // L) % 2) + 1e-6 * z
            theta = np.stack([mu, np.ones(S)], axis=1)
            out.append(dict(name=f"{kind}_S{S}", kind=kind, S=S, shape=shape, chunk_len=L, x=X_COND.copy(), theta=theta,
                            concentrated=kind == "concentrated"))
    return out


def cond_problem(case):
    """the Gaussian model spec (conftest.make_problem's layout) of a conditioning case"""
    from demc_amd import families as F
    inf = np.inf
    return dict(fam=F.FAM_GAUSSIAN, data=case["x"], dims=[len(case["x"])], hyper=None, D=2, pk=[1, 2], pa=[0, 0], pb=[10, 1], pref=[0, 0],
                lo=[-inf, 0], hi=[inf, inf])
