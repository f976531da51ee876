"""Minimal stand-in for MCMCChains.Chains: value array (iterations x parameters x chains) + names, and the
summary statistics the reference's tests read from describe(chains)[1] (:mean, :std, :rhat), plus the effective sample size,
its Monte-Carlo standard error and the autocorrelation MCMCChains adds to them (DESIGN.md section 5.5 is the definition; the device
computes the same numbers from the history without exporting it: demc_summarize), the quantile table of describe(chains)
(demc_quantiles on the device), cov(chains) / cor(chains) (demc_covariance), and WAIC from
the per-observation log-densities (demc_waic), PSIS-LOO from the same terms (demc_loo), and the marginal likelihood by
bridge sampling from two vectors of log ratios (demc_bridge), and the rank-normalised diagnostics ess_bulk,
ess_tail and rhat of the pooled, ranked history (demc_rankstats), and the highest-density intervals of
hpd(chains) read off the sorted pool (demc_hpd)."""
import math

import numpy as np

SUMMARY_COLS = ("mean", "std", "rhat", "ess", "mcse", "pairs")  # the columns of demc_summarize's out (DEMC_SUMMARY_COLS)
DEFAULT_QUANTILES = (0.025, 0.25, 0.5, 0.75, 0.975)  # MCMCChains' describe(chains)[2]
COV_MAX_COLS = 64  # DEMC_COV_MAX_COLS: the series one call of demc_covariance takes
WAIC_TOTALS = ("elpd_waic", "se_elpd", "p_waic", "lppd", "waic", "dbar", "n_high", "n_nonfinite")  # demc_waic's total_out, in order
WAIC_POINT = ("lppd", "p_waic", "mean", "elpd")  # the columns of demc_waic's pointwise_out (DEMC_WAIC_NPOINT)


class Summary:
    """The summary table of a run: `values[j]` = (mean, std, rhat, ess, mcse, pairs) of series names[j] -- the parameters,
    then acceptance and lp.  `rho` (or None): [series][lags] autocorrelations, NaN beyond the lags that were evaluated.
    `quantiles` (or None): [series][len(probs)] quantiles at `probs`, chains pooled.  `cov_matrix` / `cor_matrix`
    (or None): the covariance and correlation of the series `cov_names`, chains pooled.  `waic` (or None): the Waic
    record of the same rows.  `loo` (or None): the Loo record of the same rows.
    `bridge` (or None): the Bridge record of the same rows.  `rank` (or None): the RankStats record of the same
    rows -- ess_bulk, ess_tail and the rank-normalised rhat.  `hpd` (or None): the Hpd record of the same rows --
    the highest-density intervals at the alphas the run was summarised with."""

    def __init__(self, names, values, internals=("acceptance", "lp"), rho=None, quantiles=None, probs=None, cov=None, cor=None,
                 cov_names=None, waic=None, loo=None, bridge=None, rank=None, hpd=None):
        self.rank = rank
        self.hpd = hpd
        self.waic = waic
        self.loo = loo
        self.bridge = bridge
        self.names = list(names)
        self.values = np.asarray(values, dtype=np.float64).reshape(len(self.names), len(SUMMARY_COLS))
        self.internals = list(internals)
        self.rho = rho
        self.probs = None if quantiles is None else tuple(float(q) for q in probs)
        self.quantiles = None if quantiles is None else np.asarray(quantiles, dtype=np.float64).reshape(len(self.names), len(self.probs))
        self.cov_names = None if cov_names is None else list(cov_names)
        k = 0 if cov_names is None else len(self.cov_names)
        self.cov_matrix = None if cov is None else np.asarray(cov, dtype=np.float64).reshape(k, k)
        self.cor_matrix = None if cor is None else np.asarray(cor, dtype=np.float64).reshape(k, k)

    def __getitem__(self, name):
        return dict(zip(SUMMARY_COLS, (float(v) for v in self.values[self.names.index(name)])))

    def describe(self):
        """per parameter name the dict Chains.describe() gives (mean, std, rhat), extended by ess, mcse and pairs"""
        return {nm: self[nm] for nm in self.names if nm not in self.internals}

    def quantile(self):
        """per parameter name {q: value} at the probs the run was summarised with: what Chains.quantile(probs) gives"""
        if self.quantiles is None:
            raise ValueError("this Summary holds no quantiles: summarize(..., quantiles=DEFAULT_QUANTILES)")
        return {nm: dict(zip(self.probs, (float(v) for v in self.quantiles[j])))
                for j, nm in enumerate(self.names) if nm not in self.internals}

    def cov(self):
        """(names, matrix): the covariance of the series the run was summarised with -- what Chains.cov(names) gives"""
        if self.cov_matrix is None:
            raise ValueError("this Summary holds no covariance: summarize(..., cor=True)")
        return list(self.cov_names), self.cov_matrix

    def cor(self):
        """(names, matrix): the correlation of the series the run was summarised with -- what Chains.cor(names) gives"""
        if self.cor_matrix is None:
            raise ValueError("this Summary holds no correlation: summarize(..., cor=True)")
        return list(self.cov_names), self.cor_matrix


class Waic:
    """The eight totals of demc_waic by name (WAIC_TOTALS) and, when it was asked for, the table pointwise[N][4] = (lppd_i, p_waic_i,
    mean_i, elpd_i) in the caller's observation order."""

    def __init__(self, totals, pointwise=None):
        totals = np.asarray(totals, dtype=np.float64).reshape(len(WAIC_TOTALS))
        for nm, v in zip(WAIC_TOTALS, totals):
            setattr(self, nm, float(v))
        self.totals = totals
        self.pointwise = None if pointwise is None else np.asarray(pointwise, dtype=np.float64).reshape(-1, len(WAIC_POINT))

    def __repr__(self):
        s = (f"Waic(elpd_waic={self.elpd_waic:.2f} (se {self.se_elpd:.2f}), p_waic={self.p_waic:.2f}, lppd={self.lppd:.2f}, "
             f"waic={self.waic:.2f}, dbar={self.dbar:.2f}")
        if self.n_high:
            s += f", {int(self.n_high)} observations with p_waic > 0.4"
        if self.n_nonfinite:
            s += f", {int(self.n_nonfinite)} observations not finite"
        return s + ")"


def waic_from_loglik(ll):
    """DESIGN.md 5.8 on the host: ll[S][N] = log p(y_i | theta_s) -> Waic with its pointwise table.  The sums over the draws and
    over the observations run in np.longdouble; the results are rounded to float64 at the end."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 1 or ll.shape[1] < 1:
        raise ValueError("waic_from_loglik needs ll[S][N] with S >= 1 and N >= 1")
    S, N = ll.shape
    L = ll.astype(np.longdouble)
    nan = np.longdouble("nan")
    with np.errstate(all="ignore"):
        isnan = np.isnan(L).any(axis=0)
        bad = isnan | np.isneginf(L).any(axis=0)
        M = np.where(isnan, nan, np.max(np.where(np.isnan(L), -np.inf, L), axis=0))
        dead = np.isneginf(M)  # every draw -Inf
        E = np.exp(np.where(np.isneginf(L), -np.inf, L - np.where(dead | isnan, 0, M))).sum(axis=0)
        lppd = np.where(dead, -np.inf, M + np.log(E) - np.log(np.longdouble(S)))
        lppd = np.where(isnan, nan, lppd)
        mean = L.sum(axis=0) / S
        p_waic = ((L - mean) ** 2).sum(axis=0) / np.longdouble(S - 1) if S > 1 else np.full(N, nan)
        mean = np.where(bad, nan, mean)
        p_waic = np.where(bad, nan, p_waic)
        elpd = lppd - p_waic
        ebar = elpd.sum() / N
        se = np.sqrt(N * (((elpd - ebar) ** 2).sum() / np.longdouble(N - 1))) if N > 1 else nan
        totals = [elpd.sum(), se, p_waic.sum(), lppd.sum(), -2 * elpd.sum(), -2 * mean.sum(), float((p_waic > 0.4).sum()),
                  float((~(np.isfinite(lppd) & np.isfinite(p_waic))).sum())]
    return Waic(np.array(totals, dtype=np.float64), np.stack([lppd, p_waic, mean, elpd], axis=1).astype(np.float64))


def compare_waic(a, b):
    """two Waic records (or pointwise tables [N][4]) over the SAME observations -> dict(elpd_diff = sum_i (elpd_i^a - elpd_i^b),
    se_diff = sqrt(N var_i(elpd_i^a - elpd_i^b)), N - 1 in the variance): positive elpd_diff favours a"""
    pa, pb = (np.asarray(x.pointwise if isinstance(x, Waic) else x, dtype=np.float64) for x in (a, b))
    if pa is None or pb is None or pa.ndim != 2 or pa.shape != pb.shape or pa.shape[1] != len(WAIC_POINT):
        raise ValueError("compare_waic needs two pointwise tables [N][4] over the same observations (waic(..., pointwise=True))")
    d = (pa[:, 3] - pb[:, 3]).astype(np.longdouble)
    N = d.size
    with np.errstate(all="ignore"):
        se = float(np.sqrt(N * (((d - d.sum() / N) ** 2).sum() / np.longdouble(N - 1)))) if N > 1 else float("nan")
    return dict(elpd_diff=float(d.sum()), se_diff=se)


_SIGN, _ALL = np.uint64(1 << 63), np.uint64(0xFFFFFFFFFFFFFFFF)
_KEY_NEG_INF, _KEY_POS_INF = np.uint64(0x000FFFFFFFFFFFFF), np.uint64(0xFFF0000000000000)  # NaNs are the keys beyond them


def series_quantiles(x, probs):
    """DESIGN.md 5.6 for one series on the host: x (any shape; the chains are pooled) -> the quantiles at probs, Julia's default
    (type 7) on the values ordered by their keys, to the operation -- what demc_quantiles selects on the device, bit for bit"""
    b = np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)
    N = b.size
    if N < 1:
        raise ValueError("series_quantiles needs at least one value")
    k = np.sort(b ^ np.where(b >> np.uint64(63) != 0, _ALL, _SIGN))
    out = np.full(len(probs), float("nan"))
    if k[0] < _KEY_NEG_INF or k[-1] > _KEY_POS_INF:  # a NaN in the pool
        return out
    v = (k ^ np.where(k >> np.uint64(63) != 0, _SIGN, _ALL)).view(np.float64)  # x_(1) <= ... <= x_(N)
    with np.errstate(all="ignore"):
        for i, p in enumerate(probs):
            p = float(p)
            if not 0.0 <= p <= 1.0:
                raise ValueError("a prob is outside [0, 1]")
            if N == 1:
                out[i] = v[0]
                continue
            aleph = float(N) * p + (1.0 - p)
            j = max(1, min(int(math.trunc(aleph)), N - 1))
            g = min(1.0, max(0.0, aleph - j))
            a, c = float(v[j - 1]), float(v[j])
            if math.isfinite(a) and math.isfinite(c):
                d = np.float64(c) - np.float64(a)  # (numpy scalars: an overflow is an inf by IEEE, not an exception)
                out[i] = np.float64(a) + np.float64(g) * d
            elif g == 0.0:
                out[i] = a
            elif g == 1.0:
                out[i] = c
            else:
                out[i] = np.float64(1.0 - g) * np.float64(a) + np.float64(g) * np.float64(c)
    return out


def series_cov(value, cols=None):
    """DESIGN.md 5.7 on the host: value[n][series][chains] (the Chains value array), cols (None: every series) -> (mean[K], cov[K][K],
    cor[K][K]) of the selected series, the chains pooled -- the corrected two-pass form demc_covariance computes on the device, in
    FP64 with numpy's summation order"""
    value = np.asarray(value, dtype=np.float64)
    cols = list(range(value.shape[1])) if cols is None else [int(c) for c in cols]
    K = len(cols)
    if not 1 <= K or len(set(cols)) != K or min(cols) < 0 or max(cols) >= value.shape[1]:
        raise ValueError("series_cov needs distinct series of the value array, at least one")
    x = np.stack([value[:, c, :].reshape(-1) for c in cols], axis=1)  # [N][K]
    N = x.shape[0]
    if N < 1:
        raise ValueError("series_cov needs at least one row")
    nan = float("nan")
    with np.errstate(all="ignore"):
        mhat = x.sum(axis=0) / float(N)
        c = x - mhat
        s = c.sum(axis=0)
        Q = np.einsum("ei,ej->ij", c, c)  # (not c.T @ c: a NaN column must stay in its own row and column whatever BLAS does)
        S = Q - np.outer(s, s) / float(N)
        S = np.triu(S) + np.triu(S, 1).T
        mean = mhat + s / float(N)
        if N == 1:
            return mean, np.full((K, K), nan), np.full((K, K), nan)
        cov = S / float(N - 1)
        d = np.sqrt(np.diag(S))
        cor = S / (d[:, None] * d[None, :])
        cor = np.where(cor < -1.0, -1.0, np.where(cor > 1.0, 1.0, cor))
        dg = np.diag(S)
        cor[np.arange(K), np.arange(K)] = np.where(np.isfinite(dg) & (dg > 0.0), 1.0, nan)
    return mean, cov, cor


def series_summary(x, max_lag=0, rho_len=0):
    """DESIGN.md 5.5 for one series x[n][m] (iterations x chains) on the host -> ((mean, std, rhat, ess, mcse, pairs), rho)"""
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    nan = float("nan")
    with np.errstate(all="ignore"):
        mean = x.sum() / (n * m)
        std = float(np.sqrt(((x - mean) ** 2).sum() / (n * m - 1))) if n * m > 1 else nan
        rho = np.full(rho_len, nan)
        h = n // 2
        if h < 2:
            return (float(mean), std, nan, nan, nan, 0.0), rho
        s = np.concatenate([x[:h], x[h:2 * h]], axis=1)  # [h][M]
        M = 2 * m
        y = s - s.sum(axis=0) / h
        W = ((y * y).sum(axis=0) / h).mean() * h / (h - 1)
        mu = s.sum(axis=0) / h
        bh = ((mu - mu.mean()) ** 2).sum() / (M - 1)
        vplus = W * (h - 1) / h + bh
        rhat = float(np.sqrt(vplus / W)) if W != 0 else nan
        L = min(h - 1, max_lag) if max_lag > 0 else h - 1

        def rho_t(t):
            if t == 0:
                return 1.0
            return 1.0 - (W - ((y[:h - t] * y[t:]).sum(axis=0) / h).mean()) / vplus

        def fill(b_last):  # the device evaluates whole blocks of 64 lags, up to the block in which the sequence ended
            for t in range(min(rho_len, L + 1, 64 * (b_last + 1))):
                rho[t] = rho_t(t)

        if h < 4 or W == 0:
            fill(0)
            return (float(mean), std, rhat, nan, nan, 0.0), rho
        K, total, prev, bad, b_last = 0, 0.0, 0.0, False, L // 64
        while 2 * K + 1 <= L:
            P = rho_t(2 * K) + rho_t(2 * K + 1)
            if not P >= 0:  # the first negative pair is excluded; a NaN pair ends the sequence too, and ess is NaN
                bad = not P < 0
                b_last = (2 * K) // 64
                break
            if K > 0:
                P = min(P, prev)
            total += P
            prev = P
            K += 1
        fill(b_last)
        tau = max(-1.0 + 2.0 * total, 1.0 / np.log10(M * h))
        ess = nan if bad else M * h / tau
        return (float(mean), std, rhat, float(ess), float(std / np.sqrt(ess)), float(K)), rho


class Chains:
    def __init__(self, value, names, parameters, internals=("acceptance", "lp")):
        self.value = np.asarray(value)  # [Ns][n_parms + 2][n_chains]
        self.names = list(names)
        self.parameters = list(parameters)
        self.internals = list(internals)

    def __len__(self):  # length(chains) == number of kept iterations (test/utility_tests.jl:34-39)
        return self.value.shape[0]

    def __getitem__(self, name):
        return self.value[:, self.names.index(name), :]

    @staticmethod
    def _rhat(x):
        """split-R-hat over chains (Vehtari et al. 2021, rank-free form)."""
        n, m = x.shape
        h = n // 2
        if h < 2:
            return np.nan
        s = np.concatenate([x[:h], x[h:2 * h]], axis=1)
        w = s.var(axis=0, ddof=1).mean()
        b = h * s.mean(axis=0).var(ddof=1)
        if w == 0:
            return np.nan
        return float(np.sqrt(((h - 1) / h * w + b / h) / w))

    def describe(self):
        out = {}
        for j, nm in enumerate(self.names):
            if nm in self.internals:
                continue
            x = self.value[:, j, :]
            out[nm] = dict(mean=float(x.mean()), std=float(x.std(ddof=1)), rhat=self._rhat(x))
        return out

    def mean(self):
        return {k: v["mean"] for k, v in self.describe().items()}

    def quantile(self, q=DEFAULT_QUANTILES):
        """per parameter name {q: value}, the chains pooled as MCMCChains' quantile(chains) pools them"""
        q = tuple(float(v) for v in q)
        return {nm: dict(zip(q, (float(v) for v in series_quantiles(self.value[:, j, :], q))))
                for j, nm in enumerate(self.names) if nm not in self.internals}

    def _cols(self, names):
        """the series a covariance call selects: None -> the parameters; names may hold the internals too"""
        names = [nm for nm in self.names if nm not in self.internals] if names is None else list(names)
        return names, [self.names.index(nm) for nm in names]

    def cov(self, names=None):
        """(names, matrix): the sample covariance of the parameters (or of the series `names`), the chains pooled as
        cov(Array(chains)) pools them"""
        names, cols = self._cols(names)
        return names, series_cov(self.value, cols)[1]

    def cor(self, names=None):
        """(names, matrix): the correlation matrix that goes with cov()"""
        names, cols = self._cols(names)
        return names, series_cov(self.value, cols)[2]

    def summarystats(self, max_lag=0, rho_len=0):
        """The Summary of this object computed on the host (numpy): what demc_summarize computes on the device for a history that
        was never exported.  max_lag > 0 caps the lags of Geyer's sequence; rho_len > 0 also keeps that many autocorrelations."""
        rows, rhos = [], []
        for j in range(len(self.names)):
            vals, rho = series_summary(self.value[:, j, :], max_lag, rho_len)
            rows.append(vals)
            rhos.append(rho)
        return Summary(self.names, rows, self.internals, np.stack(rhos) if rho_len > 0 else None)

    def rankstats(self, max_lag=0):
        """The RankStats of this object computed on the host (numpy): what demc_rankstats computes on the device for a history that
        was never exported."""
        return RankStats(self.names, [series_rankstats(self.value[:, j, :], max_lag) for j in range(len(self.names))], self.internals)

    def hpd(self, alpha=0.05):
        """The Hpd of this object computed on the host (numpy): MCMCChains' hpd(chains; alpha) with the chains pooled, one row per
        series with lower and upper -- what demc_hpd computes on the device for a history that was never exported.
        alpha: one value or a tuple of them."""
        alphas = hpd_alphas(alpha)
        return Hpd(self.names, [series_hpd(self.value[:, j, :], alphas) for j in range(len(self.names))], alphas, self.internals)


# ---- rank-normalised diagnostics (demc_rankstats on the device) -------------------------------------------
RANK_COLS = ("rhat", "ess_bulk", "ess_tail", "rhat_bulk", "rhat_folded", "ess_q05", "ess_q95", "distinct")  # demc_rankstats' out (DEMC_RANK_COLS)
RANK_PROBS = (0.5, 0.05, 0.95)  # med, q05, q95

_PPND_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
           1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e0)
_PPND_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
           5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_PPND_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e0,
           3.64784832476320460504e0, 5.76949722146069140550e0, 4.63033784615654529590e0, 1.42343711074968357734e0)
_PPND_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
           6.89767334985100004550e-1, 1.67638483018380384940e0, 2.05319162663775882187e0, 1.0)
_PPND_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
           2.96560571828504891230e-1, 1.78482653991729133580e0, 5.46378491116411436990e0, 6.65790464350110377720e0)
_PPND_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
           1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _horner(r, c):  # s = s r + c, a multiplication then an addition: the operation order of csrc/demc_ppnd.hpp
    s = np.full_like(r, c[0])
    for ck in c[1:]:
        s = s * r + ck
    return s


def ppnd16(p):
    """the inverse of the standard normal distribution function, Wichura's AS 241 (PPND16), vectorised in the operation order of
    csrc/demc_ppnd.hpp: the text the device runs, restated in numpy.  p = 0 -> -inf, 1 -> +inf, outside [0, 1] or NaN -> NaN"""
    p = np.asarray(p, dtype=np.float64)
    shape = p.shape
    p = p.reshape(-1)
    out = np.full(p.shape, float("nan"))
    with np.errstate(all="ignore"):
        ok = (p >= 0.0) & (p <= 1.0)
        q = p - 0.5
        mid = ok & (np.abs(q) <= 0.425)
        qm = q[mid]
        r = 0.180625 - qm * qm
        out[mid] = qm * _horner(r, _PPND_A) / _horner(r, _PPND_B)
        tail = ok & ~mid
        pt, qt = p[tail], q[tail]
        r = np.sqrt(-np.log(np.where(qt < 0.0, pt, 1.0 - pt)))
        z = np.empty_like(r)
        near = r <= 5.0
        rn = r[near] - 1.6
        z[near] = _horner(rn, _PPND_C) / _horner(rn, _PPND_D)
        rf = r[~near] - 5.0
        z[~near] = _horner(rf, _PPND_E) / _horner(rf, _PPND_F)
        z[~(r < 1.0e300)] = float("inf")
        out[tail] = np.where(qt < 0.0, -z, z)
    return out.reshape(shape)


def series_keys(x):
    """the 64-bit keys of DESIGN.md 5.6, compared unsigned: the IEEE order with -0.0 before +0.0 and the NaNs beyond the infinities"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, _ALL, _SIGN)


def series_ranks(x):
    """x (any shape; the chains are pooled) -> (r with x's shape, distinct, has_nan): the average
    rank r = L + (E + 1) / 2 of every value among the keys of the pool, the number of distinct keys, whether a key is a NaN's"""
    x = np.asarray(x, dtype=np.float64)
    k = series_keys(x).reshape(-1)
    if k.size < 1:
        raise ValueError("series_ranks needs at least one value")
    ks = np.sort(k)
    lo = np.searchsorted(ks, k, side="left")
    hi = np.searchsorted(ks, k, side="right")
    r = lo.astype(np.float64) + ((hi - lo).astype(np.float64) + 1.0) / 2.0
    distinct = 1 + int(np.count_nonzero(ks[1:] != ks[:-1]))
    return r.reshape(x.shape), distinct, bool(ks[0] < _KEY_NEG_INF or ks[-1] > _KEY_POS_INF)


def normal_scores(r, N):
    """step 3: z = Phi^-1((r - 3/8) / (N + 1/4)), evaluated as written"""
    return ppnd16((np.asarray(r, dtype=np.float64) - 0.375) / (float(N) + 0.25))


def series_rankstats(x, max_lag=0):
    """DESIGN.md 5.11 for one series x[n][m] (iterations x chains) on the host -> (rhat, ess_bulk, ess_tail, rhat_bulk, rhat_folded,
    ess_q05, ess_q95, distinct): the keys sorted, AS 241 for the scores, series_summary and series_quantiles for the rest -- what
    demc_rankstats computes on the device"""
    x = np.asarray(x, dtype=np.float64)
    nan = float("nan")
    N = x.size
    r, distinct, has_nan = series_ranks(x)
    if has_nan:
        return (nan,) * len(RANK_COLS)
    bulk = series_summary(normal_scores(r, N), max_lag)[0]
    med, q05, q95 = (float(v) for v in series_quantiles(x, RANK_PROBS))
    with np.errstate(all="ignore"):
        zeta = np.abs(x - med)
    r2, _, nan2 = series_ranks(zeta)
    rhat_folded = nan if nan2 else series_summary(normal_scores(r2, N), max_lag)[0][2]
    e05 = series_summary((x <= q05).astype(np.float64), max_lag)[0][3]
    e95 = series_summary((x <= q95).astype(np.float64), max_lag)[0][3]
    rhat = nan if math.isnan(bulk[2]) or math.isnan(rhat_folded) else max(bulk[2], rhat_folded)
    ess_tail = nan if math.isnan(e05) or math.isnan(e95) else min(e05, e95)
    return (float(rhat), float(bulk[3]), float(ess_tail), float(bulk[2]), float(rhat_folded), float(e05), float(e95), float(distinct))


class RankStats:
    """The rank-normalised diagnostics of a run (Vehtari et al. 2021): `values[j]` = (rhat, ess_bulk, ess_tail,
    rhat_bulk, rhat_folded, ess_q05, ess_q95, distinct) of series names[j] -- the parameters, then acceptance and lp."""

    def __init__(self, names, values, internals=("acceptance", "lp")):
        self.names = list(names)
        self.values = np.asarray(values, dtype=np.float64).reshape(len(self.names), len(RANK_COLS))
        self.internals = list(internals)

    def __getitem__(self, name):
        return dict(zip(RANK_COLS, (float(v) for v in self.values[self.names.index(name)])))

    def describe(self):
        """per parameter name {rhat, ess_bulk, ess_tail}: the three columns MCMCChains.summarystats reports"""
        return {nm: {c: self[nm][c] for c in RANK_COLS[:3]} for nm in self.names if nm not in self.internals}

    def __repr__(self):
        rows = [f"  {nm:>12s}  rhat {v[0]:.4f}  ess_bulk {v[1]:.1f}  ess_tail {v[2]:.1f}" for nm, v in zip(self.names, self.values)]
        return "RankStats(\n" + "\n".join(rows) + "\n)"


# ---- highest-density intervals (demc_hpd on the device) ------------------------------------------------------
HPD_COLS = ("lower", "upper", "first", "m")  # demc_hpd's out (DEMC_HPD_COLS): first is the 0-based sorted position of lower
HPD_MAX_ALPHAS = 16  # DEMC_HPD_MAX_ALPHAS


def hpd_alphas(alpha):
    alphas = tuple(float(a) for a in (alpha if isinstance(alpha, (tuple, list, np.ndarray)) else (alpha,)))
    if not 1 <= len(alphas) <= HPD_MAX_ALPHAS or not all(math.isfinite(a) and 0.0 < a < 1.0 for a in alphas):
        raise ValueError(f"hpd takes between 1 and {HPD_MAX_ALPHAS} alphas, each strictly inside (0, 1)")
    return alphas


def hpd_candidates(N, alpha):
    """m = max(1, ceil(alpha N)): the product is one rounded double multiplication of alpha, as passed, by float(N)"""
    return max(1, math.ceil(float(np.float64(alpha) * np.float64(N))))


def series_hpd(x, alphas):
    """DESIGN.md 5.12 for one series x (any shape; the chains are pooled) on the host -> [len(alphas)][4] over HPD_COLS: the pool
    sorted by key, the m = max(1, ceil(alpha N)) candidates [y[i], y[N - m + i]], their widths by one subtraction each, and the
    first minimum in the order of Julia's findmin -- what demc_hpd computes on the device"""
    x = np.asarray(x, dtype=np.float64)
    k = np.sort(series_keys(x).reshape(-1))
    N = k.size
    if N < 1:
        raise ValueError("series_hpd needs at least one value")
    has_nan = bool(k[0] < _KEY_NEG_INF or k[-1] > _KEY_POS_INF)
    y = (k ^ np.where(k >> np.uint64(63) != 0, _SIGN, _ALL)).view(np.float64)  # y[0] <= ... <= y[N - 1], -0.0 before +0.0
    nan = float("nan")
    out = np.empty((len(alphas), len(HPD_COLS)))
    for a, alpha in enumerate(alphas):
        m = hpd_candidates(N, alpha)
        assert 1 <= m <= N
        if has_nan:
            out[a] = (nan, nan, nan, float(m))
            continue
        with np.errstate(all="ignore"):
            w = y[N - m:] - y[:m]  # inf - inf of one sign: NaN
        isnan = np.isnan(w)
        if isnan.any():  # a NaN width ranks below every number: the first of them (np.argmin is not asked what it does with NaN)
            i = int(np.flatnonzero(isnan)[0])
        else:  # compared by value; among equal widths the smallest i
            i = int(np.flatnonzero(w == w.min())[0])
        out[a] = (y[i], y[N - m + i], float(i), float(m))
    return out


class Hpd:
    """The highest-density intervals of a run (MCMCChains' hpd, chains pooled): `values[j][k]` = (lower, upper, first,
    m) of series names[j] -- the parameters, then acceptance and lp -- at alphas[k]."""

    def __init__(self, names, values, alphas, internals=("acceptance", "lp")):
        self.names = list(names)
        self.alphas = tuple(float(a) for a in alphas)
        self.values = np.asarray(values, dtype=np.float64).reshape(len(self.names), len(self.alphas), len(HPD_COLS))
        self.internals = list(internals)

    def __getitem__(self, name):
        """the four columns by name; with several alphas {alpha: columns}"""
        rows = [dict(zip(HPD_COLS, (float(v) for v in row))) for row in self.values[self.names.index(name)]]
        return rows[0] if len(rows) == 1 else dict(zip(self.alphas, rows))

    def describe(self):
        """per parameter name {lower, upper} (with several alphas {alpha: {lower, upper}}): the two columns MCMCChains.hpd reports"""
        def two(d):
            return {c: d[c] for c in HPD_COLS[:2]}
        return {nm: two(self[nm]) if len(self.alphas) == 1 else {a: two(d) for a, d in self[nm].items()}
                for nm in self.names if nm not in self.internals}

    def __repr__(self):
        rows = [f"  {nm:>12s}  " + "  ".join(f"{100 * (1 - a):g}% [{v[0]:.4f}, {v[1]:.4f}]" for a, v in zip(self.alphas, vs))
                for nm, vs in zip(self.names, self.values)]
        return "Hpd(\n" + "\n".join(rows) + "\n)"


# ---- PSIS-LOO (demc_loo on the device) ------------------------------------------------------------------

LOO_TOTALS = ("elpd_loo", "se_elpd", "p_loo", "lppd", "looic", "n_k_high", "n_k_bad", "n_nonfinite")  # demc_loo's total_out, in order
LOO_POINT = ("elpd_loo", "p_loo", "khat", "lppd", "n_tail", "l_cut")  # the columns of demc_loo's pointwise_out (DEMC_LOO_NPOINT)
LOO_LOG_MIN = -708.3964185322641  # log(DBL_MIN) rounded to FP64: the floor of a shifted log ratio


class Loo:
    """The eight totals of demc_loo by name (LOO_TOTALS) and, when it was asked for, the table pointwise[N][6] = (elpd_loo_i, p_loo_i,
    khat_i, lppd_i, n_tail_i, l_cut_i) in the caller's observation order."""

    def __init__(self, totals, pointwise=None):
        totals = np.asarray(totals, dtype=np.float64).reshape(len(LOO_TOTALS))
        for nm, v in zip(LOO_TOTALS, totals):
            setattr(self, nm, float(v))
        self.totals = totals
        self.pointwise = None if pointwise is None else np.asarray(pointwise, dtype=np.float64).reshape(-1, len(LOO_POINT))

    def __repr__(self):
        s = (f"Loo(elpd_loo={self.elpd_loo:.2f} (se {self.se_elpd:.2f}), p_loo={self.p_loo:.2f}, lppd={self.lppd:.2f}, "
             f"looic={self.looic:.2f}")
        if self.n_k_high:
            s += f", {int(self.n_k_high)} observations with khat > 0.7 ({int(self.n_k_bad)} above 1)"
        if self.n_nonfinite:
            s += f", {int(self.n_nonfinite)} observations not finite"
        return s + ")"


def loo_tail_len(S):
    """M = ceil(min(0.2 S, 3 sqrt(S))) in FP64 as written"""
    return int(math.ceil(min(0.2 * float(S), 3.0 * math.sqrt(float(S)))))


def psis_fit(e):
    """the Zhang-Stephens profile fit of DESIGN.md 5.9: e_(1) <= ... <= e_(n), n > 4 and e_(q) > 0 -> (khat, sigma); the sums over
    the tail and over the profile points run in np.longdouble"""
    e = np.asarray(e, dtype=np.float64)
    n = e.size
    m = 30 + int(math.floor(math.sqrt(float(n))))
    q = int(math.floor(n / 4.0 + 0.5))
    j = np.arange(1, m + 1, dtype=np.float64)
    b = (1.0 - np.sqrt(float(m) / (j - 0.5))) / (3.0 * e[q - 1]) + 1.0 / e[n - 1]
    L_ = e.astype(np.longdouble)
    with np.errstate(all="ignore"):
        k = np.array([np.log1p(-np.longdouble(bj) * L_).sum() / n for bj in b], dtype=np.longdouble)
        Lj = n * (np.log(-b.astype(np.longdouble) / k) - k - 1)
        w = np.array([1 / np.exp(Lj - Lj[i]).sum() for i in range(m)], dtype=np.longdouble)
        bhat = (b.astype(np.longdouble) * w).sum()
        kk = np.log1p(-bhat * L_).sum() / n
        sigma = -kk / bhat
        khat = (n * kk + 5) / (n + 10)
    return float(khat), float(sigma)


def psis_smooth(khat, sigma, n, exc):
    """the smoothed shifted log weights of a fitted tail: x~_(t) = min(log(g_t + exc), 0), g_t the generalised Pareto quantile at
    p_t = (t - 0.5) / n (khat == 0: the exponential limit), exc = exp(x_cut)"""
    p = (np.arange(1, n + 1, dtype=np.float64) - 0.5) / float(n)
    with np.errstate(all="ignore"):
        lq = np.log1p(-p)
        g = -sigma * lq if khat == 0.0 else sigma * np.expm1(-khat * lq) / khat
        return np.minimum(np.log(g + exc), 0.0)


def _loo_column(l):
    """one observation: l[S] float64 without NaN, +Inf or -Inf -> (elpd_loo, khat, n_tail, l_cut)"""
    S = l.size
    nan, inf = float("nan"), float("inf")
    b = l.view(np.uint64)
    order = np.argsort(b ^ np.where(b >> np.uint64(63) != 0, _ALL, _SIGN), kind="stable")  # the key order of section 5.6
    ls = l[order]
    lmin = ls[0]
    x = lmin - ls  # descending from 0
    n2, l_cut, khat = 0, nan, inf
    xt = np.empty(0)
    if S > 20:
        M = loo_tail_len(S)
        l_cut = ls[M]
        x_cut = max(lmin - l_cut, LOO_LOG_MIN)
        n2 = int((x > x_cut).sum())  # a prefix of the ordered terms: ties at the cutoff and floored ratios stay outside
        xt = x[:n2][::-1].copy()  # x ascending
        if n2 > 4:
            with np.errstate(all="ignore"):
                exc = np.exp(x_cut)
                e = np.exp(xt) - exc
            if e[int(math.floor(n2 / 4.0 + 0.5)) - 1] > 0.0:
                khat, sigma = psis_fit(e)
                xt = psis_smooth(khat, sigma, n2, exc)
    lt = ls[:n2][::-1]
    xo, lo = x[n2:].astype(np.longdouble), ls[n2:].astype(np.longdouble)
    v = xt.astype(np.longdouble) + lt.astype(np.longdouble)
    shift = max(np.longdouble(lmin), v.max()) if n2 else np.longdouble(lmin)
    with np.errstate(all="ignore"):
        num = np.exp((xo + lo) - shift).sum() + np.exp(v - shift).sum()
        den = np.exp(xo).sum() + np.exp(xt.astype(np.longdouble)).sum()
        elpd = shift + (np.log(num) - np.log(den))
    return float(elpd), khat, n2, float(l_cut)


def loo_from_loglik(ll):
    """DESIGN.md 5.9 on the host: ll[S][N] = log p(y_i | theta_s) -> Loo with its pointwise table.  The selection is exact (a sort by
    the keys of section 5.6); the sums over the draws, the tail and the observations run in np.longdouble, and the results are
    rounded to float64 at the end."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[0] < 1 or ll.shape[1] < 1:
        raise ValueError("loo_from_loglik needs ll[S][N] with S >= 1 and N >= 1")
    S, N = ll.shape
    nan, inf = float("nan"), float("inf")
    lppd = waic_from_loglik(np.where(np.isposinf(ll), nan, ll)).pointwise[:, 0]
    pt = np.empty((N, len(LOO_POINT)))
    with np.errstate(all="ignore"):
        for i in range(N):
            col = np.ascontiguousarray(ll[:, i])
            if np.isnan(col).any() or np.isposinf(col).any():
                pt[i] = nan
            elif np.isneginf(col).any():
                pt[i] = (-inf, np.float64(lppd[i]) - np.float64(-inf), inf, lppd[i], 0.0, -inf)
            else:
                elpd, khat, n2, l_cut = _loo_column(col)
                pt[i] = (elpd, np.float64(lppd[i]) - np.float64(elpd), khat, lppd[i], float(n2), l_cut)
        e = pt[:, 0].astype(np.longdouble)
        se = float(np.sqrt(N * (((e - e.sum() / N) ** 2).sum() / np.longdouble(N - 1)))) if N > 1 else nan
        totals = [float(e.sum()), se, float(pt[:, 1].astype(np.longdouble).sum()), float(pt[:, 3].astype(np.longdouble).sum()), float(-2 * e.sum()),
                  float((pt[:, 2] > 0.7).sum()), float((pt[:, 2] > 1.0).sum()), float((~(np.isfinite(pt[:, 0]) & np.isfinite(pt[:, 3]))).sum())]
    return Loo(np.array(totals, dtype=np.float64), pt)


def compare_loo(a, b):
    """two Loo records (or pointwise tables [N][6]) over the SAME observations -> dict(elpd_diff = sum_i (elpd_loo_i^a - elpd_loo_i^b),
    se_diff = sqrt(N var_i(elpd_loo_i^a - elpd_loo_i^b)), N - 1 in the variance): positive elpd_diff favours a"""
    pa, pb = (x.pointwise if isinstance(x, Loo) else x for x in (a, b))
    if pa is None or pb is None:
        raise ValueError("compare_loo needs two pointwise tables [N][6] over the same observations (loo(..., pointwise=True))")
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    if pa.ndim != 2 or pa.shape != pb.shape or pa.shape[1] != len(LOO_POINT):
        raise ValueError("compare_loo needs two pointwise tables [N][6] over the same observations (loo(..., pointwise=True))")
    d = (pa[:, 0] - pb[:, 0]).astype(np.longdouble)
    N = d.size
    with np.errstate(all="ignore"):
        se = float(np.sqrt(N * (((d - d.sum() / N) ** 2).sum() / np.longdouble(N - 1)))) if N > 1 else float("nan")
    return dict(elpd_diff=float(d.sum()), se_diff=se)


# ---- the marginal likelihood by bridge sampling (demc_bridge on the device) --------------------------------

BRIDGE_OUT = ("logml", "re2_prop", "re2_post_iid", "n_iter", "converged", "n_fit", "n1", "n2", "l_star", "n_zero_prop", "n_nonfinite",
              "rel_change")  # demc_bridge's out, in order (DEMC_BRIDGE_NOUT)
BRIDGE_STREAM = 7  # the Philox stream of the proposal draws
BRIDGE_TOL, BRIDGE_MAX_ITER = 1e-10, 1000


class Bridge:
    """The twelve values of demc_bridge by name (BRIDGE_OUT) and, when the diagnostics were asked for, the device's own stages:
    prop[N2][D+3] = (theta, lp, logJ, log g) of the proposal draws, post[N1][3] = (lp, logJ, log g) of the estimate half, fit = (m, L).
    `rho` is the autocorrelation factor se() is scaled by when none is given to compare_bridge (1: independent draws)."""

    def __init__(self, out, prop=None, post=None, fit=None, rho=1.0):
        out = np.asarray(out, dtype=np.float64).reshape(len(BRIDGE_OUT))
        for nm, v in zip(BRIDGE_OUT, out):
            setattr(self, nm, float(v))
        self.out = out
        self.prop, self.post, self.fit = prop, post, fit
        self.rho = float(rho)

    def se(self, rho=1.0):
        """the approximate standard error of logml: sqrt(re2_prop + rho re2_post_iid), rho the autocorrelation factor of the posterior
        draws (kept draws / effective draws; 1: independent)"""
        return math.sqrt(self.re2_prop + rho * self.re2_post_iid)

    def __repr__(self):
        s = f"Bridge(logml={self.logml:.4f} (se {self.se(self.rho):.4f}), {int(self.n_iter)} iterations"
        if not self.converged:
            s += ", NOT converged"
        if self.n_zero_prop:
            s += f", {int(self.n_zero_prop)} of {int(self.n2)} proposal draws outside the support"
        if self.n_nonfinite:
            s += f", {int(self.n_nonfinite)} log ratios not finite"
        return s + ")"


def _bridge_bounds(D, lo, hi):
    lo = np.full(D, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64).reshape(D)
    hi = np.full(D, np.inf) if hi is None else np.asarray(hi, dtype=np.float64).reshape(D)
    return lo, hi, (lo > -np.inf).astype(int) + 2 * (hi < np.inf).astype(int)  # 0 none, 1 lower, 2 upper, 3 both


def _bridge_logjac(xi, lo, hi, kind):
    lj = np.zeros(xi.shape[0])
    for k in range(xi.shape[1]):
        x = xi[:, k]
        if kind[k] in (1, 2):
            lj = lj + x
        elif kind[k] == 3:
            a = np.abs(x)
            lj = lj + (math.log(hi[k] - lo[k]) - a - 2.0 * np.log1p(np.exp(-a)))
    return lj


def bridge_transform(theta, lo=None, hi=None):
    """theta[n][D] and the bounds -> (xi[n][D], logJ[n]) of DESIGN.md 5.10; a draw on or outside a finite bound gives a xi that is not finite"""
    theta = np.asarray(theta, dtype=np.float64)
    lo, hi, kind = _bridge_bounds(theta.shape[1], lo, hi)
    xi = theta.copy()
    with np.errstate(all="ignore"):
        for k in range(theta.shape[1]):
            t = theta[:, k]
            if kind[k] == 1:
                xi[:, k] = np.log(t - lo[k])
            elif kind[k] == 2:
                xi[:, k] = np.log(hi[k] - t)
            elif kind[k] == 3:
                u = (t - lo[k]) / (hi[k] - lo[k])
                xi[:, k] = np.log(u) - np.log1p(-u)
        return xi, _bridge_logjac(xi, lo, hi, kind)


def bridge_inverse(xi, lo=None, hi=None):
    """xi[n][D] -> (theta[n][D], logJ[n])"""
    xi = np.asarray(xi, dtype=np.float64)
    lo, hi, kind = _bridge_bounds(xi.shape[1], lo, hi)
    th = xi.copy()
    with np.errstate(all="ignore"):
        for k in range(xi.shape[1]):
            x = xi[:, k]
            if kind[k] == 1:
                th[:, k] = lo[k] + np.exp(x)
            elif kind[k] == 2:
                th[:, k] = hi[k] - np.exp(x)
            elif kind[k] == 3:
                th[:, k] = lo[k] + (hi[k] - lo[k]) / (1.0 + np.exp(-x))
        return th, _bridge_logjac(xi, lo, hi, kind)


def bridge_cholesky(V):
    """the lower factor of V column by column, the sums in index order (csrc/demc_bridgeplan.hpp); ValueError at a pivot that is not positive"""
    V = np.asarray(V, dtype=np.float64)
    D = V.shape[0]
    L = np.zeros((D, D))
    for j in range(D):
        s = V[j, j]
        for k in range(j):
            s -= L[j, k] * L[j, k]
        if not (s > 0.0) or not math.isfinite(s):
            raise ValueError(f"bridge_cholesky: pivot {j} of {D} is not positive")
        L[j, j] = math.sqrt(s)
        for i in range(j + 1, D):
            t = V[i, j]
            for k in range(j):
                t -= L[i, k] * L[j, k]
            L[i, j] = t / L[j, j]
    return L


def bridge_fit(xi):
    """xi[n][D] of the fit half -> (m[D], L[D][D]): the mean, and the lower Cholesky factor of the covariance (n - 1 divisor, the
    corrected two-pass form of DESIGN.md 5.7, sums in np.longdouble)"""
    x = np.asarray(xi, dtype=np.float64).astype(np.longdouble)
    n = x.shape[0]
    mhat = x.sum(axis=0) / n
    c = x - mhat
    s = c.sum(axis=0)
    S = c.T @ c - np.outer(s, s) / n
    return (mhat + s / n).astype(np.float64), bridge_cholesky((S / (n - 1)).astype(np.float64))


def bridge_logg(xi, m, L):
    """log g(xi) = -|L^-1 (xi - m)|^2 / 2 - sum_k log L_kk - (D / 2) log 2 pi, by forward substitution"""
    xi, m, L = np.asarray(xi, dtype=np.float64), np.asarray(m, dtype=np.float64), np.asarray(L, dtype=np.float64)
    n, D = xi.shape
    y = np.zeros((n, D))
    for k in range(D):
        t = xi[:, k] - m[k]
        for c in range(k):
            t = t - L[k, c] * y[:, c]
        y[:, k] = t / L[k, k]
    return -0.5 * (y * y).sum(axis=1) - (np.log(np.diag(L)).sum() + 0.5 * D * math.log(2.0 * math.pi))


def philox4x32_10(ctr, key):
    """Philox4x32-10 over numpy arrays: ctr = four arrays of 32-bit words, key = two words (csrc/demc_philox.hpp) -> four uint64 arrays"""
    M32 = np.uint64(0xFFFFFFFF)
    c = [np.asarray(w, dtype=np.uint64) & M32 for w in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def bridge_normals(n, D, seed):
    """z[n][D]: draw j takes Philox block k at (key = seed, stream 7, sweep 0, iteration 0, entity j, block k); u1 = u53(x, y),
    u2 = u53(z, w); z_2k = sqrt(-2 log(1 - u1)) cos(2 pi u2), z_2k+1 = ... sin(2 pi u2)"""
    nb = (D + 1) // 2
    ent, blk = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(nb, dtype=np.uint64), indexing="ij")
    zero = np.zeros_like(ent)
    c = philox4x32_10([blk, ent, zero, zero + np.uint64(BRIDGE_STREAM << 24)], (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u53 = lambda lo, hi: (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53  # noqa: E731
    u1, u2 = u53(c[0], c[1]), u53(c[2], c[3])
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    z = np.empty((n, 2 * nb))
    z[:, 0::2] = rad * np.cos(2.0 * math.pi * u2)
    z[:, 1::2] = rad * np.sin(2.0 * math.pi * u2)
    return z[:, :D]


def bridge_draws(m, L, n, seed, lo=None, hi=None):
    """the n proposal draws of DESIGN.md 5.10 -> (theta[n][D], logJ[n], log g[n]): xi = m + L z with bridge_normals' z, the inverse
    transform, and log g = -|z|^2 / 2 - sum_k log L_kk - (D / 2) log 2 pi"""
    m, L = np.asarray(m, dtype=np.float64), np.asarray(L, dtype=np.float64)
    D = m.size
    z = bridge_normals(n, D, seed)
    xi = m[None, :] + z @ np.tril(L).T
    theta, lj = bridge_inverse(xi, lo, hi)
    return theta, lj, -0.5 * (z * z).sum(axis=1) - (np.log(np.diag(L)).sum() + 0.5 * D * math.log(2.0 * math.pi))


def bridge_from_logs(l1, l2, n_fit=float("nan"), lp2=None, trace=None):
    """DESIGN.md 5.10 from the two log-ratio vectors: l1[N1] over the estimate half, l2[N2] over the proposal draws -> Bridge.  The sums
    run in np.longdouble and are rounded to float64; r, the terms and the test of convergence are float64 as on the device.  lp2 (the
    log posterior of the proposal draws) only feeds the count n_zero_prop; without it the -Inf among l2 are counted.  An iterate that
    is not a positive finite number stops the iteration (counted, not converged, NaN outputs).  trace: a list that receives
    (r_{t+1}, |r_{t+1} - r_t| / |r_{t+1}|) of every iteration (NaN for the change of an iterate that stops it)."""
    l1, l2 = np.asarray(l1, dtype=np.float64).ravel(), np.asarray(l2, dtype=np.float64).ravel()
    N1, N2 = l1.size, l2.size
    nan, inf = float("nan"), float("inf")
    s1, s2 = N1 / (N1 + N2), N2 / (N1 + N2)
    n_zero = int(np.isneginf(l2 if lp2 is None else np.asarray(lp2)).sum())
    n_bad = int((np.isnan(l1) | np.isposinf(l1)).sum() + (np.isnan(l2) | np.isposinf(l2)).sum())
    ok1 = l1[~np.isnan(l1)]
    l_star = float(ok1.max()) if ok1.size else nan
    if n_bad or not math.isfinite(l_star):
        return Bridge([nan, nan, nan, 0, 0, n_fit, N1, N2, l_star, n_zero, n_bad, nan])
    mean = lambda v: float(v.astype(np.longdouble).sum() / v.size)  # noqa: E731
    with np.errstate(all="ignore"):
        e1, e2 = np.exp(l1 - l_star), np.exp(l_star - l2)
        big = np.isposinf(e2)
        f1_of = lambda r: np.where(big, 0.0, 1.0 / (s1 + (s2 * r) * np.where(big, 1.0, e2)))  # noqa: E731
        r, n_iter, conv, rel = 1.0, 0, 0, 0.0
        while n_iter < BRIDGE_MAX_ITER:
            rn = mean(f1_of(r)) / mean(1.0 / (s1 * e1 + s2 * r))
            n_iter += 1
            if not (math.isfinite(rn) and rn > 0.0):  # 0 by underflow, +Inf, NaN: the iteration stops, counted and not converged
                if trace is not None:
                    trace.append((rn, nan))
                return Bridge([nan, nan, nan, n_iter, 0, n_fit, N1, N2, l_star, n_zero, n_bad, nan])
            change = abs(rn - r)
            rel = change / abs(rn)
            r = rn
            if trace is not None:
                trace.append((rn, rel))
            if change <= BRIDGE_TOL * abs(rn):
                conv = 1
                break
        f1, f2 = f1_of(r), 1.0 / ((s1 * e1) / r + s2)
        m1, m2 = mean(f1), mean(f2)
        ss = lambda f, m: float(((f - m) ** 2).astype(np.longdouble).sum())  # noqa: E731
        # (np.float64 divides as the device does: a mean whose square underflows gives Inf or NaN, not an exception)
        re1 = float(np.float64(ss(f1, m1)) / (N2 - 1) / np.float64(m1 * m1) / N2) if N2 > 1 else nan
        re2 = float(np.float64(ss(f2, m2)) / (N1 - 1) / np.float64(m2 * m2) / N1) if N1 > 1 else nan
        return Bridge([math.log(r) + l_star if r > 0 else nan, re1, re2, n_iter, conv, n_fit, N1, N2, l_star, n_zero, n_bad, rel])


def compare_bridge(a, b, prior_odds=1.0):
    """two Bridge records of two models fitted to the SAME data -> dict(log_bf = logml_a - logml_b, se = sqrt(se_a^2 + se_b^2) with each
    record's own rho, prob_a and prob_b = the posterior model probabilities under prior_odds = p(a) / p(b)): positive log_bf favours a"""
    log_bf = a.logml - b.logml
    t = log_bf + math.log(prior_odds)
    pa = 1.0 / (1.0 + math.exp(-t)) if t >= 0 else math.exp(t) / (1.0 + math.exp(t))
    return dict(log_bf=log_bf, se=math.sqrt(a.se(a.rho) ** 2 + b.se(b.rho) ** 2), prob_a=pa, prob_b=1.0 - pa)
