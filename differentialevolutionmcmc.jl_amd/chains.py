"""Minimal stand-in for MCMCChains.Chains: value array (iterations x parameters x chains) + names, and the
summary statistics the reference's tests read from describe(chains)[1] (:mean, :std, :rhat), plus the effective sample size,
its Monte-Carlo standard error and the autocorrelation MCMCChains adds to them (DESIGN.md section 5.5 is the definition; the device
computes the same numbers from the history without exporting it: demc_summarize)."""
import numpy as np

SUMMARY_COLS = ("mean", "std", "rhat", "ess", "mcse", "pairs")  # the columns of demc_summarize's out (DEMC_SUMMARY_COLS)


class Summary:
    """The summary table of a run: `values[j]` = (mean, std, rhat, ess, mcse, pairs) of series names[j] -- the parameters,
    then acceptance and lp.  `rho` (or None): [series][lags] autocorrelations, NaN beyond the lags that were evaluated."""

    def __init__(self, names, values, internals=("acceptance", "lp"), rho=None):
        self.names = list(names)
        self.values = np.asarray(values, dtype=np.float64).reshape(len(self.names), len(SUMMARY_COLS))
        self.internals = list(internals)
        self.rho = rho

    def __getitem__(self, name):
        return dict(zip(SUMMARY_COLS, (float(v) for v in self.values[self.names.index(name)])))

    def describe(self):
        """per parameter name the dict Chains.describe() gives (mean, std, rhat), extended by ess, mcse and pairs"""
        return {nm: self[nm] for nm in self.names if nm not in self.internals}


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

    def summarystats(self, max_lag=0, rho_len=0):
        """The Summary of this object computed on the host (numpy): what demc_summarize computes on the device for a history that
        was never exported.  max_lag > 0 caps the lags of Geyer's sequence; rho_len > 0 also keeps that many autocorrelations."""
        rows, rhos = [], []
        for j in range(len(self.names)):
            vals, rho = series_summary(self.value[:, j, :], max_lag, rho_len)
            rows.append(vals)
            rhos.append(rho)
        return Summary(self.names, rows, self.internals, np.stack(rhos) if rho_len > 0 else None)
