#!/usr/bin/env python3
"""The Gaussian example's run summarised on the device: summarize() is sample() followed by the summary table -- mean, std, split-R-hat,
effective sample size, Monte-Carlo standard error -- computed from the history where it lives (demc_summarize), so that no chain is
exported.  The host form of the same table is chains.summarystats().  With quantiles=... the same run also selects the quantile table
of describe(chains) on the device (demc_quantiles, chains pooled); its host form is chains.quantile().  With cor=True it also forms
the posterior covariance and correlation of the parameters there (demc_covariance); the host form is chains.cor().  With rank=True it
also ranks the pooled history of every series there and reports MCMCChains' ess_bulk, ess_tail and rank-normalised rhat
(demc_rankstats); the host form is chains.rankstats().  With hpd=0.05 it also reads the 95 % highest-density interval of every series
off the same sorted pool (demc_hpd); the host form is chains.hpd()."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import demc_amd as D  # noqa: E402

rng = np.random.default_rng(50514)
data = rng.normal(0.0, 1.0, 50)


def sample_prior():
    return [rng.normal(0, 1), abs(rng.standard_cauchy())]


model = D.DEModel(sample_prior=sample_prior, names=("μ", "σ"), data=data,
                  prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)), loglike=D.GaussianLikelihood())
de = D.DE(sample_prior=sample_prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=1000, Np=6)
summary = D.summarize(model, de, D.HIPBackend(seed=1), 2000, quantiles=D.chains.DEFAULT_QUANTILES, cor=True, rank=True, hpd=0.05)
for name, s in summary.describe().items():
    print(f"{name}: mean {s['mean']:.3f}  std {s['std']:.3f}  rhat {s['rhat']:.3f}  ess {s['ess']:.0f}  mcse {s['mcse']:.4f}  "
          f"({s['pairs']:.0f} pairs of lags)")
print(f"acceptance rate {summary['acceptance']['mean']:.3f}")
for name, r in summary.rank.describe().items():
    print(f"{name}: rank-normalised rhat {r['rhat']:.3f}  ess_bulk {r['ess_bulk']:.0f}  ess_tail {r['ess_tail']:.0f}")
print(f"lp: rank-normalised rhat {summary.rank['lp']['rhat']:.3f}  ess_bulk {summary.rank['lp']['ess_bulk']:.0f}  ess_tail {summary.rank['lp']['ess_tail']:.0f}")
print("quantiles  " + "  ".join(f"{100 * q:5.1f}%" for q in summary.probs))
hpd = summary.hpd.describe()
for name, row in summary.quantile().items():
    print(f"{name}:         " + "  ".join(f"{v:6.3f}" for v in row.values()) + f"   95% HPD [{hpd[name]['lower']:6.3f}, {hpd[name]['upper']:6.3f}]")
names, cor = summary.cor()
print("cor        " + "  ".join(f"{nm:>6}" for nm in names))
for nm, row in zip(names, cor):
    print(f"{nm}:         " + "  ".join(f"{v:6.3f}" for v in row))
