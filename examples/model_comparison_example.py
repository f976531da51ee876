#!/usr/bin/env python3
"""Model comparison on the device: the data of test/lognormal_race_tests.jl fitted twice -- with the σ the data were simulated under and
with one twice as wide -- and the two fits compared by WAIC and by PSIS-LOO.  summarize(..., waic="pointwise", loo="pointwise") is
sample() followed by demc_waic and demc_loo over the kept rows: the log-density of every trial under every kept draw is formed
where the history lives, reduced there to lppd_i, p_waic_i and elpd_i per trial and to elpd_loo_i with its Pareto
khat_i, and only those tables come back.  compare_waic() and compare_loo() read the two tables; the khat counts say
whether the importance weights behind elpd_loo can be trusted where WAIC's p_waic_i > 0.4 flag says WAIC cannot."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import demc_amd as D  # noqa: E402

rng = np.random.default_rng(65)
N, nu_true, sigma_true, tau_true = 200, np.array([-1.0, -0.5, 0.0]), 1.0, 0.3
t = np.exp(nu_true[None, :] + sigma_true * rng.normal(0, 1, (N, 3)))  # the first accumulator to finish wins
choice, rt = np.argmin(t, axis=1) + 1.0, t.min(axis=1) + tau_true
min_rt = rt.min()


def sample_prior():
    return D.as_union([rng.normal(0, 3, 3), rng.uniform(0, min_rt)])


def fit(sigma):
    model = D.DEModel(sample_prior=sample_prior, names=("ν", "τ"), data=(choice, rt),
                      prior_loglike=D.Priors(ν=D.Normal(0, 3), τ=D.Uniform(0, min_rt)), loglike=D.LNRLikelihood(sigma=sigma))
    de = D.DE(sample_prior=sample_prior, bounds=((-np.inf, np.inf), (0.0, min_rt)), burnin=1000, Np=8)
    return D.summarize(model, de, D.HIPBackend(seed=3), 2000, waic="pointwise", loo="pointwise")


fits = {sigma: fit(sigma) for sigma in (1.0, 2.0)}
for sigma, s in fits.items():
    print(f"σ = {sigma}: {s.waic}")
    print(f"         {s.loo}")
    print(f"         khat > 0.7: {int(s.loo.n_k_high)} of {N} trials, khat > 1: {int(s.loo.n_k_bad)}; p_waic > 0.4: {int(s.waic.n_high)}")
    print("         " + "  ".join(f"{name} {v['mean']:.3f}" for name, v in s.describe().items()))
cmp = D.compare_waic(fits[1.0].waic, fits[2.0].waic)
print(f"elpd(σ = 1) - elpd(σ = 2) = {cmp['elpd_diff']:.2f} (se {cmp['se_diff']:.2f}): "
      f"{'the σ the data were simulated under predicts better' if cmp['elpd_diff'] > 0 else 'the wider σ predicts better'}")
cmp = D.compare_loo(fits[1.0].loo, fits[2.0].loo)
print(f"elpd_loo(σ = 1) - elpd_loo(σ = 2) = {cmp['elpd_diff']:.2f} (se {cmp['se_diff']:.2f})")
