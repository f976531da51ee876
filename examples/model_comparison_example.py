#!/usr/bin/env python3
"""Model comparison on the device: the data of test/lognormal_race_tests.jl fitted twice -- with the σ the data were simulated under and
with one twice as wide -- and the two fits compared by WAIC and by PSIS-LOO.  summarize(..., waic="pointwise", loo="pointwise") is
sample() followed by demc_waic and demc_loo over the kept rows: the log-density of every trial under every kept draw is formed
where the history lives, reduced there to lppd_i, p_waic_i and elpd_i per trial and to elpd_loo_i with its Pareto
khat_i, and only those tables come back.  compare_waic() and compare_loo() read the two tables; the khat counts say
whether the importance weights behind elpd_loo can be trusted where WAIC's p_waic_i > 0.4 flag says WAIC cannot.  The last part forms
a Bayes factor between two priors on the same Binomial data by bridge sampling on the device (summarize(..., bridge=True), demc_bridge)."""
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

# A Bayes factor, where the question is which model the data support, not which predicts better: the same Binomial data under two
# priors, the log marginal likelihood of each fit formed on the device by bridge sampling over the kept rows (summarize(..., bridge=True),
# demc_bridge).  Both have closed forms, printed beside the estimates.
import math  # noqa: E402

n_trials, k = np.array([12.0, 9.0, 15.0, 11.0, 8.0]), np.array([9.0, 7.0, 12.0, 8.0, 7.0])


def fit_binomial(a, b):
    sp = lambda: [rng.uniform(0.05, 0.95)]  # noqa: E731
    model = D.DEModel(sample_prior=sp, names=("θ",), data=dict(N=n_trials, k=k), prior_loglike=D.Priors(θ=D.Beta(a, b)), loglike=D.BinomialLikelihood())
    de = D.DE(sample_prior=sp, bounds=((0.0, 1.0),), burnin=500, Np=8)
    return D.summarize(model, de, D.HIPBackend(seed=4), 2500, bridge=dict(n_prop=20000, seed=1))


def exact(a, b):
    lbeta = lambda p, q: math.lgamma(p) + math.lgamma(q) - math.lgamma(p + q)  # noqa: E731
    return (sum(math.lgamma(x + 1) - math.lgamma(y + 1) - math.lgamma(x - y + 1) for x, y in zip(n_trials, k))
            + lbeta(a + k.sum(), b + (n_trials - k).sum()) - lbeta(a, b))


priors = {"Beta(1, 1)": (1.0, 1.0), "Beta(2, 8)": (2.0, 8.0)}
bridges = {name: fit_binomial(*ab).bridge for name, ab in priors.items()}
for name, br in bridges.items():
    print(f"θ ~ {name}: {br}; exact {exact(*priors[name]):.4f}; autocorrelation factor {br.rho:.1f}")
bf = D.compare_bridge(bridges["Beta(1, 1)"], bridges["Beta(2, 8)"])
print(f"log Bayes factor Beta(1, 1) : Beta(2, 8) = {bf['log_bf']:.3f} (se {bf['se']:.3f}; exact {exact(1.0, 1.0) - exact(2.0, 8.0):.3f}), "
      f"posterior probability of the flat prior {bf['prob_a']:.3f} at even prior odds")
