#!/usr/bin/env python3
"""test/lognormal_race_tests.jl twice on the MI355X path: once with the closed-form likelihood of the log-normal race
(LNRLikelihood) and once likelihood-free -- every proposal simulates 10 000 (choice, response time) pairs from the race and scores
the data under the per-choice defective Epanechnikov density of them (probability density approximation, Turner & Sederberg 2014);
nu ~ N(0, 3), tau ~ U(0, min rt).  Prints both posteriors side by side."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import demc_amd as D  # noqa: E402

data_rng = np.random.default_rng(9918)
nu, tau, N = np.array([-2.0, -2.0, -3.0, -3.0]), 0.5, 100          # lognormal_race_tests.jl:6-7
t = np.exp(data_rng.normal(nu, 1.0, (N, 4)))
choice, rt = t.argmin(1) + 1.0, t.min(1) + tau
min_rt = float(rt.min())


def run(loglike, n_iter=3000):
    rng = np.random.default_rng(68541)

    def sample_prior():
        return [rng.normal(0, 3, 4), rng.uniform(0, min_rt)]

    model = D.DEModel(sample_prior=sample_prior, names=("ν", "τ"), data=(choice, rt), loglike=loglike,
                      prior_loglike=D.Priors(ν=D.Normal(0, 3), τ=D.Uniform(0.0, min_rt)))    # lognormal_race_tests.jl:14-18
    de = D.DE(sample_prior=sample_prior, bounds=((-np.inf, np.inf), (0.0, min_rt)), burnin=1000, Np=24, n_groups=4)
    return D.sample(model, de, D.HIPBackend(seed=2024), n_iter).describe()


exact = run(D.LNRLikelihood(sigma=1.0))
pda = run(D.SimulatedLikelihood(D.SimLNR(sigma=1.0), estimator="kde_choice", n_sim=10_000))
print(f"{'':8s} {'closed form':>24s}   {'simulated (kde_choice)':>24s}")
for name in exact:
    a, b = exact[name], pda[name]
    print(f"{name:8s} mean {a['mean']:7.3f}  std {a['std']:6.3f}   mean {b['mean']:7.3f}  std {b['std']:6.3f}   rhat {b['rhat']:.3f}")
