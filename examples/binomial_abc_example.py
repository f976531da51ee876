#!/usr/bin/env python3
"""Examples/Binomial_ABC.jl on the MI355X path: approximate Bayesian computation for a Binomial rate -- every proposal simulates
10 000 Binomial(N, theta) counts and its log-likelihood is the log of the share that equals the observed count; theta ~ Beta(1,1)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import demc_amd as D  # noqa: E402

rng = np.random.default_rng(88484)
N = 10
data = dict(N=N, k=int(rng.binomial(N, 0.5)))


def sample_prior():
    return [rng.beta(1, 1)]


model = D.DEModel(sample_prior=sample_prior, names=("θ",), data=data,
                  prior_loglike=D.Priors(θ=D.Beta(1, 1)),                                                   # Binomial_ABC.jl:6
                  loglike=D.SimulatedLikelihood(D.SimBinomial(N), estimator="frequency", n_sim=10_000))     # Binomial_ABC.jl:15-22
de = D.DE(sample_prior=sample_prior, bounds=((0.0, 1.0),), burnin=1000, Np=3, σ=0.01)
chains = D.sample(model, de, D.MCMCThreads(), 2000, progress=True)
for name, s in chains.describe().items():
    print(f"{name}: mean {s['mean']:.3f}  std {s['std']:.3f}  rhat {s['rhat']:.3f}")
print(f"observed k = {data['k']} of N = {N}; Beta(1,1) prior: exact posterior mean {(data['k'] + 1) / (N + 2):.3f}")
