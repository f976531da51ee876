#!/usr/bin/env python3
"""Examples/Predator_Prey_Example.jl on the MI355X path: the parameters of the Lotka-Volterra equations fitted to noisy
trajectories.  The reference's settings -- Np = 12, n_groups = 3, burnin = 1000, 3000 iterations, truth (1.5, 1.0, 3.0, 1.0), noise
0.5, observations every 0.1 on (0, 10) -- with two deviations: the library integrates with classical RK4 at a fixed step
(LotkaVolterraLikelihood(substeps=10): 3e-7 from the converged trajectory) instead of the adaptive Tsit5(), and
sigma's prior is LogNormal(0.4, 0.8) -- median 1.5, most of its mass on (0.3, 7) like the reference's InverseGamma(2, 3) (mode 1,
mean 3) -- because InverseGamma is not a registered prior kind: it needs a case of its own in the device's prior switch, which is a
change to every kernel that carries it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import demc_amd as D  # noqa: E402

TRUTH, U0, DT, T = (1.5, 1.0, 3.0, 1.0), (1.0, 1.0), 0.1, 101


def trajectory(p, substeps=640):
    """the data-generating solution at fine steps: classical RK4, 640 steps per observation interval"""
    al, be, ga, de = p
    f = lambda x, y: ((al - be * y) * x, (de * x - ga) * y)  # noqa: E731  Predator_Prey_Example.jl:6-11
    h = DT / substeps
    x, y = U0
    out = [(x, y)]
    for _ in range((T - 1) * substeps):
        k1 = f(x, y)
        k2 = f(x + 0.5 * h * k1[0], y + 0.5 * h * k1[1])
        k3 = f(x + 0.5 * h * k2[0], y + 0.5 * h * k2[1])
        k4 = f(x + h * k3[0], y + h * k3[1])
        x += h / 6.0 * (k1[0] + 2.0 * k2[0] + 2.0 * k3[0] + k4[0])
        y += h / 6.0 * (k1[1] + 2.0 * k2[1] + 2.0 * k3[1] + k4[1])
        out.append((x, y))
    return np.array(out[::substeps]).T   # 2 x T, the reference's layout


rng = np.random.default_rng(42)
data = trajectory(TRUTH) + 0.5 * rng.normal(size=(2, T))                       # Predator_Prey_Example.jl:21-22
bounds = ((0.5, 2.5), (0.0, 2.0), (1.0, 4.0), (0.0, 2.0), (0.0, np.inf))       # :45-51
priors = dict(α=D.TruncatedNormal(1.5, 0.5), β=D.TruncatedNormal(1.2, 0.5), γ=D.TruncatedNormal(3.0, 0.5),
              δ=D.TruncatedNormal(1.0, 0.5), σ=D.LogNormal(0.4, 0.8))           # :26-34 (σ: see above)


def sample_prior():                                                             # :36-43
    def truncated(p, lo, hi):
        while True:
            v = rng.normal(p.a, p.b)
            if lo <= v <= hi:
                return v
    return [truncated(priors[n], *b) for n, b in zip("αβγδ", bounds)] + [float(rng.lognormal(0.4, 0.8))]


model = D.DEModel(sample_prior=sample_prior, names=("α", "β", "γ", "δ", "σ"), data=data, prior_loglike=D.Priors(**priors),
                  loglike=D.LotkaVolterraLikelihood(u0=U0, dt=DT, substeps=10))
de = D.DE(sample_prior=sample_prior, bounds=bounds, burnin=1000, Np=12, n_groups=3)
chains = D.sample(model, de, D.HIPBackend(seed=2026), 3000)
print(f"{'':4s} {'mean':>8s} {'std':>8s} {'rhat':>7s} {'truth':>6s}")
for name, truth in zip(("α", "β", "γ", "δ", "σ"), TRUTH + (0.5,)):
    d = chains.describe()[name]
    print(f"{name:4s} {d['mean']:8.3f} {d['std']:8.3f} {d['rhat']:7.3f} {truth:6.2f}")
