"""MI355X-native DE-MCMC hot path behind the API of itsdfish/DifferentialEvolutionMCMC.jl.

Exports follow src/DifferentialEvolutionMCMC.jl:15-18.  Compute happens only in libdemc_hip.so (hand-written
gfx950 kernels behind the C-ABI of include/demc.h); importing this package without the built library works, but
any sampling call raises -- there is no CPU fallback.
"""
from . import _ffi, families
from ._ffi import DemcError, HipEngine, MultiEngine
from .chains import (Bridge, Chains, Hpd, Loo, RankStats, Summary, Waic, bridge_draws, bridge_fit, bridge_from_logs, bridge_transform, compare_bridge, compare_loo,
                     compare_waic, loo_from_loglik, waic_from_loglik)
from .families import (Beta, BinomialLikelihood, Cauchy, Exponential, Flat, Gamma, GaussianLikelihood, LogNormal, HierBinomialLikelihood,
                       HierGaussianLikelihood, LBALikelihood, LNRLikelihood, LotkaVolterraLikelihood, MvNormalFullLikelihood,
                       MvNormalIsoLikelihood, Normal, Priors, RastriginObjective, SimBinomial, SimLNR, SimNormal, SimSource,
                       SimulatedLikelihood, SourceLikelihood, TruncatedCauchy, TruncatedNormal, Uniform)
from .sampler import get_optimal, optimize, sample, summarize
from .structs import (DE, DEModel, HIPBackend, MCMCThreads, Particle, as_union, compute_posterior, evaluate_fun,
                      fixed_gamma, maximize, mh_update, minimize, project, random_gamma, resample, sample_current,
                      variable_gamma)

DEMCMC = __name__

__all__ = ["DE", "Particle", "DEModel", "sample", "MCMCThreads", "HIPBackend", "fixed_gamma", "variable_gamma",
           "random_gamma", "evaluate_fun", "compute_posterior", "optimize", "get_optimal", "resample", "as_union",
           "mh_update", "maximize", "minimize", "Chains", "Summary", "RankStats", "Hpd", "Waic", "compare_waic", "waic_from_loglik", "Loo", "compare_loo", "loo_from_loglik", "Bridge", "compare_bridge", "bridge_from_logs", "bridge_transform", "bridge_fit", "bridge_draws", "summarize", "Priors", "HipEngine", "MultiEngine", "DemcError"]
