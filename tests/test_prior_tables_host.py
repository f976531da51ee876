"""The prior tables that tests/test_gpu_prior_kernels.py feeds to the update kernels, and the evidence -- from the CPU oracle
alone, no GPU -- that each of them is a test: a case whose prior decided nothing, or whose run accepted nothing, would pass
against any kernel.

CASES is the one list both modules read.  A case is a workload (workloads.py's dict: model, per-scalar prior table, bounds,
starting rows), a population, the sampler's settings, the kernel instance the engine must report and -- `under_test` -- the
prior kinds the case is about.  Kinds are families.py's: Gamma(shape, scale), Exponential(scale), LogNormal(mu, sigma),
Cauchy(loc, scale), TruncatedCauchy(loc, scale) [half-Cauchy], Beta(a, b), Uniform(a, b), Flat, TruncatedNormal(mu, sd).

For every case the oracle is run as tests/test_gpu_production.py::free_run runs it (same seeds, same starting rows) and

  * run again with the kinds under test replaced by Flat: the accept history must differ (the prior decided something);
  * its acceptance rate must be above free_run's own floor of 0.02;
  * where a bound is said to bite (`bites`), opening that bound must change the accept history;
  * the two cases whose prior support is narrower than the bounds must START partly outside it: at least one and at most half
    of the starting rows at -Inf, no group entirely at -Inf (that edge has its own test, test_gpu_edge_cases.py).

The oracle knows no truncated Normal: it is given Normal(a, b) with the same bounds (the two differ by a constant, which no
decision sees); the GPU module adds that constant to the oracle's log-posteriors."""
import numpy as np
import pytest

from demc_amd import families as F
from demc_amd import workloads as W

INF = np.inf
PLAIN = (F.PRIOR_FLAT, F.PRIOR_NORMAL, F.PRIOR_NORMAL_REF)
Z = dict(schedule=1, partner_kind=1)  # DE-MC_Z: partners from the history, the synchronous schedule


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
def table(segs, ref=1):
    """[(n scalars, prior, lo, hi), ...] -> the per-scalar arrays of a workload; Normal(a, "name") reads scalar `ref`"""
    t = dict(pk=[], pa=[], pb=[], pref=[], lo=[], hi=[])
    for n, pr, lo, hi in segs:
        t["pk"] += [pr.kind] * n
        t["pa"] += [pr.a] * n
        t["pb"] += [pr.b] * n
        t["pref"] += [ref if pr.kind == F.PRIOR_NORMAL_REF else 0] * n
        t["lo"] += [lo] * n
        t["hi"] += [hi] * n
    return t


def with_table(w, segs, **more):
    t = table(segs)
    assert len(t["pk"]) == w["D"], (len(t["pk"]), w["D"])
    return dict(w, **t, **more)


def for_oracle(w):
    """the workload as the oracle is given it: TruncatedNormal(a, b) as Normal(a, b), bounds unchanged"""
    return dict(w, pk=[F.PRIOR_NORMAL if k == F.PRIOR_TRUNCNORMAL else k for k in w["pk"]])


def truncnormal_log_mass(w):
    """sum over the TruncatedNormal scalars of log(mass of Normal(a, b) between the scalar's bounds): what the library takes off
    the log-posterior of every in-bounds row and the oracle's Normal does not"""
    return sum(F.TruncatedNormal(a, b).log_mass(lo, hi)
               for k, a, b, lo, hi in zip(w["pk"], w["pa"], w["pb"], w["lo"], w["hi"]) if k == F.PRIOR_TRUNCNORMAL)


def flattened(w, kinds):
    return dict(w, pk=[F.PRIOR_FLAT if k in kinds else k for k in w["pk"]])


def opened(w, scalars):
    lo, hi = list(w["lo"]), list(w["hi"])
    for j in scalars:
        lo[j], hi[j] = -INF, INF
    return dict(w, lo=lo, hi=hi)


# ---------------------------------------------------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------------------------------------------------
def mvn_small(d, centre=0.5, spread=0.15):
    """MvNormal-full with 24 observations whose mean is `centre` in every dimension; starting rows centre + spread z: near
    the posterior (sd ~ 0.2), so that a prior with scale 0.05 .. 0.3 around there has a say in the decisions"""
    w = W.mvn_full(d, 24, seed=1)
    X = w["data"] - w["data"].mean(0) + centre
    return dict(w, data=np.ascontiguousarray(X), init=lambda P, rng: centre + spread * rng.normal(0, 1, (P, d)))


def cfg2_shifted(centre):
    """BASELINE cfg2's data (D = 8) with 1030 observations -- a last chunk of one ragged tile for the streaming forms -- moved so
    that the mean is `centre` in every dimension (None: as generated), starting rows around it"""
    w = W.cfg2(N=1030)
    if centre is None:
        return w
    X = w["data"] - w["data"].mean(0) + centre
    return dict(w, data=np.ascontiguousarray(X), init=lambda P, rng: centre + 0.5 * rng.normal(0, 1, (P, 8)))


def mvn_iso(d, centre=None, seed=41):
    """MvNormal(mu, sigma^2 I), sigma the last scalar: conftest.make_problem's model, the means optionally at `centre`"""
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 1, (100, d)) + (rng.normal(0, 1, d) if centre is None else centre)
    m = X.mean(0)
    return dict(fam=F.FAM_MVN_ISO, data=X, dims=[100, d], hyper=None, D=d + 1, masks=None, engine={},
                init=lambda P, rng_: np.concatenate([m + 0.3 * rng_.normal(0, 1, (P, d)), rng_.uniform(0.6, 1.8, (P, 1))], 1))


def gaussian50():
    rng = np.random.default_rng(311)
    data = rng.normal(0.3, 1.2, 50)
    return dict(fam=F.FAM_GAUSSIAN, data=data, dims=[50], hyper=None, D=2, masks=None, engine={},
                init=lambda P, rng_: np.stack([rng_.normal(0, 1, P), rng_.uniform(0.4, 2.5, P)], 1))


def binomial5():
    rng = np.random.default_rng(311)
    n = rng.integers(5, 20, 5).astype(float)
    k = np.floor(n * rng.uniform(0.2, 0.8, 5))
    return dict(fam=F.FAM_BINOMIAL, data=np.concatenate([n, k]), dims=[5], hyper=None, D=1, masks=None, engine={},
                init=lambda P, rng_: rng_.uniform(0.05, 0.95, (P, 1)))


def lnr(N, na):
    rng = np.random.default_rng(311)
    choice = rng.integers(1, na + 1, N).astype(float)
    rt = rng.uniform(0.45, 1.6, N)
    mr = float(rt.min())
    return dict(fam=F.FAM_LNR, data=np.concatenate([choice, rt]), dims=[N, na], hyper=[1.0], D=na + 1, masks=None, engine={}, min_rt=mr,
                init=lambda P, rng_: np.concatenate([rng_.normal(-1, 1, (P, na)), rng_.uniform(0.05, mr * 0.9, (P, 1))], 1))


def hier_binomial(S, seed, blocks=None):
    """conftest.make_problem's hierarchical Binomial (theta = mu_b0, sd_b0, b0[S]) with blocks [hyper ; subjects] in the given order"""
    rng = np.random.default_rng(seed)
    b0 = rng.normal(0, 1, S)
    k = rng.binomial(50, 1 / (1 + np.exp(-(1.0 + b0)))).astype(float)
    D = S + 2
    m0 = np.zeros(D, np.uint8)
    m0[:2] = 1
    masks = {None: None, "hyper_first": np.stack([m0, 1 - m0]), "subjects_first": np.stack([1 - m0, m0])}[blocks]
    # (starting rows around the generating parameters: from prior draws a run this short only climbs -- every improvement accepted,
    # everything else rejected by hundreds of log units -- and no prior term has a say in a decision)
    return dict(fam=F.FAM_HIER_BINOMIAL, data=k, dims=[S], hyper=[50.0], D=D, masks=masks, engine={},
                init=lambda P, rng_: np.concatenate([rng_.normal(1, 0.1, (P, 1)), rng_.uniform(0.7, 1.4, (P, 1)), b0 + 0.3 * rng_.normal(0, 1, (P, S))], 1))


# ---------------------------------------------------------------------------------------------------------------------
# priors under test
# ---------------------------------------------------------------------------------------------------------------------
ONE_SEGMENT = {  # name -> (prior, lo, hi) for every scalar of an MvNormal-full row around 0.5
    "gamma": (F.Gamma(2.5, 0.2), -INF, INF),
    "exponential": (F.Exponential(0.1), -INF, INF),
    "lognormal": (F.LogNormal(-1.0, 0.3), -INF, INF),
    "cauchy": (F.Cauchy(0.0, 0.05), -INF, INF),
    "beta": (F.Beta(2.0, 5.0), -INF, INF),
    "halfcauchy": (F.TruncatedCauchy(0.0, 0.05), -INF, INF),
    "uniform": (F.Uniform(0.2, 0.8), -INF, INF),
    "flat": (F.Flat(), -INF, INF),
    "truncnormal": (F.TruncatedNormal(0.4, 0.2), 0.1, 0.9),
}
SIGMA = {  # priors of a scale parameter near 1
    "gamma": F.Gamma(2.0, 0.5), "exponential": F.Exponential(1.0), "lognormal": F.LogNormal(0.0, 0.5),
}


def one_segment(w, name):
    pr, lo, hi = ONE_SEGMENT[name]
    return with_table(w, [(w["D"], pr, lo, hi)])


# segments that straddle the lanes' four-scalar blocks; the bounds differ per segment, the Flat scalar's bite (`bites`)
MIXED12 = [(3, F.Normal(0.0, 1.0), -5.0, 5.0), (2, F.Gamma(2.5, 0.2), 0.02, 2.0), (1, F.Flat(), 0.3, 0.7),
           (3, F.LogNormal(-1.0, 0.3), 0.0, 3.0), (3, F.Cauchy(0.0, 0.05), -1.0, 4.0)]
MIXED7 = [(1, F.Beta(2.0, 5.0), 0.0, 1.0), (2, F.Normal(0.0, 1.0), -INF, INF), (3, F.Exponential(0.1), 0.0, 6.0),
          (1, F.Uniform(0.1, 0.9), 0.35, 0.65)]
# MvNormal-iso, d = 5: two tables that together hold every registered kind next to Normal and Flat (k_propose's own look-up)
ISO5_A = [(2, F.Cauchy(0.0, 1.0), -INF, INF), (1, F.Flat(), -INF, INF), (2, F.Normal(0.0, 1.0), -INF, INF), (1, F.Gamma(2.0, 0.5), 0.0, INF)]
ISO5_B = [(1, F.TruncatedCauchy(0.0, 0.5), -INF, INF), (1, F.Uniform(0.25, 0.75), -INF, INF), (1, F.Beta(2.0, 5.0), -INF, INF),
          (1, F.Exponential(0.5), -INF, INF), (1, F.TruncatedNormal(0.4, 0.5), -1.0, 2.0), (1, F.LogNormal(0.0, 0.5), 0.0, INF)]
# per-phase chain: every scalar's support narrower than its (open) bounds -- K3 has to carry K1's prior sum, -Inf included
CHAIN5 = [(2, F.Gamma(2.5, 0.2), -INF, INF), (1, F.Uniform(0.2, 0.8), -INF, INF), (1, F.TruncatedCauchy(0.0, 0.05), -INF, INF),
          (1, F.Beta(2.0, 5.0), -INF, INF)]


def hier_table(sd_prior, subjects):
    return [(1, F.Normal(1.0, 1.0), -INF, INF), (1, sd_prior, 0.0, INF)] + [(n, pr, -INF, INF) for n, pr in subjects]


def subjects_short():
    return [(15, F.Normal(0.0, "sd_b0")), (10, F.Cauchy(0.0, 1.0)), (10, F.Normal(0.0, 1.5)), (5, F.Flat())]


def subjects_long(S):  # every border inside a round of 256 scalars, a non-plain segment between plain ones
    return [(1000, F.Normal(0.0, "sd_b0")), (600, F.Cauchy(0.0, 1.0)), (500, F.Normal(0.0, 1.5)), (S - 2100, F.Flat())]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
CASES = []


def case(id, make, n_it, G, Np, kernel, theta_exact, under_test=None, support=False, bites=None, exact=True, lp_rtol=1e-9, **cfg):
    """kernel: what last_kernels() must report (exact=False: the substrings it must hold).  under_test: the kinds replaced by
    Flat for the `prior decides` check (None: every kind but Flat / Normal / Normal-ref; (): the check does not apply)."""
    CASES.append(dict(id=id, make=make, n_it=n_it, G=G, Np=Np, kernel=kernel, theta_exact=theta_exact, under_test=under_test,
                      support=support, bites=bites, exact=exact, lp_rtol=lp_rtol, cfg=cfg))


def _a(beta):
    return dict(n_it=12, G=4, Np=16, theta_exact=beta == 0.0, beta=beta, alpha=0.3, loglike_mode=1)


# (a) k_res_mvn, SUFFSTAT, two_colour
for _beta in (0.0, 0.1):
    for _name in ONE_SEGMENT:
        case(f"a-d8-{_name}-beta{_beta:g}", lambda n=_name: one_segment(mvn_small(8), n), kernel="k_res_mvn<256,false,8>",
             under_test=() if _name == "flat" else None, **_a(_beta))
    for _name in ("gamma", "beta", "truncnormal"):
        case(f"a-d32-{_name}-beta{_beta:g}", lambda n=_name: one_segment(mvn_small(32), n), kernel="k_res_mvn<256,false,32>", **_a(_beta))
    case(f"a-d12-mixed-beta{_beta:g}", lambda: with_table(mvn_small(12), MIXED12), kernel="k_res_mvn<256,false,0>", bites=[5], **_a(_beta))
    case(f"a-d7-mixed-beta{_beta:g}", lambda: with_table(mvn_small(7), MIXED7), kernel="k_res_mvn<256,false,0>", bites=[6], **_a(_beta))
case("a-d12-mixed-Np130", lambda: with_table(mvn_small(12), MIXED12), 12, 4, 130, "k_res_mvn<512,false,0>", False, bites=[5], beta=0.1,
     alpha=0.3, loglike_mode=1)
# support narrower than the (open) bounds: data and starts at 0.1, a fifth of the rows start with a scalar <= 0
case("a-d8-gamma-open-support", lambda: one_segment(mvn_small(8, centre=0.1, spread=0.05), "gamma"), 12, 4, 16, "k_res_mvn<256,false,8>",
     False, support=True, beta=0.1, alpha=0.3, loglike_mode=1)

# (b) k_res_mvn, the other forms
for _mode, _kern in ((0, "k_res_mvn<256,true,8>"), (2, "k_res_mvn<512,true,8,direct>")):
    _tag = "streaming" if _mode == 0 else "direct"
    case(f"b-{_tag}-cauchy", lambda: with_table(cfg2_shifted(None), [(8, F.Cauchy(0.0, 0.5), -INF, INF)]), 6, 32, 64, _kern, True,
         beta=0.0, alpha=0.3, loglike_mode=_mode)
    case(f"b-{_tag}-gamma", lambda: with_table(cfg2_shifted(3.0), [(8, F.Gamma(2.5, 0.2), -INF, INF)]), 6, 32, 64, _kern, False,
         beta=0.1, alpha=0.3, loglike_mode=_mode)
for _hist, _extra in ((2, dict(burnin=100)), (1, dict(burnin=0)), (3, dict(burnin=3, theta_snooker=0.1))):
    case(f"b-demcz-d8-gamma-hist{_hist}", lambda: one_segment(mvn_small(8), "gamma"), 6 + 10, 4, 16, f"k_res_mvn<256,false,8,{_hist}>",
         _hist != 3, beta=0.0, loglike_mode=1, n_initial=6, **Z, **_extra)
    case(f"b-demcz-d12-mixed-hist{_hist}", lambda: with_table(mvn_small(12), MIXED12), 6 + 10, 4, 16, f"k_res_mvn<256,false,0,{_hist}>",
         _hist != 3, bites=[5], beta=0.0, loglike_mode=1, n_initial=6, **Z, **_extra)
for (_name, _pr), (_hist, _extra) in zip(SIGMA.items(), ((1, dict(burnin=0)), (2, dict(burnin=100)), (3, dict(burnin=3, theta_snooker=0.1)))):
    case(f"b-iso5-sigma-{_name}-hist{_hist}", lambda pr=_pr: with_table(mvn_iso(5), [(5, F.Normal(0.0, 1.0), -INF, INF), (1, pr, 0.0, INF)]),
         6 + 10, 4, 16, f"k_res_mvn<256,false,0,{_hist},iso>", False, beta=0.1, loglike_mode=1, n_initial=6, **Z, **_extra)


def mvn30_table():
    w = W.mvn30(G=4, Np=16)
    w = dict(w, init=lambda P, rng: np.concatenate([rng.normal(0, 0.3, (P, 30)), rng.uniform(0.6, 1.8, (P, 1))], 1))
    return with_table(w, [(30, F.Cauchy(0.0, 1.0), -INF, INF), (1, F.LogNormal(0.0, 0.5), 0.0, INF)])


for _hist, _extra in ((3, dict(burnin=100, theta_snooker=0.1)), (1, dict(burnin=0))):
    case(f"b-mvn30-hist{_hist}", mvn30_table, 8 + 12, 4, 16, f"k_res_mvn<256,false,31,{_hist},iso>", _hist == 1, beta=0.0, loglike_mode=1,
         n_initial=8, **Z, **_extra)

# (c) k_res_obs<256>
_C = dict(n_it=24, kernel="k_res_obs<256>", alpha=0.3)
for _mu_name, _mu in (("cauchy", F.Cauchy(0.0, 1.0)), ("flat", F.Flat())):
    for _name, _pr, _lo, _hi in (("gamma", SIGMA["gamma"], 0.0, INF), ("exponential", SIGMA["exponential"], 0.0, INF),
                                 ("lognormal", SIGMA["lognormal"], 0.0, INF), ("truncnormal", F.TruncatedNormal(1.0, 0.5), 0.2, 3.0),
                                 ("halfcauchy", F.TruncatedCauchy(0.0, 0.5), 0.0, INF)):
        _beta = 0.0 if (_mu_name == "flat") == (_name in ("gamma", "lognormal")) else 0.1
        case(f"c-gaussian-mu-{_mu_name}-sigma-{_name}", lambda mu=_mu, pr=_pr, lo=_lo, hi=_hi: with_table(gaussian50(), [(1, mu, -INF, INF), (1, pr, lo, hi)]),
             G=4, Np=10, theta_exact=_beta == 0.0, beta=_beta, **_C)
case("c-binomial-beta-2-5", lambda: with_table(binomial5(), [(1, F.Beta(2.0, 5.0), 0.0, 1.0)]), G=6, Np=12, theta_exact=False, beta=0.1, **_C)
case("c-binomial-beta-half-half", lambda: with_table(binomial5(), [(1, F.Beta(0.5, 0.5), 0.0, 1.0)]), G=6, Np=12, theta_exact=True, beta=0.0, **_C)
case("c-binomial-uniform-inside-bounds", lambda: with_table(binomial5(), [(1, F.Uniform(0.1, 0.9), 0.0, 1.0)]), G=6, Np=12, theta_exact=False,
     support=True, beta=0.1, **_C)
for _N, _na, _G, _Np in ((100, 3, 4, 24), (60, 8, 3, 8)):
    for _name, _mk in (("gamma", lambda mr: F.Gamma(2.0, 0.1)), ("exponential", lambda mr: F.Exponential(0.2)), ("beta", lambda mr: F.Beta(8.0, 2.0))):
        def _lnr(N=_N, na=_na, mk=_mk):
            w = lnr(N, na)
            return with_table(w, [(na, F.Cauchy(0.0, 2.0), -INF, INF), (1, mk(w["min_rt"]), 0.0, w["min_rt"])])
        case(f"c-lnr-na{_na}-tau-{_name}", _lnr, G=_G, Np=_Np, theta_exact=False, beta=0.1, **_C)

# (d) k_propose
case("d-resident-iso5", lambda: with_table(mvn_iso(5), ISO5_A), 12, 4, 16, "k_propose<256,true,TAIL_PREP,true,true>", False, beta=0.1, alpha=0.3,
     loglike_mode=1)
case("d-resident-iso5-snooker", lambda: with_table(mvn_iso(5), ISO5_A), 12, 4, 16, "k_propose<256,true,TAIL_PREP,true,2>", False, beta=0.1,
     alpha=0.3, loglike_mode=1, theta_snooker=0.1)
case("d-resident-iso5-other-kinds", lambda: with_table(mvn_iso(5, centre=0.5), ISO5_B), 12, 4, 16, "k_propose<256,true,TAIL_PREP,true,true>", False,
     beta=0.1, alpha=0.3, loglike_mode=1)
case("d-chain-fuse2-d5", lambda: with_table(mvn_small(5), CHAIN5), 12, 4, 16,
     ["k_propose<256,true,TAIL_PREP_MFMA,false,true>", "k_cross_mfma<", "k_accept_store"], False, exact=False, beta=0.1, alpha=0.3,
     loglike_mode=0, fuse=2)
for _name in ("gamma", "lognormal"):
    case(f"d-tail-obs-hier40-sd-{_name}", lambda pr=SIGMA[_name]: with_table(hier_binomial(40, 92), hier_table(pr, subjects_short())), 12, 6, 16,
         "k_propose<256,true,TAIL_OBS,true,true>", False, lp_rtol=1e-9, beta=0.1, alpha=0.3)

# (e) the long-row kernels: hierarchical Binomial, S = 2600 (2601: an odd row, the general body throughout)
_E = dict(theta_snooker=0.2, beta=0.2, burnin=3, theta_exact=False)


def hier_long(S, sd, blocks):
    return lambda: with_table(hier_binomial(S, 93, blocks), hier_table(SIGMA[sd], subjects_long(S)))


case("e-longrow512-sd-gamma", hier_long(2600, "gamma", "hyper_first"), 6, 16, 16, "k_longrow<512>", **_E)
case("e-longrow512-sd-exponential-subjects-first", hier_long(2600, "exponential", "subjects_first"), 6, 16, 16, "k_longrow<512>", **_E)
# (two 256-thread workgroups per CU once the geometry's moving particles outnumber twice the CUs; recombination keeps the
# row-streaming kernel, which has no such form, out)
case("e-longrow256-sd-lognormal", hier_long(2600, "lognormal", "hyper_first"), 6, 16, 16, "k_longrow<256>", geometry_groups=512, kappa=0.9, **_E)
case("e-longrow256-sd-gamma-subjects-first", hier_long(2600, "gamma", "subjects_first"), 6, 16, 16, "k_longrow<256>", geometry_groups=512, kappa=0.9, **_E)
# (... and an unblocked row at kappa = 1: the whole row in the span loops of the 256-thread instance, which with blocks only runs
# where recombination takes the general per-pair body)
case("e-longrow256-sd-exponential-no-blocks", hier_long(2600, "exponential", None), 6, 16, 16, "k_longrow<256>", geometry_groups=512, **_E)
# 40 x 32: 640 moving particles per colour phase -- the row-streaming kernel; the name is the LAST sweep's
case("e-frozen-big-sd-gamma", hier_long(2600, "gamma", "hyper_first"), 6, 40, 32, "k_frozen_sweep<256,big>", **_E)
case("e-frozen-big-sd-lognormal", hier_long(2600, "lognormal", "hyper_first"), 6, 40, 32, "k_frozen_sweep<256,big>", **_E)
case("e-frozen-sd-exponential-subjects-first", hier_long(2600, "exponential", "subjects_first"), 6, 40, 32, "k_frozen_sweep<256>", **_E)
case("e-frozen-sd-lognormal-subjects-first", hier_long(2600, "lognormal", "subjects_first"), 6, 40, 32, "k_frozen_sweep<256>", **_E)
# DE-MC_Z: history partners; the run is iterations 5 .. 10 behind four prior rows: burnin = 7 puts three of them inside burn-in (a
# base row from the sweep-start snapshot) and three past it, burnin = 3 all six past it
case("e-demcz-longrow512-sd-lognormal", hier_long(2600, "lognormal", "hyper_first"), 4 + 6, 16, 16, "k_longrow<512>", n_initial=4, **Z,
     **dict(_E, burnin=7))
case("e-demcz-frozen-big-sd-exponential", hier_long(2600, "exponential", "hyper_first"), 4 + 6, 40, 16, "k_frozen_sweep<256,big>", n_initial=4,
     **Z, **_E)
case("e-odd-row-longrow512-sd-gamma", hier_long(2601, "gamma", "hyper_first"), 6, 16, 16, "k_longrow<512>", **_E)
case("e-odd-row-longrow256-sd-exponential", hier_long(2601, "exponential", "hyper_first"), 6, 40, 32, "k_longrow<256>", **_E)

assert len({c["id"] for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle alone, as free_run runs it
# ---------------------------------------------------------------------------------------------------------------------
def run_config(c, w):
    """the engine / oracle configuration of a case: free_run's defaults, the workload's own fields, the case's"""
    base = dict(n_groups=c["G"], Np=c["Np"], D=w["D"], n_rows=c["n_it"], schedule=2, seed=4242, burnin=c["n_it"] // 2, trace=0)
    base.update(w["engine"])
    base.update(c["cfg"])
    return base


def oracle_run(orc, c, w):
    """-> (log-posteriors of the starting rows, accept history) of the oracle on workload `w` with the case's settings: the
    sequence of calls and seeds of tests/test_gpu_production.py::free_run"""
    base = run_config(c, w)
    w = for_oracle(w)
    o = orc.Oracle(n_threads=8, **{k: v for k, v in base.items() if k in orc.CFG_KEYS})
    W.configure(o, w)
    rng = np.random.default_rng(5)
    P = c["G"] * c["Np"]
    n_init = int(base.get("n_initial", 0))
    if n_init:
        o.set_history_rows(0, np.stack([w["init"](P, rng) for _ in range(n_init)]))
    o.set_state(w["init"](P, rng))
    lp0 = o.get_state()[1].copy()
    o.step(1 + n_init, c["n_it"] - n_init)
    acc = o.get_history(n_init, c["n_it"])[1].copy()
    o.close()
    return lp0, acc


def kinds_under_test(c, w):
    if c["under_test"] is not None:
        return tuple(c["under_test"])
    return tuple(sorted({k for k in w["pk"] if k not in PLAIN}))


_IDS = [c["id"] for c in CASES]


@pytest.fixture(scope="module")
def runs(orc):
    """each case's oracle run, made once and shared by the tests below"""
    cache = {}

    def get(c):
        if c["id"] not in cache:
            w = c["make"]()
            cache[c["id"]] = (w,) + oracle_run(orc, c, w)
        return cache[c["id"]]
    return get


@pytest.mark.parametrize("c", CASES, ids=_IDS)
def test_the_prior_under_test_decides_something(orc, runs, c):
    """the same run with the kinds under test replaced by Flat makes other accept decisions: a kernel that dropped, or misread,
    the case's prior terms cannot make the oracle's"""
    w, _, acc = runs(c)
    kinds = kinds_under_test(c, w)
    if not kinds:
        assert set(w["pk"]) == {F.PRIOR_FLAT}, "only the all-Flat table has no kind to replace"
        return
    assert any(k in kinds for k in w["pk"])
    _, acc_flat = oracle_run(orc, c, flattened(w, kinds))
    n = int((acc != acc_flat).sum())
    assert n > 0, "the prior under test changed no decision"


@pytest.mark.parametrize("c", CASES, ids=_IDS)
def test_acceptance_is_above_the_free_run_floor(runs, c):
    _, _, acc = runs(c)
    assert acc.mean() > 0.02, f"acceptance {acc.mean():.4f}: free_run would call the comparison vacuous"


@pytest.mark.parametrize("c", [c for c in CASES if c["bites"]], ids=[c["id"] for c in CASES if c["bites"]])
def test_the_bound_that_is_said_to_bite_does(orc, runs, c):
    w, _, acc = runs(c)
    _, acc_open = oracle_run(orc, c, opened(w, c["bites"]))
    assert int((acc != acc_open).sum()) > 0, "opening the bound changed no decision"


@pytest.mark.parametrize("c", [c for c in CASES if c["support"]], ids=[c["id"] for c in CASES if c["support"]])
def test_support_cases_start_partly_outside_the_support(runs, c):
    w, lp0, acc = runs(c)
    out = np.isneginf(lp0)
    assert not np.isnan(lp0).any()
    assert 1 <= out.sum() <= lp0.size // 2, f"{int(out.sum())} of {lp0.size} starting rows at -Inf"
    assert not out.reshape(c["G"], c["Np"]).all(1).any(), "a whole group starts at -Inf"
    lo, hi = np.asarray(w["lo"]), np.asarray(w["hi"])
    th0 = _starting_rows(c, w)
    assert ((th0 >= lo) & (th0 <= hi)).all(), "the -Inf starts must come from the prior's support, not from the bounds"


def _starting_rows(c, w):
    rng = np.random.default_rng(5)
    P = c["G"] * c["Np"]
    for _ in range(int(run_config(c, w).get("n_initial", 0))):
        w["init"](P, rng)
    return w["init"](P, rng)


def test_every_kind_reaches_every_kernel_family():
    """the coverage the case list is for, read from the tables themselves: kinds 2, 3, 4 (a, b != 1), 6, 7, 8, 9 and 10 inside
    k_res_mvn, k_res_obs and k_propose; 6 .. 9 inside k_longrow and k_frozen_sweep"""
    seen = {}
    for c in CASES:
        w = c["make"]()
        name = c["kernel"] if isinstance(c["kernel"], str) else c["kernel"][0]
        fam = name.split("<")[0]
        kinds = {k for k, a, b in zip(w["pk"], w["pa"], w["pb"]) if not (k == F.PRIOR_BETA and a == 1.0 and b == 1.0)}
        seen.setdefault(fam, set()).update(kinds)
    every = {F.PRIOR_HALFCAUCHY, F.PRIOR_UNIFORM, F.PRIOR_BETA, F.PRIOR_GAMMA, F.PRIOR_EXPONENTIAL, F.PRIOR_LOGNORMAL, F.PRIOR_CAUCHY,
             F.PRIOR_TRUNCNORMAL}
    assert every <= seen["k_res_mvn"], every - seen["k_res_mvn"]
    assert every <= seen["k_propose"], every - seen["k_propose"]
    assert every <= seen["k_res_obs"], every - seen["k_res_obs"]
    long_kinds = {F.PRIOR_GAMMA, F.PRIOR_EXPONENTIAL, F.PRIOR_LOGNORMAL, F.PRIOR_CAUCHY}
    assert long_kinds <= seen["k_longrow"] and long_kinds <= seen["k_frozen_sweep"]
