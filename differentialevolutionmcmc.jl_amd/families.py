"""Registered model family = what replaces the user closures of DEModel on the device.

The reference's `prior_loglike(theta...)` and `loglike(data, theta...)` are arbitrary Julia closures
(src/structs.jl:176-189); closures cannot run inside a HIP kernel, so the drop-in path accepts the
compositions of Distributions.logpdf that the reference's own tests and examples use, as data:
a per-parameter prior table and a likelihood family id.  Anything else raises DEMC_EUNSUPPORTED.
"""
import numpy as np

# likelihood family ids (include/demc.h)
FAM_GAUSSIAN, FAM_MVN_ISO, FAM_MVN_FULL, FAM_BINOMIAL, FAM_HIER_BINOMIAL, FAM_HIER_GAUSSIAN, FAM_LBA, FAM_LNR, \
    FAM_RASTRIGIN = range(9)
FAM_ODE_LV = 9
FAM_USER = 100
ODE_MAX_T, ODE_MAX_SUBSTEPS = 4096, 1024  # the caps of DEMC_FAM_ODE_LV (csrc/demc_ode.hpp)
# simulation-based likelihoods (demc_set_model_sim): simulator and estimator codes (include/demc.h)
SIM_NORMAL, SIM_BINOMIAL, SIM_LNR, SIM_USER = 0, 1, 2, 100
SIMEST_KDE_EPANECHNIKOV, SIMEST_FREQUENCY, SIMEST_KDE_CHOICE = 0, 1, 2
SIM_MAX_N = 16384
SIM_CHOICE_MAX_N = 15000  # the cap of the "kde_choice" estimator: a choice byte beside every simulated time, and the per-choice tables
PRIOR_FLAT, PRIOR_NORMAL, PRIOR_HALFCAUCHY, PRIOR_UNIFORM, PRIOR_BETA, PRIOR_NORMAL_REF, PRIOR_GAMMA, \
    PRIOR_EXPONENTIAL, PRIOR_LOGNORMAL, PRIOR_CAUCHY = range(10)
PRIOR_TRUNCNORMAL = 10


# ---- priors: named like Distributions.jl -------------------------------------------------------
class Prior:
    kind = PRIOR_FLAT
    a = 0.0
    b = 1.0
    ref = None  # name of the parameter that supplies the scale (hierarchical)


class Flat(Prior):
    pass


class Normal(Prior):
    """Normal(mu, sigma); sigma may be the NAME of another scalar parameter (Normal(0, sigma_b0))."""

    def __init__(self, mu=0.0, sigma=1.0):
        self.a = float(mu)
        if isinstance(sigma, str):
            self.kind, self.ref, self.b = PRIOR_NORMAL_REF, sigma, 1.0
        else:
            self.kind, self.b = PRIOR_NORMAL, float(sigma)


class TruncatedCauchy(Prior):
    """truncated(Cauchy(loc, scale), 0, Inf) (Examples/Gaussian_Example.jl:14)."""
    kind = PRIOR_HALFCAUCHY

    def __init__(self, loc=0.0, scale=1.0):
        self.a, self.b = float(loc), float(scale)


class Uniform(Prior):
    kind = PRIOR_UNIFORM

    def __init__(self, a=0.0, b=1.0):
        self.a, self.b = float(a), float(b)


class Beta(Prior):
    kind = PRIOR_BETA

    def __init__(self, a=1.0, b=1.0):
        self.a, self.b = float(a), float(b)


class Gamma(Prior):
    """Gamma(shape, scale) (Distributions.jl parameterisation)"""
    kind = PRIOR_GAMMA

    def __init__(self, shape=1.0, scale=1.0):
        self.a, self.b = float(shape), float(scale)


class Exponential(Prior):
    """Exponential(scale)"""
    kind = PRIOR_EXPONENTIAL

    def __init__(self, scale=1.0):
        self.a, self.b = 0.0, float(scale)


class LogNormal(Prior):
    kind = PRIOR_LOGNORMAL

    def __init__(self, mu=0.0, sigma=1.0):
        self.a, self.b = float(mu), float(sigma)


class Cauchy(Prior):
    kind = PRIOR_CAUCHY

    def __init__(self, loc=0.0, scale=1.0):
        self.a, self.b = float(loc), float(scale)


class TruncatedNormal(Prior):
    """truncated(Normal(mu, sd), lo, hi) with [lo, hi] the parameter's bounds in DE(bounds=...)
    (Examples/Predator_Prey_Example.jl:28-31): the library divides the Normal density by its mass between the bounds."""
    kind = PRIOR_TRUNCNORMAL

    def __init__(self, mu=0.0, sd=1.0):
        if not (np.isfinite(mu) and np.isfinite(sd) and float(sd) > 0):
            raise ValueError("TruncatedNormal(mu, sd): a finite mu and a finite sd > 0")
        self.a, self.b = float(mu), float(sd)

    def log_mass(self, lo, hi):
        """log(Phi((hi - mu) / sd) - Phi((lo - mu) / sd)) as the library forms it (erfc on the side of the mean where the
        difference does not cancel): what demc_set_priors / demc_set_bounds take off the Normal's constant.  Raises where the
        library refuses: lo >= hi, or a mass that is 0 or not finite."""
        import math
        lo, hi = float(lo), float(hi)
        if not lo < hi:
            raise ValueError("TruncatedNormal: the bounds lo >= hi leave nothing to truncate to")
        zl, zh, r = (lo - self.a) / self.b, (hi - self.a) / self.b, math.sqrt(0.5)
        mass = 0.5 * (math.erfc(zl * r) - math.erfc(zh * r)) if zl > 0.0 else 0.5 * (math.erfc(-zh * r) - math.erfc(-zl * r))
        if not (mass > 0.0 and math.isfinite(mass)):
            raise ValueError("TruncatedNormal: the mass of the Normal between the bounds is 0 or not finite")
        return math.log(mass)


class Priors:
    """prior_loglike as data: one Prior per top-level parameter (applied element-wise to array parameters),
    e.g. Priors(mu=Normal(0, 1), sigma=TruncatedCauchy(0, 1))."""

    def __init__(self, **by_name):
        self.by_name = by_name


# ---- likelihoods -------------------------------------------------------------------------------
class Likelihood:
    family = None

    def pack(self, data, shapes):
        """-> (data array, dims, hyper or None); shapes = list of np.shape of each top-level parameter."""
        raise NotImplementedError


class GaussianLikelihood(Likelihood):
    """sum(logpdf.(Normal(mu, sigma), data)) (Examples/Gaussian_Example.jl:26-28); theta = (mu, sigma)."""
    family = FAM_GAUSSIAN

    def pack(self, data, shapes):
        x = np.asarray(data, dtype=np.float64).ravel()
        return x, [x.size], None


class MvNormalIsoLikelihood(Likelihood):
    """sum(logpdf(MvNormal(mu, sigma^2 I), data)) with data d x N (test/multivariate_normal_tests.jl:31-33);
    theta = (mu[d], sigma)."""
    family = FAM_MVN_ISO

    def pack(self, data, shapes):
        x = np.asarray(data, dtype=np.float64)  # Julia layout: d x N (columns are observations)
        return np.ascontiguousarray(x.T), [x.shape[1], x.shape[0]], None


class MvNormalFullLikelihood(Likelihood):
    """sum(logpdf(MvNormal(mu, Sigma), data)), known full Sigma, data d x N; theta = mu[d] (BASELINE cfg2/cfg3)."""
    family = FAM_MVN_FULL

    def __init__(self, Sigma):
        self.Sigma = np.ascontiguousarray(Sigma, dtype=np.float64)

    def pack(self, data, shapes):
        x = np.asarray(data, dtype=np.float64)
        return np.ascontiguousarray(x.T), [x.shape[1], x.shape[0]], self.Sigma


class BinomialLikelihood(Likelihood):
    """logpdf(Binomial(data.N, theta), data.k) (test/binomial_tests.jl:15-17); data = (N=..., k=...) or arrays."""
    family = FAM_BINOMIAL

    def pack(self, data, shapes):
        n = np.atleast_1d(np.asarray(data["N"] if isinstance(data, dict) else data.N, dtype=np.float64))
        k = np.atleast_1d(np.asarray(data["k"] if isinstance(data, dict) else data.k, dtype=np.float64))
        return np.concatenate([n, k]), [n.size], None


class HierBinomialLikelihood(Likelihood):
    """k_s ~ Binomial(n, logistic(mu_b0 + b0_s)); theta = (mu_b0, sigma_b0, b0[S]) -- the shape of
    Examples/Hierarchical_Example.jl with a Binomial observation model (BASELINE cfg4)."""
    family = FAM_HIER_BINOMIAL

    def __init__(self, n):
        self.n = float(n)

    def pack(self, data, shapes):
        k = np.asarray(data, dtype=np.float64).ravel()
        return k, [k.size], [self.n]


class HierGaussianLikelihood(Likelihood):
    """Examples/Hierarchical_Example.jl:36-44; theta = (mu_b0, sigma_b0, b0[S], sigma); data = S vectors of n."""
    family = FAM_HIER_GAUSSIAN

    def pack(self, data, shapes):
        y = np.ascontiguousarray(np.asarray(data, dtype=np.float64))
        return y, [y.shape[0], y.shape[1]], None


class LBALikelihood(Likelihood):
    """sum(logpdf.(LBA(nu, A, k, tau), choice, rt)) (Examples/Run_LBA.jl:33-37); data = (choice, rt)."""
    family = FAM_LBA

    def pack(self, data, shapes):
        c = np.asarray(data[0], dtype=np.float64).ravel()
        rt = np.asarray(data[1], dtype=np.float64).ravel()
        return np.concatenate([c, rt]), [c.size, int(np.prod(shapes[0])) if shapes[0] else 1], None


class LNRLikelihood(Likelihood):
    """sum(logpdf(LNR(nu, sigma=1, tau), data)) (test/lognormal_race_tests.jl:9-12); data = (choice, rt)."""
    family = FAM_LNR

    def __init__(self, sigma=1.0):
        self.sigma = float(sigma)

    def pack(self, data, shapes):
        c = np.asarray(data[0], dtype=np.float64).ravel()
        rt = np.asarray(data[1], dtype=np.float64).ravel()
        return np.concatenate([c, rt]), [c.size, int(np.prod(shapes[0])) if shapes[0] else 1], [self.sigma]


class LotkaVolterraLikelihood(Likelihood):
    """Examples/Predator_Prey_Example.jl:6-11,56-65: data[:, j] ~ MvNormal(u(t_j), sigma) with u = (x, y) the solution of
    dx/dt = (alpha - beta y) x, dy/dt = (delta x - gamma) y from u0 at t = 0, observed at t_j = j dt; theta = (alpha, beta, gamma,
    delta, sigma).  data: 2 x T as in the reference (row 0 = x, row 1 = y; T x 2 is taken as given when T != 2).  The library
    integrates with classical RK4 at the fixed step dt / substeps, not with the reference's adaptive Tsit5(): DESIGN.md 5.4 has the
    global error against substeps, from which the default is taken."""
    family = FAM_ODE_LV

    def __init__(self, u0=(1.0, 1.0), dt=0.1, substeps=10):
        u0 = np.asarray(u0, dtype=np.float64).ravel()
        if u0.size != 2 or not np.all(np.isfinite(u0)):
            raise ValueError("LotkaVolterraLikelihood: u0 = (x0, y0), finite")
        if not (np.isfinite(dt) and float(dt) > 0):
            raise ValueError("LotkaVolterraLikelihood: dt must be finite and positive")
        if int(substeps) != substeps or not 1 <= int(substeps) <= ODE_MAX_SUBSTEPS:
            raise ValueError(f"LotkaVolterraLikelihood: substeps must be an integer in [1, {ODE_MAX_SUBSTEPS}]")
        self.u0, self.dt, self.substeps = (float(u0[0]), float(u0[1])), float(dt), int(substeps)

    def pack(self, data, shapes):
        """-> (Y[T][2] row-major, [T, 2], [x0, y0, dt, substeps]); refuses what demc_set_model refuses"""
        D = int(sum(int(np.prod(s)) if len(s) else 1 for s in shapes))
        if D != 5:
            raise ValueError(f"LotkaVolterraLikelihood reads theta = (alpha, beta, gamma, delta, sigma): D = 5, the model has {D}")
        y = np.asarray(data, dtype=np.float64)
        if y.ndim != 2 or 2 not in y.shape:
            raise ValueError("LotkaVolterraLikelihood: data must be 2 x T (or T x 2): the observed x and y per time")
        if y.shape[0] == 2:  # the reference's layout: a column per time
            y = y.T
        T = y.shape[0]
        if not 1 <= T <= ODE_MAX_T:
            raise ValueError(f"LotkaVolterraLikelihood: T = {T} observation times, must be in [1, {ODE_MAX_T}]")
        if not np.all(np.isfinite(y)):
            raise ValueError("LotkaVolterraLikelihood: data must be finite")
        return np.ascontiguousarray(y), [T, 2], [self.u0[0], self.u0[1], self.dt, float(self.substeps)]


class RastriginObjective(Likelihood):
    """objective of test/optimization_tests.jl:15-23 (optimize mode only)."""
    family = FAM_RASTRIGIN

    def pack(self, data, shapes):
        return None, [], None


class SourceLikelihood(Likelihood):
    """Plug-in for models outside the registered family.  The reference's `loglike(data, theta...)` closures are sums
    of per-observation log-densities (e.g. Examples/Gaussian_Example.jl:26-28); a Julia closure cannot run in a kernel,
    but the same term written as a HIP device function can:

        __device__ double demc_user_obs(const double* theta, int D, const double* data, long long N, long long i,
                                        const double* hyper, int nhyper);   // log-density of observation i

    `data` is flattened row-major with shape (N, ...) (observations first); the source is JIT-compiled for gfx950 by
    demc_set_model_source (include/demc.h)."""
    family = FAM_USER

    def __init__(self, source, hyper=None, row=False, has_prior=False):
        """row=True: the whole-row form (demc_set_model_source_row): `source` defines demc_user_loglike_row(theta, D, data, dims,
        ndims, hyper, nhyper, lane, n_lanes) -- and demc_user_prior_row(...) with has_prior=True -- evaluated by one workgroup
        per proposal; for likelihoods that are not a flat sum over observations and priors the per-scalar table cannot
        express (Examples/Hierarchical_Example.jl:26-44)."""
        self.source, self.hyper, self.row, self.has_prior = source, hyper, bool(row), bool(has_prior)

    def pack(self, data, shapes):
        x = np.ascontiguousarray(np.asarray(data, dtype=np.float64))
        return x, list(x.shape), self.hyper


# ---- simulation-based likelihoods: the model is a simulator (Examples/KDE_Example.jl, Examples/Binomial_ABC.jl) ----
class Simulator:
    code = None
    source = None
    n_params = None  # scalars of theta the simulator reads (None: any)
    pairs = False    # True: a simulated value is a (choice, response time) pair -- the "kde_choice" estimator's simulators

    def hyper(self):
        return []


class SimNormal(Simulator):
    """rand(Normal(mu, sigma), n_sim) (Examples/KDE_Example.jl:12); theta = (mu, sigma)."""
    code = SIM_NORMAL
    n_params = 2


class SimBinomial(Simulator):
    """rand(Binomial(n, theta)) n_sim times (Examples/Binomial_ABC.jl:19); theta = p."""
    code = SIM_BINOMIAL
    n_params = 1

    def __init__(self, n):
        if int(n) != n or not 1 <= int(n) <= 1024:
            raise ValueError("SimBinomial(n): n must be an integer in [1, 1024]")
        self.n = int(n)

    def hyper(self):
        return [float(self.n)]


class SimLNR(Simulator):
    """The log-normal race of LNRLikelihood as a simulator of (choice, response time) pairs: theta = (nu[K], tau), K in [2, 8];
    T_k = exp(nu_k + sigma z_k), choice = 1 + argmin_k T_k, rt = tau + min_k T_k.  For the "kde_choice" estimator."""
    code = SIM_LNR
    pairs = True

    def __init__(self, sigma=1.0):
        if not float(sigma) > 0:
            raise ValueError("SimLNR(sigma): sigma > 0")
        self.sigma = float(sigma)

    def hyper(self):
        return [self.sigma]


class SimSource(Simulator):
    """A simulator written as a HIP device function, one call per simulated value:

        __device__ double demc_user_sim(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng);

    which draws with demc_sim_uniform(rng) / demc_sim_normal(rng) / demc_sim_u32(rng) (include/demc.h).  choice=True: a simulator
    of (choice, response time) pairs for the "kde_choice" estimator,

        __device__ double demc_user_sim_choice(const double* theta, int D, const double* hyper, int nhyper,
                                               demc_sim_rng* rng, int* choice);   // returns t, sets *choice in [0, 255]

    (choice 0: no response)."""
    code = SIM_USER

    def __init__(self, source, hyper=None, choice=False):
        if not isinstance(source, str) or not source.strip():
            raise ValueError("SimSource(source): HIP source defining demc_user_sim (demc_user_sim_choice with choice=True)")
        self.source = source
        self.pairs = bool(choice)
        self._hyper = [] if hyper is None else [float(x) for x in np.asarray(hyper, dtype=np.float64).ravel()]

    def hyper(self):
        return self._hyper


class SimulatedLikelihood(Likelihood):
    """A likelihood without a closed form, estimated per proposal from n_sim simulated values (demc_set_model_sim):
    estimator "kde" = sum(log(max(1e-10, pdf(kde, x)))) with an Epanechnikov kernel (Examples/KDE_Example.jl:10-18; bandwidth
    0.0 = the rule of thumb 0.9 sd n^(-1/5)), "frequency" = log(#{sim == x} / n_sim) summed over the observations
    (Examples/Binomial_ABC.jl:15-22).  Data: scalar observations (or the reference's (N=..., k=...) with a SimBinomial).
    "kde_choice" = choice and response-time models: the simulator (SimLNR(), SimSource(..., choice=True)) gives (choice, rt) pairs,
    the data are (choice, rt) as for LBALikelihood / LNRLikelihood, and each observation is scored under the defective
    Epanechnikov density of its choice, normalised by ALL n_sim values (include/demc.h: DEMC_SIMEST_KDE_CHOICE)."""
    family = None  # not a DEMC_FAM_* family: sampler.configure_engine routes it to set_model_sim
    ESTIMATORS = {"kde": SIMEST_KDE_EPANECHNIKOV, "frequency": SIMEST_FREQUENCY, "kde_choice": SIMEST_KDE_CHOICE}

    def __init__(self, simulator, estimator="kde", n_sim=10_000, bandwidth=0.0):
        if not isinstance(simulator, Simulator) or simulator.code is None:
            raise TypeError("SimulatedLikelihood(simulator): SimNormal(), SimBinomial(n), SimLNR() or SimSource(source)")
        if estimator not in self.ESTIMATORS:
            raise ValueError(f"estimator must be one of {sorted(self.ESTIMATORS)}")
        if simulator.pairs != (estimator == "kde_choice"):
            raise ValueError(f"{type(simulator).__name__} simulates {'(choice, rt) pairs' if simulator.pairs else 'scalars'}: "
                             f"it cannot be scored by the {estimator!r} estimator")
        cap = SIM_CHOICE_MAX_N if estimator == "kde_choice" else SIM_MAX_N
        if int(n_sim) != n_sim or not 2 <= int(n_sim) <= cap:
            raise ValueError(f"n_sim must be an integer in [2, {cap}] (the sample of a proposal is held in LDS)")
        if not np.isfinite(bandwidth) or bandwidth < 0:
            raise ValueError("bandwidth must be finite and >= 0 (0: the rule of thumb)")
        self.simulator, self.estimator, self.n_sim, self.bandwidth = simulator, estimator, int(n_sim), float(bandwidth)

    def pack(self, data, shapes):
        """-> (observations, [N], hyper = [bandwidth, the simulator's own ...]); "kde_choice": observations = [choices..., rts...]"""
        D = int(sum(int(np.prod(s)) if len(s) else 1 for s in shapes))
        if self.estimator == "kde_choice":
            c = np.atleast_1d(np.asarray(data[0], dtype=np.float64)).ravel()
            rt = np.atleast_1d(np.asarray(data[1], dtype=np.float64)).ravel()
            if c.size < 1 or c.size != rt.size:
                raise ValueError("SimulatedLikelihood: data = (choice, rt), two arrays of the same length >= 1")
            lnr = isinstance(self.simulator, SimLNR)
            if lnr and not 2 <= D - 1 <= 8:
                raise ValueError(f"SimLNR reads (nu[K], tau) with K in [2, 8], the model has {D} parameters")
            hi = D - 1 if lnr else 255
            if not np.all((c == np.floor(c)) & (c >= 1) & (c <= hi)):
                raise ValueError(f"choices must be integers in [1, {hi}]")
            if not np.all(np.isfinite(rt)):
                raise ValueError("response times must be finite")
            return np.concatenate([c, rt]), [c.size], [self.bandwidth] + list(self.simulator.hyper())
        if isinstance(data, dict) or hasattr(data, "k"):  # the reference's NamedTuple (N = ..., k = ...)
            data = data["k"] if isinstance(data, dict) else data.k
        x = np.atleast_1d(np.asarray(data, dtype=np.float64)).ravel()
        if x.size < 1:
            raise ValueError("SimulatedLikelihood: no observations")
        if self.estimator == "frequency" and not np.all(x == np.floor(x)):
            raise ValueError("the frequency estimator needs integer-valued data")
        if self.simulator.n_params is not None and D != self.simulator.n_params:
            raise ValueError(f"{type(self.simulator).__name__} reads {self.simulator.n_params} parameters, the model has {D}")
        return x, [x.size], [self.bandwidth] + list(self.simulator.hyper())

    def configure(self, eng, data, shapes):
        x, _, hyper = self.pack(data, shapes)
        eng.set_model_sim(self.simulator.code, self.ESTIMATORS[self.estimator], self.n_sim, x, hyper, self.simulator.source)
