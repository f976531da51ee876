"""A handle that is given one model after another (demc_set_model, demc_set_model_source[_row], demc_set_model_sim in any order)
runs each of them exactly as a handle that only ever held that model: state, weights, history rows and the kernel instances
launched are compared byte for byte.  What a set-model call resets therefore has to be everything the previous model defined --
its buffers, its JIT module, its sizes, its plans.  A refused call leaves what the header says it leaves, and a replay that is
cleared leaves nothing.

Shapes are tiny (4 groups x 8 particles, a few dozen observations, 6 iterations with a migration in every one, history on): the
point is the sequence of calls, not the kernels."""
import numpy as np
import pytest

from conftest import make_problem
from demc_amd import families as F

pytestmark = pytest.mark.gpu
INF = np.inf
G, NP, ITERS = 4, 8, 6
P = G * NP
LOGLIKE_DIRECT = 2


def engine(demc, D, **kw):
    return demc.HipEngine(n_groups=G, Np=NP, D=D, n_rows=ITERS, schedule=2, seed=11, alpha=1.0, burnin=3, **kw)


class Model:
    """one entry of a chain: `apply(engine)` sets the model, its priors and its bounds; `theta0` the rows a run starts from"""

    def __init__(self, name, apply, theta0):
        self.name, self.apply, self.theta0 = name, apply, np.ascontiguousarray(theta0)


def registered(name, prob):
    def apply(e):
        e.set_model(prob["fam"], prob["data"], prob["dims"], prob["hyper"])
        e.set_priors(prob["pk"], prob["pa"], prob["pb"], prob["pref"])
        e.set_bounds(prob["lo"], prob["hi"])
    return Model(name, apply, prob["init"](P))


def run(e, model):
    """priors, bounds and state, then 6 iterations -> everything a caller can read back"""
    model.apply(e)
    e.set_state(model.theta0, ids=np.arange(P))  # (migration moves the ids: every run starts from the same ones)
    e.step(1, ITERS)
    th, w, ids = e.get_state()
    return dict(theta=th, weight=w, ids=ids, kernels=e.last_kernels(), **dict(zip(("h_theta", "h_acc", "h_lp", "h_id"), e.get_history(0, ITERS))))


def assert_same_run(got, want, what):
    assert got["kernels"] == want["kernels"], f"{what}: launched {got['kernels']!r}, a fresh handle {want['kernels']!r}"
    for k, v in want.items():
        if k != "kernels":
            assert got[k].tobytes() == v.tobytes(), f"{what}: {k} differs from a fresh handle's"
    assert got["h_acc"].any(), f"{what}: vacuity guard, nothing was accepted in {ITERS} iterations"


def check_chain(demc, D, chain, **kw):
    veteran = engine(demc, D, **kw)
    try:
        for i, model in enumerate(chain):
            got = run(veteran, model)
            fresh = engine(demc, D, **kw)
            try:
                want = run(fresh, model)
            finally:
                fresh.close()
            assert_same_run(got, want, f"model {i} ({model.name}) after {[m.name for m in chain[:i]]}")
    finally:
        veteran.close()


# ---- the models ---------------------------------------------------------------------------------------------------------
OBS5_SRC = """
__device__ double demc_user_obs(const double* th, int D, const double* x, long long N, long long i,
                                const double* hyper, int nhyper) {
    const double z = (x[i] - (th[0] + th[1] + th[2] + th[3]) * hyper[0]) / th[4];
    return -0.5 * (z * z + 1.8378770664093453) - log(th[4]);
}
"""
GAUSS_SRC = """
__device__ double demc_user_obs(const double* th, int D, const double* x, long long N, long long i,
                                const double* hyper, int nhyper) {
    const double z = (x[i] - th[0]) / th[1];
    return -0.5 * (z * z + 1.8378770664093453) - log(th[1]);
}
"""
# theta = (mu_b0, sd_b0, b0[1:S], sigma), data Y[S][n]; its own prior (Examples/Hierarchical_Example.jl:26-44)
ROW5_SRC = r"""
__device__ double norm_lpdf(double x, double m, double s) { const double z = (x - m) / s; return -(z * z + 1.8378770664093453) / 2.0 - log(s); }
__device__ double hcauchy_lpdf(double x) { return x < 0.0 ? -INFINITY : 0.6931471805599453 - 1.1447298858494002 - log1p(x * x); }
__device__ double demc_user_loglike_row(const double* th, int D, const double* Y, const long long* dims, int ndims,
                                        const double* hyper, int nhyper, int lane, int n_lanes) {
    const long long S = dims[0], n = dims[1];
    double acc = 0.0;
    for (long long s = lane; s < S; s += n_lanes)
        for (long long i = 0; i < n; ++i) acc += norm_lpdf(Y[s * n + i], th[0] + th[2 + s], th[2 + S]);
    return acc;
}
__device__ double demc_user_prior_row(const double* th, int D, const double* hyper, int nhyper, int lane, int n_lanes) {
    const int S = D - 3;
    double acc = 0.0;
    if (lane == 0) acc = norm_lpdf(th[0], 1.0, 1.0) + hcauchy_lpdf(th[1]) + hcauchy_lpdf(th[2 + S]);
    for (int s = lane; s < S; s += n_lanes) acc += norm_lpdf(th[2 + s], 0.0, th[1]);
    return acc;
}
"""
SIM_NORMAL_SRC = """
__device__ double demc_user_sim(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng) {
    return theta[0] + theta[1] * demc_sim_normal(rng);
}
"""


def chain_d5():
    rng = np.random.default_rng(501)
    mvn = registered("MVN_FULL", make_problem("mvn_full", rng, N=40, d=5))
    lba = registered("LBA/2", make_problem("lba", rng, N=36, na=2))
    hbin = registered("HIER_BINOMIAL/3", make_problem("hier_binomial", rng, S=3))

    x = rng.normal(0.4, 1.1, 30)

    def obs(e):
        e.set_model_source(OBS5_SRC, x, [30], hyper=[0.25])
        e.set_priors([F.PRIOR_NORMAL] * 4 + [F.PRIOR_HALFCAUCHY], [0] * 5, [2, 2, 2, 2, 1])
        e.set_bounds([-INF] * 4 + [0], [INF] * 5)
    obs = Model("source", obs, np.concatenate([rng.normal(0, 1, (P, 4)), rng.uniform(0.5, 2.0, (P, 1))], 1))

    hg = make_problem("hier_gaussian", rng, S=2, n=12)

    def row(e):
        e.set_model_source_row(ROW5_SRC, hg["data"], hg["dims"], has_prior=True)
        e.set_priors([F.PRIOR_FLAT] * 5, [0] * 5, [1] * 5)  # the table flat: the source's own function is the prior
        e.set_bounds(hg["lo"], hg["hi"])
    row = Model("row source + prior", row, hg["init"](P))

    Y = np.abs(rng.normal(1.5, 0.6, (24, 2))) + 0.1

    def ode(e):
        e.set_model(F.FAM_ODE_LV, Y, [24, 2], [1.0, 1.0, 0.1, 4])
        e.set_priors([F.PRIOR_NORMAL] * 5, [1.5, 1.0, 3.0, 1.0, 0.6], [0.5, 0.5, 0.5, 0.5, 0.3])
        e.set_bounds([0.1] * 5, [4.0] * 5)
    ode = Model("ODE_LV", ode, np.stack([rng.uniform(1.2, 1.8, P), rng.uniform(0.7, 1.3, P), rng.uniform(2.5, 3.5, P),
                                         rng.uniform(0.7, 1.3, P), rng.uniform(0.4, 0.9, P)], 1))
    return [mvn, lba, obs, row, ode, hbin, mvn]


def chain_d2():
    rng = np.random.default_rng(502)
    prob = make_problem("gaussian", rng, N=40)
    gauss = registered("GAUSSIAN", prob)
    th0 = np.stack([rng.normal(0.3, 0.3, P), rng.uniform(0.8, 1.6, P)], 1)

    def with_table(set_model):
        def apply(e):
            set_model(e)
            e.set_priors(prob["pk"], prob["pa"], prob["pb"], prob["pref"])
            e.set_bounds(prob["lo"], prob["hi"])
        return apply
    sim = Model("SIM_NORMAL/kde", with_table(lambda e: e.set_model_sim(F.SIM_NORMAL, F.SIMEST_KDE_EPANECHNIKOV, 96, prob["data"])), th0)
    usim = Model("user simulator", with_table(lambda e: e.set_model_sim(F.SIM_USER, F.SIMEST_KDE_EPANECHNIKOV, 80, prob["data"], hyper=[0.4],
                                                                          source=SIM_NORMAL_SRC)), th0)
    src = Model("source", with_table(lambda e: e.set_model_source(GAUSS_SRC, prob["data"], [40])), th0)
    return [gauss, sim, usim, src, gauss]


def chain_d1():
    rng = np.random.default_rng(503)
    prob = make_problem("binomial", rng, N=24)
    binom = registered("BINOMIAL", prob)
    k = rng.binomial(12, 0.4, 30).astype(float)

    def freq(e):  # the frequency estimator's table of log(c / n_sim) is a buffer only this kind of model has
        e.set_model_sim(F.SIM_BINOMIAL, F.SIMEST_FREQUENCY, 128, k, hyper=[0.0, 12.0])
        e.set_priors(prob["pk"], prob["pa"], prob["pb"], prob["pref"])
        e.set_bounds(prob["lo"], prob["hi"])
    return [binom, Model("SIM_BINOMIAL/frequency", freq, rng.uniform(0.25, 0.55, (P, 1))), binom]


# ---- chains ---------------------------------------------------------------------------------------------------------------
def test_direct_handle_runs_seven_models_in_turn_like_fresh_handles(demc):
    chain = chain_d5()
    assert len(chain) >= 6 and chain[0] is chain[-1]
    check_chain(demc, 5, chain, loglike_mode=LOGLIKE_DIRECT)


def test_registered_simulated_and_compiled_models_in_turn(demc):
    check_chain(demc, 2, chain_d2())


def test_frequency_table_goes_with_its_model(demc):
    check_chain(demc, 1, chain_d1())


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refused_set_model_sim_leaves_the_previous_model_in_force(demc):
    """demc_set_model_sim validates before it touches the handle: after a refusal the handle steps as one that never saw the call"""
    gauss = chain_d2()[0]
    a, b = engine(demc, 2), engine(demc, 2)
    try:
        gauss.apply(a)
        with pytest.raises(demc.DemcError) as err:
            a.set_model_sim(F.SIM_NORMAL, F.SIMEST_KDE_EPANECHNIKOV, 1, [0.1, 0.2])
        assert err.value.code == demc._ffi.EINVAL and "n_sim < 2" in str(err.value)
        with pytest.raises(demc.DemcError) as err:  # ... and one refused at the last check of the validation, at the data
            a.set_model_sim(F.SIM_NORMAL, F.SIMEST_FREQUENCY, 64, [1.0, 2.5])
        assert err.value.code == demc._ffi.EINVAL and "integer-valued" in str(err.value)
        assert_same_run(run(a, Model("GAUSSIAN", lambda e: None, gauss.theta0)), run(b, gauss), "after a refused demc_set_model_sim")
    finally:
        a.close()
        b.close()


def test_refused_set_model_leaves_no_model(demc):
    """demc_set_model releases the previous model before it reads the new one: after a refusal there is none, and the calls that
    need one say so"""
    gauss = chain_d2()[0]
    e, fresh = engine(demc, 2), engine(demc, 2)
    try:
        run(e, gauss)
        with pytest.raises(demc.DemcError) as err:
            e.set_model(F.FAM_GAUSSIAN, [0.0], [0])
        assert err.value.code == demc._ffi.EINVAL and "GAUSSIAN" in str(err.value)
        for call in (lambda: e.logpost(gauss.theta0), lambda: e.step(1, 1)):
            with pytest.raises(demc.DemcError) as err:
                call()
            assert err.value.code == demc._ffi.EINVAL and "demc_set_model has not been called" in str(err.value)
        assert_same_run(run(e, gauss), run(fresh, gauss), "the model set again")  # (and the handle takes a model again)
    finally:
        e.close()
        fresh.close()


# ---- replay ---------------------------------------------------------------------------------------------------------------
def test_cleared_replay_leaves_nothing_behind(demc):
    gauss = chain_d2()[0]
    rng = np.random.default_rng(504)
    half = NP // 2
    partner = np.empty((P, 3), np.int64)
    for s in range(P):  # two_colour: partners from the resting half
        partner[s] = rng.choice(np.arange(half, NP) if s % NP < half else np.arange(0, half), 3, replace=False)
    a, b = engine(demc, 2), engine(demc, 2)
    try:
        gauss.apply(a)
        a.set_replay(u_step=[0.0], u_group=rng.uniform(0, 1, G), u_part=rng.uniform(0, 1, (P, 5)), partner=partner,
                     u_noise=rng.uniform(0, 1, (P, 2)), z_noise=rng.normal(0, 1, (P, 2)), u_recomb=rng.uniform(0, 1, (P, 2)),
                     mig_groups=[0, 2, 3], mig_particle=rng.integers(0, NP, G))
        a.set_replay()
        assert_same_run(run(a, gauss), run(b, gauss), "after a replay was set and cleared")
    finally:
        a.close()
        b.close()
