"""Simulation-based likelihoods on the GPU (include/demc.h: demc_set_model_sim; csrc/demc_simlike.hpp: k_sim_loglike) against the
numpy restatement of tests/test_simlike_host.py, which regenerates every draw from the addressed Philox stream 7.

Bars: log-likelihoods / log-posteriors at rtol 1e-9 (the project's log-posterior bar) where no observation sits at the 1e-10
floor -- asserted on the restatement, min f >= 1e-2 --; the frequency estimator bit for bit (integer counts, the log terms from
the host's libm); accept decisions exactly, except where |u - exp(w' - w)| < 1e-7 (a 1e-9 difference in w' can flip those);
same seed, sharded or not: same bits."""
import math

import numpy as np
import pytest

import test_simlike_host as R

pytestmark = pytest.mark.gpu
INF = np.inf
SIM_NORMAL, SIM_BINOMIAL, SIM_USER, KDE, FREQ = 0, 1, 100, 0, 1


@pytest.fixture()
def D(demc):
    return demc


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / max(abs(b), 1e-300)


def clipped_data(rng, mu, sg, N):
    """observations as they come from N(0, 1), clipped to within 1.5 sigma of the row's mu: none of them at the floor"""
    return np.clip(rng.normal(0.0, 1.0, N), mu - 1.5 * sg, mu + 1.5 * sg)


# ---- 4. demc_logpost vs the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 50, 333])
@pytest.mark.parametrize("n_sim", [257, 4096, 10_000])
def test_logpost_kde_normal_equals_the_restatement(D, n_sim, N):
    rng = np.random.default_rng(1000 * N + n_sim)
    seed, n_rows = 77 + n_sim, 6
    theta = np.stack([rng.normal(0, 0.5, n_rows), rng.uniform(0.5, 2.0, n_rows)], 1)
    e = D.HipEngine(n_groups=2, Np=4, D=2, seed=seed, schedule=2)
    worst = 0.0
    try:
        e.set_bounds([-INF, 0.0], [INF, INF])
        for r in range(n_rows):
            x = clipped_data(rng, theta[r, 0], theta[r, 1], N)
            e.set_model_sim(SIM_NORMAL, KDE, n_sim, x)
            got = e.logpost(theta)[r]  # row r of the call is evaluated at entity r, iter = sweep = 0
            want, f = R.kde_loglike(R.sim_normal(theta[r], seed, 0, 0, r, n_sim), x)
            assert f.min() >= 1e-2, f"vacuity guard: an observation at the floor (min f = {f.min():.3g})"
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-9, (r, got, want)
    finally:
        e.close()
    print(f"kde/normal n_sim={n_sim} N={N}: max relative difference {worst:.3g}")


def test_logpost_kde_fixed_bandwidth_floor_and_degenerate_rows(D):
    seed, n_sim = 5, 2000
    e = D.HipEngine(n_groups=1, Np=4, D=2, seed=seed)
    try:
        e.set_bounds([-INF, -INF], [INF, INF])
        th = np.array([[0.2, 1.1], [0.0, 0.0], [0.0, INF], [0.3, 0.7]])
        s0 = R.sim_normal(th[0], seed, 0, 0, 0, n_sim)
        _, h = R.kde_density(s0, [0.0])
        # one observation >= 10 h outside the sample: its term is exactly log(1e-10)
        far = s0.max() + 10.0 * h
        e.set_model_sim(SIM_NORMAL, KDE, n_sim, [far])
        got = e.logpost(th)
        assert got[0] == math.log(1e-10), (got[0], math.log(1e-10))
        assert got[1] == -INF and got[2] == -INF  # sd == 0; non-finite simulated values: -Inf, never NaN
        x = np.array([0.1, 0.4, far, -0.3])
        e.set_model_sim(SIM_NORMAL, KDE, n_sim, x)
        got = e.logpost(th)
        want, f = R.kde_loglike(s0, x)
        assert f[2] == 0.0 and rel(got[0], want) <= 1e-9, (got[0], want)
        # a caller's bandwidth (hyper[0] > 0) replaces the rule of thumb
        e.set_model_sim(SIM_NORMAL, KDE, n_sim, x[[0, 1, 3]], hyper=[0.31])
        got = e.logpost(th)
        for r in (0, 3):
            want, f = R.kde_loglike(R.sim_normal(th[r], seed, 0, 0, r, n_sim), x[[0, 1, 3]], 0.31)
            assert f.min() >= 1e-2 and rel(got[r], want) <= 1e-9, (r, got[r], want)
    finally:
        e.close()


@pytest.mark.parametrize("N", [1, 50, 333])
@pytest.mark.parametrize("n_sim", [257, 4096, 10_000])
def test_logpost_frequency_binomial_bit_for_bit(D, n_sim, N):
    rng = np.random.default_rng(31 * N + n_sim)
    seed, n_trials = 4242 + N, 10
    k = rng.binomial(n_trials, 0.5, N).astype(np.float64)
    p = np.array([0.5, 0.31, 0.77, 0.02, 0.5, 0.93])  # 0.02: some observed count is never simulated -> -Inf (N > 1)
    e = D.HipEngine(n_groups=2, Np=4, D=1, seed=seed)
    try:
        e.set_bounds([0.0], [1.0])
        e.set_model_sim(SIM_BINOMIAL, FREQ, n_sim, k, hyper=[0.0, n_trials])
        got = e.logpost(p[:, None])
        want = np.array([R.freq_loglike(R.sim_binomial(p[r], n_trials, seed, 0, 0, r, n_sim), k) for r in range(p.size)])
        assert np.array_equal(got, want), (got, want)  # bit for bit, -Inf included
        if N >= 50:
            assert want[3] == -INF and np.isfinite(want[0])
    finally:
        e.close()
    print(f"frequency/binomial n_sim={n_sim} N={N}: bit-identical, {int(np.isinf(want).sum())} rows at -Inf")


def test_logpost_equals_the_weights_of_set_state_and_kde_on_counts(D):
    """demc_logpost(theta)[r] is the weight demc_set_state gives slot r; the KDE estimator also runs on the Binomial simulator"""
    seed, n_sim, n_trials = 9, 3000, 40
    rng = np.random.default_rng(2)
    k = np.clip(rng.binomial(n_trials, 0.4, 25), 13, 19).astype(np.float64)  # (inside the bulk for every row below)
    p = rng.uniform(0.37, 0.43, (8, 1))
    e = D.HipEngine(n_groups=2, Np=4, D=1, seed=seed)
    try:
        e.set_bounds([0.0], [1.0])
        e.set_priors([4], [2.0], [3.0])
        e.set_model_sim(SIM_BINOMIAL, KDE, n_sim, k, hyper=[0.0, n_trials])
        e.set_state(p)
        w = e.get_state()[1]
        assert np.array_equal(w, e.logpost(p))
        for r in range(8):
            ll, f = R.kde_loglike(R.sim_binomial(p[r, 0], n_trials, seed, 0, 0, r, n_sim), k)
            assert f.min() >= 1e-2
            assert rel(w[r], ll + R.log_prior(4, 2.0, 3.0, p[r, 0])) <= 1e-9
    finally:
        e.close()


# ---- 5. teacher-forced steps ---------------------------------------------------------------------------------------------
def _migrate(e, it):
    e.migration_pack_dev(it, None)  # NULL: the handle's own staging rows (single shard)
    e.migration_apply_dev(it, None)


def _expected_w(prop, x, n_sim, seed, sweep, it, slot):
    if not prop[1] >= 0.0:  # outside the bounds: -Inf (utilities.jl:92-99)
        return -INF
    ll, _ = R.kde_loglike(R.sim_normal(prop, seed, sweep, it, slot, n_sim), x)
    return R.log_prior(1, 0.0, 1.0, prop[0]) + R.log_prior(2, 0.0, 1.0, prop[1]) + ll


def test_teacher_forced_steps(D):
    G, Np, n_sim, N, seed, n_it, burnin = 4, 6, 1000, 20, 20250, 30, 15
    rng = np.random.default_rng(8)
    x = rng.normal(0.2, 1.0, N)
    cfg = dict(n_groups=G, Np=Np, D=2, n_rows=n_it, seed=seed, burnin=burnin, alpha=0.3, beta=0.15, trace=1, schedule=2)
    th0 = np.stack([rng.normal(0.2, 0.3, G * Np), rng.uniform(0.8, 1.5, G * Np)], 1)

    def setup(e, sim=True):
        if sim:
            e.set_model_sim(SIM_NORMAL, KDE, n_sim, x)
        else:
            e.set_model(D.families.FAM_GAUSSIAN, x, [N])
        e.set_priors([1, 2], [0.0, 0.0], [1.0, 1.0])
        e.set_bounds([-INF, 0.0], [INF, INF])

    e, gauss = D.HipEngine(**cfg), D.HipEngine(**cfg)
    worst, n_dec, n_skip, n_acc, n_mig = 0.0, 0, 0, 0, 0
    try:
        setup(e)
        setup(gauss, sim=False)
        e.set_state(th0)
        # the new stream disturbs no other: from the same state and weights a Gaussian-family handle makes the same first-phase
        # proposals, bit for bit (the second colour phase reads rows the first phase's accept decisions have already moved)
        _, w0, ids = e.get_state()
        gauss.set_state(th0, w0, ids)
        clone = D.HipEngine(**cfg)
        try:
            setup(clone)
            clone.set_state(th0, w0, ids)
            clone.step(1, 1)
            gauss.step(1, 1)
            first = (np.arange(G * Np) % Np) < Np // 2
            assert np.array_equal(clone.get_trace()["proposal"][first], gauss.get_trace()["proposal"][first])
            assert np.array_equal(clone.get_trace()["idx"][first], gauss.get_trace()["idx"][first])
            assert "k_sim_loglike<kde,normal> + k_accept_store" in clone.last_kernels(), clone.last_kernels()
        finally:
            clone.close()
        for it in range(1, n_it + 1):
            if e.migration_due(it):
                _migrate(e, it)
                n_mig += 1
            tb, wb, _ = e.get_state()
            e.update(it, 1)
            tr = e.get_trace()
            ta, wa, _ = e.get_state()
            for s in range(G * Np):
                prop = tr["proposal"][s]
                want = _expected_w(prop, x, n_sim, seed, 0, it, s)
                got = tr["w_prop"][s]
                worst = max(worst, rel(got, want))
                assert rel(got, want) <= 1e-9, (it, s, got, want)
                ua = R.draw_blocks(seed, R.S_PART, 0, it, s, [3])[0]
                u = R.u53(ua[0], ua[1])
                ratio = math.exp(want - wb[s] + tr["log_adj"][s]) if want > -INF else 0.0
                n_dec += 1
                if abs(u - ratio) < 1e-7:
                    n_skip += 1
                else:
                    assert bool(tr["accepted"][s]) == (ratio >= 1.0 or u <= ratio), (it, s, u, ratio)
                if tr["accepted"][s]:
                    n_acc += 1
                    assert np.array_equal(ta[s], prop) and wa[s] == got
                else:
                    assert np.array_equal(ta[s], tb[s]) and wa[s] == wb[s]  # the resting particle keeps its noisy weight
        assert n_mig >= 3 and 0 < n_acc < n_dec
        assert n_skip < 0.01 * n_dec
    finally:
        e.close()
        gauss.close()
    print(f"teacher-forced: {n_dec} decisions, {n_acc} accepted, {n_skip} skipped, {n_mig} migrations, max relative difference of w' {worst:.3g}")


def test_teacher_forced_block_sweeps_address_the_sweep(D):
    G, Np, n_sim, N, seed = 3, 4, 600, 12, 606
    rng = np.random.default_rng(18)
    x = rng.normal(0.0, 1.0, N)
    e = D.HipEngine(n_groups=G, Np=Np, D=2, n_rows=6, seed=seed, burnin=3, alpha=0.3, beta=0.1, trace=1, schedule=2)
    worst = 0.0
    try:
        e.set_model_sim(SIM_NORMAL, KDE, n_sim, x)
        e.set_priors([1, 2], [0.0, 0.0], [1.0, 1.0])
        e.set_bounds([-INF, 0.0], [INF, INF])
        e.set_blocks([[1, 0], [0, 1]])
        e.set_state(np.stack([rng.normal(0, 0.3, G * Np), rng.uniform(0.8, 1.5, G * Np)], 1))
        for it in range(1, 7):
            e.step(it, 1)
            tr = e.get_trace()  # of the LAST sweep of the iteration: sweep 1
            ta, wa, _ = e.get_state()
            for s in range(G * Np):
                want = _expected_w(tr["proposal"][s], x, n_sim, seed, 1, it, s)
                worst = max(worst, rel(tr["w_prop"][s], want))
                assert rel(tr["w_prop"][s], want) <= 1e-9, (it, s, tr["w_prop"][s], want)
                if np.isfinite(want):
                    assert rel(tr["w_prop"][s], _expected_w(tr["proposal"][s], x, n_sim, seed, 0, it, s)) > 1e-9  # not sweep 0's draws
                if tr["accepted"][s]:
                    assert np.array_equal(ta[s], tr["proposal"][s]) and wa[s] == tr["w_prop"][s]
    finally:
        e.close()
    print(f"block sweeps: max relative difference of w' {worst:.3g}")


# ---- 6. determinism, shards, geometry ------------------------------------------------------------------------------------
def _run(D, make, n_it, th0, x, n_sim, sharded=False):
    e = make()

    def setup(s):
        s.set_model_sim(SIM_NORMAL, KDE, n_sim, x)
        s.set_priors([1, 2], [0.0, 0.0], [1.0, 1.0])
        s.set_bounds([-INF, 0.0], [INF, INF])

    try:
        e.each(setup) if sharded else setup(e)
        e.set_state(th0)
        e.step(1, n_it)
        return e.get_history(0, n_it) + e.get_state()
    finally:
        e.close()


def test_same_seed_same_bits_sharded_or_not(D):
    G, Np, n_sim, n_it = 4, 6, 512, 25
    rng = np.random.default_rng(44)
    x = rng.normal(0.1, 1.0, 30)
    th0 = np.stack([rng.normal(0, 0.3, G * Np), rng.uniform(0.8, 1.5, G * Np)], 1)
    cfg = dict(n_groups=G, Np=Np, D=2, n_rows=n_it, seed=31337, burnin=10, alpha=0.3, beta=0.1)
    ref = _run(D, lambda: D.HipEngine(**cfg), n_it, th0, x, n_sim)
    assert np.isfinite(ref[2]).all() and ref[1].sum() > 0
    for name, out in (("again", _run(D, lambda: D.HipEngine(**cfg), n_it, th0, x, n_sim)),
                      ("geometry_groups", _run(D, lambda: D.HipEngine(geometry_groups=64, **cfg), n_it, th0, x, n_sim)),
                      ("two shards", _run(D, lambda: D.MultiEngine(2, device_ids=[0, 0], **cfg), n_it, th0, x, n_sim, sharded=True))):
        for a, b in zip(ref, out):
            assert np.array_equal(a, b), name


# ---- 7. user simulators ---------------------------------------------------------------------------------------------------
SRC_NORMAL = """
__device__ double demc_user_sim(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng) {
    return theta[0] + theta[1] * demc_sim_normal(rng);
}
"""
SRC_SHIFTED_EXP = """
__device__ double demc_user_sim(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng) {
    return hyper[0] - theta[0] * log(demc_sim_uniform(rng));   // shift + Exponential(scale theta[0])
}
"""


def test_user_simulators_equal_the_restatement(D):
    seed, n_sim = 12321, 4096
    rng = np.random.default_rng(3)
    worst = 0.0
    e = D.HipEngine(n_groups=2, Np=4, D=2, seed=seed, n_rows=2)
    try:
        e.set_bounds([-INF, 0.0], [INF, INF])
        th = np.stack([rng.normal(0, 0.5, 5), rng.uniform(0.5, 2.0, 5)], 1)
        for r in range(5):
            x = clipped_data(rng, th[r, 0], th[r, 1], 40)
            e.set_model_sim(SIM_USER, KDE, n_sim, x, source=SRC_NORMAL)
            got = e.logpost(th)[r]
            w = R.user_words(seed, 0, 0, r, n_sim, 1)
            want, f = R.kde_loglike(th[r, 0] + th[r, 1] * R.box_muller(w[:, 0], w[:, 1])[0], x)
            assert f.min() >= 1e-2
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-9, (r, got, want)
        e.set_state(np.tile(th[:4], (2, 1)))
        e.step(1, 1)
        assert "k_sim_loglike<kde,user> + k_accept_store" in e.last_kernels(), e.last_kernels()
    finally:
        e.close()
    e = D.HipEngine(n_groups=2, Np=4, D=1, seed=seed)
    try:
        e.set_bounds([0.0], [INF])
        shift = 0.25
        scale = np.array([0.6, 1.0, 1.7, 2.4])
        for r in range(4):
            x = shift + scale[r] * rng.uniform(0.3, 1.5, 30)  # inside the bulk of the density: no observation at the floor
            e.set_model_sim(SIM_USER, KDE, n_sim, x, hyper=[0.0, shift], source=SRC_SHIFTED_EXP)
            got = e.logpost(scale[:, None])[r]
            w = R.user_words(seed, 0, 0, r, n_sim, 1)
            want, f = R.kde_loglike(shift - scale[r] * np.log(R.u32unit(w[:, 0])), x)
            assert f.min() >= 1e-2
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-9, (r, got, want)
        with pytest.raises(D.DemcError) as err:
            e.set_model_sim(SIM_USER, KDE, n_sim, [1.0], source="__device__ double demc_user_sim(const double* theta, int D, "
                            "const double* hyper, int nhyper, demc_sim_rng* rng) { return theta[0] +; }")
        assert err.value.code == D._ffi.EINVAL and "error" in str(err.value) and "does not compile" in str(err.value)
    finally:
        e.close()
    print(f"user simulators: max relative difference {worst:.3g}")


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(D):
    e = D.HipEngine(n_groups=1, Np=4, D=2, seed=1)
    try:
        for kw, text in ((dict(simulator=SIM_NORMAL, estimator=KDE, n_sim=16385, data=[0.0]), "above the cap of 16384"),
                         (dict(simulator=SIM_NORMAL, estimator=FREQ, n_sim=100, data=[1.0, 2.5]), "integer-valued"),
                         (dict(simulator=SIM_NORMAL, estimator=KDE, n_sim=1, data=[0.0]), "n_sim < 2"),
                         (dict(simulator=SIM_USER, estimator=KDE, n_sim=100, data=[0.0]), "needs hip_source"),
                         (dict(simulator=SIM_NORMAL, estimator=KDE, n_sim=100, data=[0.0], source=SRC_NORMAL), "registered simulator"),
                         (dict(simulator=SIM_BINOMIAL, estimator=FREQ, n_sim=100, data=[1.0], hyper=[0.0, 10.0]), "theta=p")):
            with pytest.raises(D.DemcError) as err:
                e.set_model_sim(**kw)
            assert err.value.code == D._ffi.EINVAL and text in str(err.value), (text, str(err.value))
        with pytest.raises(D.DemcError):  # ... and the handle is left without a model, not with half of one
            e.logpost(np.zeros((1, 2)))
    finally:
        e.close()


# ---- 9. statistical gates: the reference's two examples against the closed-form families ----------------------------------
def _mcse(x):
    """Monte-Carlo standard error of the mean from the split chains (chains.py's split): [n][chains]"""
    h = x.shape[0] // 2
    s = np.concatenate([x[:h], x[h:2 * h]], axis=1)
    return float(s.mean(axis=0).std(ddof=1) / math.sqrt(s.shape[1]))


def test_kde_example_posterior_matches_the_gaussian_family(D):
    data = np.random.default_rng(50514).normal(0.0, 1.0, 50)

    def run(loglike):
        rng = np.random.default_rng(7)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("mu", "sigma"), data=data, loglike=loglike,
                          prior_loglike=D.Priors(mu=D.Normal(0, 1), sigma=D.TruncatedCauchy(0, 1)))
        de = D.DE(sample_prior=prior, bounds=((-INF, INF), (0.0, INF)), burnin=1000, Np=6, n_groups=4)
        return D.sample(model, de, D.HIPBackend(seed=2024), 3000)

    yard = run(D.GaussianLikelihood())
    kde = run(D.SimulatedLikelihood(D.SimNormal(), estimator="kde", n_sim=10_000))
    assert len(kde) == 2000
    ym, km = yard.mean(), kde.mean()
    # the kernel adds variance h^2 / 5, h = 0.9 sigma (10^4)^(-1/5) = 0.143 sigma: the KDE's sigma sits 0.2 % off; mu: no bias
    bias = dict(mu=0.0, sigma=0.5 * (0.9 * 10_000 ** -0.2) ** 2 / 5 * ym["sigma"])
    for nm in ("mu", "sigma"):
        margin = 5.0 * _mcse(yard[nm]) + bias[nm]
        print(f"KDE example {nm}: yardstick {ym[nm]:.5f}, simulated {km[nm]:.5f}, difference {km[nm] - ym[nm]:+.5f}, margin {margin:.5f}")
    for nm in ("mu", "sigma"):
        assert abs(km[nm] - ym[nm]) <= 5.0 * _mcse(yard[nm]) + bias[nm], nm


def test_binomial_abc_posterior_matches_the_binomial_family(D):
    N, k = 10, 6

    def run(loglike, data):
        rng = np.random.default_rng(88484)
        prior = lambda: [rng.beta(1, 1)]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("theta",), data=data, loglike=loglike, prior_loglike=D.Priors(theta=D.Beta(1, 1)))
        de = D.DE(sample_prior=prior, bounds=((0.0, 1.0),), burnin=1000, Np=3, n_groups=4, sigma=0.01)
        return D.sample(model, de, D.HIPBackend(seed=515, schedule="synchronous"), 3000)

    yard = run(D.BinomialLikelihood(), dict(N=[N], k=[k]))
    abc = run(D.SimulatedLikelihood(D.SimBinomial(N), estimator="frequency", n_sim=10_000), dict(N=N, k=k))
    diff, margin = abc.mean()["theta"] - yard.mean()["theta"], 5.0 * _mcse(yard["theta"])
    print(f"Binomial ABC theta: yardstick {yard.mean()['theta']:.5f}, simulated {abc.mean()['theta']:.5f}, difference {diff:+.5f}, margin {margin:.5f}")
    assert abs(diff) <= margin
