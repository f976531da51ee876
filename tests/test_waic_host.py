"""WAIC on the host: chains.waic_from_loglik -- the definition demc_waic is held to on the GPU -- against known
answers, and compare_waic.  No GPU."""
import math

import numpy as np
import pytest


def _point(w):
    return {k: w.pointwise[:, j] for j, k in enumerate(("lppd", "p_waic", "mean", "elpd"))}


def test_identical_draws_have_no_penalty(demc):
    l = np.array([-1.25, -0.5, -7.0, 0.75])
    w = demc.waic_from_loglik(np.tile(l, (17, 1)))
    p = _point(w)
    assert np.array_equal(p["p_waic"], np.zeros(4)) and np.array_equal(p["mean"], l)
    np.testing.assert_allclose(p["lppd"], l, rtol=0, atol=4e-16 * 7)  # (log(17 e^0) - log 17 in the reference's own arithmetic)
    assert w.p_waic == 0.0 and w.n_high == 0 and w.n_nonfinite == 0
    assert w.lppd == pytest.approx(l.sum(), abs=1e-14) and w.waic == -2 * w.elpd_waic and w.dbar == pytest.approx(-2 * l.sum(), abs=1e-14)


def test_two_draws_by_hand(demc):
    # observation 0: l = (log 1/2, log 1/4): lppd = log((1/2 + 1/4) / 2) = log 3/8; mean = -(3/2) log 2; p_waic = (log 2)^2 / 2
    # observation 1: l = (0, -2): lppd = log((1 + e^-2) / 2); mean = -1; p_waic = 2
    ll = np.array([[math.log(0.5), 0.0], [math.log(0.25), -2.0]])
    w = demc.waic_from_loglik(ll)
    lppd = [math.log(3 / 8), math.log((1 + math.exp(-2)) / 2)]
    pw = [math.log(2) ** 2 / 2, 2.0]
    want = np.array([[lppd[0], pw[0], -1.5 * math.log(2), lppd[0] - pw[0]], [lppd[1], pw[1], -1.0, lppd[1] - pw[1]]])
    np.testing.assert_allclose(w.pointwise, want, rtol=1e-15, atol=1e-16)
    e = want[:, 3]
    assert w.elpd_waic == pytest.approx(e.sum(), rel=1e-15) and w.lppd == pytest.approx(sum(lppd), rel=1e-15)
    assert w.p_waic == pytest.approx(sum(pw), rel=1e-15) and w.waic == pytest.approx(-2 * e.sum(), rel=1e-15)
    assert w.dbar == pytest.approx(-2 * (-1.5 * math.log(2) - 1.0), rel=1e-15)
    assert w.se_elpd == pytest.approx(math.sqrt(2 * ((e[0] - e.mean()) ** 2 + (e[1] - e.mean()) ** 2) / 1), rel=1e-14)  # sqrt(N var), N - 1 = 1
    assert (w.n_high, w.n_nonfinite) == (1, 0)  # p_waic_1 = 2 > 0.4 > (log 2)^2 / 2 = 0.24
    assert "elpd_waic" in repr(w) and "p_waic > 0.4" in repr(w)


def test_one_draw_and_one_observation(demc):
    w = demc.waic_from_loglik(np.array([[-1.0, -2.0, -3.0]]))  # S = 1
    assert np.array_equal(w.pointwise[:, 0], [-1.0, -2.0, -3.0]) and np.array_equal(w.pointwise[:, 2], [-1.0, -2.0, -3.0])
    assert np.isnan(w.pointwise[:, 1]).all() and np.isnan(w.pointwise[:, 3]).all()
    assert math.isnan(w.p_waic) and math.isnan(w.elpd_waic) and w.lppd == -6.0 and w.n_nonfinite == 3
    w1 = demc.waic_from_loglik(np.array([[-1.0], [-2.0]]))  # N = 1: no spread between observations
    assert math.isnan(w1.se_elpd) and math.isfinite(w1.elpd_waic)


def test_minus_infinity_in_some_draws(demc):
    ll = np.array([[-1.0, -1.0], [-np.inf, -1.5], [-2.0, -0.5]])
    w = demc.waic_from_loglik(ll)
    assert w.pointwise[0, 0] == pytest.approx(math.log((math.exp(-1) + math.exp(-2)) / 3), rel=1e-15)  # finite: two of three draws are
    assert np.isnan(w.pointwise[0, 1:]).all() and np.isfinite(w.pointwise[1]).all()
    assert w.n_nonfinite == 1 and math.isnan(w.elpd_waic) and math.isnan(w.p_waic) and math.isfinite(w.lppd)


def test_minus_infinity_in_every_draw(demc):
    w = demc.waic_from_loglik(np.array([[-np.inf, -1.0], [-np.inf, -1.5]]))
    assert w.pointwise[0, 0] == -np.inf and np.isnan(w.pointwise[0, 1:]).all()
    assert w.lppd == -np.inf and w.n_nonfinite == 1 and math.isnan(w.dbar)


def test_nan_draw(demc):
    w = demc.waic_from_loglik(np.array([[-1.0, -1.0], [np.nan, -1.5], [-np.inf, -1.0]]))
    assert np.isnan(w.pointwise[0]).all() and np.isfinite(w.pointwise[1]).all()
    assert math.isnan(w.lppd) and math.isnan(w.elpd_waic) and w.n_nonfinite == 1 and w.n_high == 0


def test_compare_with_itself_and_with_another(demc):
    rng = np.random.default_rng(3)
    a = demc.waic_from_loglik(rng.normal(-1, 0.3, (50, 20)))
    b = demc.waic_from_loglik(rng.normal(-1.2, 0.3, (50, 20)))
    assert demc.compare_waic(a, a) == dict(elpd_diff=0.0, se_diff=0.0)
    c = demc.compare_waic(a, b)
    d = a.pointwise[:, 3] - b.pointwise[:, 3]
    assert c["elpd_diff"] == pytest.approx(a.elpd_waic - b.elpd_waic, rel=1e-13) and c["se_diff"] == pytest.approx(math.sqrt(20 * d.var(ddof=1)), rel=1e-13)
    assert demc.compare_waic(b.pointwise, a.pointwise)["elpd_diff"] == -c["elpd_diff"]
    with pytest.raises(ValueError):
        demc.compare_waic(a, demc.Waic(a.totals))  # totals alone: no pointwise table
    with pytest.raises(ValueError):
        demc.compare_waic(a.pointwise, b.pointwise[:-1])


def test_gaussian_against_the_direct_form(demc):
    """S = 200 draws, N = 50 observations: the log-mean-exp written directly, in long double"""
    rng = np.random.default_rng(11)
    x = rng.normal(0.3, 1.2, 50)
    mu, sg = rng.normal(0.3, 0.15, 200), np.abs(rng.normal(1.2, 0.1, 200))
    ll = -0.5 * ((x[None, :] - mu[:, None]) / sg[:, None]) ** 2 - np.log(sg)[:, None] - 0.5 * math.log(2 * math.pi)
    w = demc.waic_from_loglik(ll)
    L = ll.astype(np.longdouble)
    lppd = np.log(np.mean(np.exp(L), axis=0))
    pw = L.var(axis=0, ddof=1)
    np.testing.assert_allclose(w.pointwise[:, 0], lppd.astype(np.float64), rtol=1e-14)
    np.testing.assert_allclose(w.pointwise[:, 1], pw.astype(np.float64), rtol=1e-13)
    np.testing.assert_allclose(w.pointwise[:, 2], L.mean(axis=0).astype(np.float64), rtol=1e-14)
    assert w.elpd_waic == pytest.approx(float((lppd - pw).sum()), rel=1e-13) and w.p_waic == pytest.approx(float(pw.sum()), rel=1e-13)
    assert w.se_elpd == pytest.approx(float(np.sqrt(50 * (lppd - pw).var(ddof=1))), rel=1e-12)
    assert 0 < w.p_waic < 50 and w.n_nonfinite == 0


def test_summarize_refuses_an_engine_without_waic(demc):
    """there is no host form of WAIC (the host has no densities): an injected engine without waic() is refused before it runs"""
    class Bare:
        def __init__(self, **cfg):
            self.closed = False

        def close(self):
            self.closed = True

    made = []

    def factory(**cfg):
        made.append(Bare(**cfg))
        return made[-1]

    sp = lambda: [0.1, 1.0]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, prior_loglike=demc.Priors(μ=demc.Normal(0, 10), σ=demc.TruncatedCauchy(0, 1)),
                         loglike=demc.GaussianLikelihood(), data=np.arange(5.0), names=("μ", "σ"))
    de = demc.DE(sample_prior=sp, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=2, Np=4)
    with pytest.raises(demc.DemcError) as e:
        demc.summarize(model, de, 4, waic=True, engine_factory=factory)
    assert e.value.code == demc._ffi.EUNSUPPORTED and "waic" in str(e.value)
    assert len(made) == 1 and made[0].closed  # refused before anything ran, and the engine was released


def test_summarize_asks_before_the_run_what_waic_is_certain_to_refuse(demc):
    """an engine that has waic() but whose handle demc_waic would refuse (an unserved family, MvNormal outside DIRECT mode, a shard) is
    refused by waic_served() once the model is on it and before anything is stepped"""
    log = []

    class Refusing:
        def __init__(self, **cfg):
            pass

        def __getattr__(self, name):  # set_model, set_priors, set_bounds, ...: noted, nothing done
            if name.startswith("__"):
                raise AttributeError(name)
            return lambda *a, **k: log.append(name)

        def waic_served(self):
            log.append("waic_served")
            raise demc.DemcError(demc._ffi.EUNSUPPORTED, "demc_waic: the MvNormal families answer per observation only with loglike_mode = direct")

    sp = lambda: [0.1, 1.0]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, prior_loglike=demc.Priors(μ=demc.Normal(0, 10), σ=demc.TruncatedCauchy(0, 1)),
                         loglike=demc.GaussianLikelihood(), data=np.arange(5.0), names=("μ", "σ"))
    de = demc.DE(sample_prior=sp, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=2, Np=4)
    with pytest.raises(demc.DemcError) as e:
        demc.summarize(model, de, 4, waic=True, engine_factory=Refusing)
    assert e.value.code == demc._ffi.EUNSUPPORTED and "loglike_mode = direct" in str(e.value)
    assert "set_model" in log and log.index("set_model") < log.index("waic_served")
    assert "step" not in log and "set_state" not in log and log[-1] == "close"


def test_waic_served_restates_the_refusals_of_the_call(demc):
    """HipEngine.waic_served on the attributes set_model keeps (no device needed): the families of csrc/demc_pwplan.hpp's pw_family"""
    F = demc.families

    def handle(family, mode=0, n_obs=10, shards=1):
        e = demc.HipEngine.__new__(demc.HipEngine)
        e.cfg = demc._ffi.make_config(n_groups=2, Np=4, D=2, loglike_mode=mode, n_groups_total=2 * shards)
        e.family, e.n_obs, e.h = family, n_obs, None
        return e

    for fam in (F.FAM_GAUSSIAN, F.FAM_BINOMIAL, F.FAM_LNR, F.FAM_LBA):
        for mode in (0, 1, 2):
            handle(fam, mode).waic_served()
    handle(F.FAM_MVN_ISO, 2).waic_served()
    handle(F.FAM_MVN_FULL, 2).waic_served()
    U, E = demc._ffi.EUNSUPPORTED, demc._ffi.EINVAL
    cases = [(handle(F.FAM_MVN_FULL, 0), U, "loglike_mode = direct"), (handle(F.FAM_MVN_ISO, 1), U, "loglike_mode = direct"),
             (handle(F.FAM_HIER_BINOMIAL), U, "no per-observation"), (handle(F.FAM_HIER_GAUSSIAN), U, "no per-observation"),
             (handle(F.FAM_RASTRIGIN), U, "no per-observation"), (handle(None), U, "no per-observation"),
             (handle(F.FAM_LBA, n_obs=0), E, "no observations"), (handle(F.FAM_GAUSSIAN, shards=2), E, "sharded handle")]
    for e, code, word in cases:
        with pytest.raises(demc.DemcError) as err:
            e.waic_served()
        assert err.value.code == code and word in str(err.value), (code, word, str(err.value))
