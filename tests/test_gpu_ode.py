"""ODE-trajectory likelihoods on the GPU (include/demc.h: DEMC_FAM_ODE_LV, DEMC_PRIOR_TRUNCNORMAL; csrc/demc_ode.hpp: k_ode_loglike)
against the numpy restatement of tests/test_ode_host.py and against the same model written as a user's whole-row source.

Bars: log-likelihoods / log-posteriors at rtol 1e-9 (the project's log-posterior bar; the kernel and the restatement share every
operation but the one log of sigma); accept decisions exactly, except where |u - exp(w' - w)| < 1e-7; the registered family and the
whole-row source: the same accept flags, ids and theta bit for bit; same seed, sharded or not: same bits."""
import math

import numpy as np
import pytest

import test_ode_host as O
import test_simlike_host as R

pytestmark = pytest.mark.gpu
INF = np.inf
FAM_ODE_LV, TRUNCNORMAL, LOGNORMAL = 9, 10, 8
# the example's priors and bounds (Examples/Predator_Prey_Example.jl:28-31,45-51; sigma: the registered LogNormal the example uses)
PRIORS = [(1.5, 0.5), (1.2, 0.5), (3.0, 0.5), (1.0, 0.5)]
SIGMA_PRIOR = (0.4, 0.8)
LO, HI = [0.5, 0.0, 1.0, 0.0, 0.0], [2.5, 2.0, 4.0, 2.0, INF]


@pytest.fixture()
def D(demc):
    return demc


@pytest.fixture(scope="module")
def data():
    """the example's data, computed once: [101][2]"""
    Y = O.example_data()
    Y.setflags(write=False)
    return Y


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / max(abs(b), 1e-300)


def rows_in_bounds(rng, n):
    return np.stack([rng.uniform(0.6, 2.4, n), rng.uniform(0.1, 1.9, n), rng.uniform(1.1, 3.9, n), rng.uniform(0.1, 1.9, n),
                     rng.uniform(0.2, 2.0, n)], 1)


def start_rows(rng, n):
    """near the truth, as draws of the example's priors that a run has already pulled in"""
    return np.stack([rng.normal(1.5, 0.1, n), rng.normal(1.0, 0.1, n), rng.normal(3.0, 0.2, n), rng.normal(1.0, 0.1, n),
                     rng.uniform(0.4, 0.9, n)], 1)


def setup(e, Y, substeps=10, dt=0.1, u0=(1.0, 1.0), priors=True, bounds_first=False):
    e.set_model(FAM_ODE_LV, Y, [Y.shape[0], 2], [u0[0], u0[1], dt, substeps])
    pri = lambda: e.set_priors([TRUNCNORMAL] * 4 + [LOGNORMAL], [p[0] for p in PRIORS] + [SIGMA_PRIOR[0]],  # noqa: E731
                               [p[1] for p in PRIORS] + [SIGMA_PRIOR[1]])
    if bounds_first:
        e.set_bounds(LO, HI)
    if priors:
        pri()
    if not bounds_first:
        e.set_bounds(LO, HI)


def log_prior(th, lo=LO, hi=HI):
    lp = sum(O.log_truncnormal(m, s, lo[i], hi[i], th[i]) for i, (m, s) in enumerate(PRIORS))
    z = (math.log(th[4]) - SIGMA_PRIOR[0]) / SIGMA_PRIOR[1]
    return lp + (-0.5 * z * z - math.log(th[4]) - math.log(SIGMA_PRIOR[1]) - 0.5 * O.LOG_2PI)


def in_bounds(th, lo=LO, hi=HI):
    return all(lo[i] <= th[i] <= hi[i] for i in range(5))


# ---- (a) demc_logpost vs the restatement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("T", [1, 2, 101])
def test_logpost_equals_the_restatement(D, data, T, substeps):
    """65 rows (one full wave plus one lane) inside the example's bounds + sigma = 1e-3, sigma = 0 (-Inf), the truth; flat priors
    and open bounds, so that the value is the log-likelihood alone.  T = 1: no step at all, the residual is taken at u0."""
    rng = np.random.default_rng(1000 * T + substeps)
    Y = np.ascontiguousarray(data[:T])
    th = rows_in_bounds(rng, 65)
    th[61] = list(O.TRUTH) + [1e-3]
    th[62] = list(O.TRUTH) + [0.0]
    th[63] = list(O.TRUTH) + [0.5]
    e = D.HipEngine(n_groups=2, Np=6, D=5, seed=3, schedule=2)
    try:
        e.set_model(FAM_ODE_LV, Y, [T, 2], [1.0, 1.0, 0.1, substeps])
        got = e.logpost(th)
    finally:
        e.close()
    want = O.lv_loglike(th, Y, substeps=substeps)
    assert want[62] == -INF and got[62] == -INF and np.isfinite(np.delete(want, 62)).all()
    worst = max(rel(g, w) for g, w in zip(got, want))
    print(f"T={T} substeps={substeps}: max relative difference {worst:.3g}; sigma = 1e-3 row {got[61]!r} vs {want[61]!r}")
    for r in range(65):
        assert rel(got[r], want[r]) <= 1e-9, (r, got[r], want[r])


def test_a_row_that_overflows_is_minus_inf_not_nan(D, data):
    """substeps = 1 at dt = 5: one Runge-Kutta step of five time units; the unstable rows leave the double range within a few
    observations -- restatement and kernel both -Inf -- and the rows that stay finite still agree"""
    Y = np.ascontiguousarray(data[:12])
    th = np.array([[2.5, 0.0, 1.0, 2.0, 0.5], list(O.TRUTH) + [0.5], [0.6, 1.9, 3.9, 0.1, 1.0]])
    e = D.HipEngine(n_groups=1, Np=4, D=5, seed=3, schedule=2)
    try:
        e.set_model(FAM_ODE_LV, Y, [12, 2], [1.0, 1.0, 5.0, 1])
        got = e.logpost(th)
    finally:
        e.close()
    want = O.lv_loglike(th, Y, dt=5.0, substeps=1)
    print("dt = 5, substeps = 1:", got, want)
    assert want[0] == -INF and got[0] == -INF and not np.isnan(got).any()
    for r in range(3):
        assert (got[r] == want[r]) if not np.isfinite(want[r]) else rel(got[r], want[r]) <= 1e-9, (r, got[r], want[r])


# ---- (b) teacher-forced steps ----------------------------------------------------------------------------------------------------
def _migrate(e, it):
    e.migration_pack_dev(it, None)  # NULL: the handle's own staging rows (single shard)
    e.migration_apply_dev(it, None)


def test_teacher_forced_steps(D, data):
    """3 groups x 12, 30 iterations with migrations: every weight against the restatement at 1e-9, every accept decision against
    the one recomputed from the restated weights.  Decisions whose log-ratio sits within 1e-7 of its uniform are excluded and
    counted (at most 1 %); with this seed the restated weights exclude none of the 1080 (smallest |u - ratio| 1.4e-3)."""
    G, Np, seed, n_it, burnin, substeps = 3, 12, 4242, 30, 15, 2
    rng = np.random.default_rng(8)
    cfg = dict(n_groups=G, Np=Np, D=5, n_rows=n_it, seed=seed, burnin=burnin, alpha=0.3, beta=0.15, trace=1, schedule=2)
    e = D.HipEngine(**cfg)
    worst, n_dec, n_skip, n_acc, n_mig, gap = 0.0, 0, 0, 0, 0, INF
    try:
        setup(e, data, substeps=substeps)
        e.set_state(start_rows(rng, G * Np))
        for it in range(1, n_it + 1):
            if e.migration_due(it):
                _migrate(e, it)
                n_mig += 1
            tb, wb, _ = e.get_state()
            e.update(it, 1)
            tr = e.get_trace()
            ta, wa, _ = e.get_state()
            ll = O.lv_loglike(tr["proposal"], data, substeps=substeps)
            for s in range(G * Np):
                prop = tr["proposal"][s]
                want = log_prior(prop) + ll[s] if in_bounds(prop) else -INF
                got = tr["w_prop"][s]
                worst = max(worst, rel(got, want))
                assert rel(got, want) <= 1e-9, (it, s, got, want)
                ua = R.draw_blocks(seed, R.S_PART, 0, it, s, [3])[0]
                u = R.u53(ua[0], ua[1])
                ratio = math.exp(min(want - wb[s] + tr["log_adj"][s], 700.0)) if want > -INF else 0.0
                n_dec += 1
                gap = min(gap, abs(u - ratio))
                if abs(u - ratio) < 1e-7:
                    n_skip += 1
                else:
                    assert bool(tr["accepted"][s]) == (ratio >= 1.0 or u <= ratio), (it, s, u, ratio)
                if tr["accepted"][s]:
                    n_acc += 1
                    assert np.array_equal(ta[s], prop) and wa[s] == got
                else:
                    assert np.array_equal(ta[s], tb[s]) and wa[s] == wb[s]
        assert "k_ode_loglike<lv> + k_accept_store" in e.last_kernels(), e.last_kernels()
        assert n_mig >= 3 and 0 < n_acc < n_dec
        assert n_skip <= 0.01 * n_dec
    finally:
        e.close()
    print(f"teacher-forced: {n_dec} decisions, {n_acc} accepted, {n_skip} excluded (smallest |u - ratio| {gap:.3g}), {n_mig} migrations, "
          f"max relative difference of w' {worst:.3g}")


# ---- (c) the same model as a user's whole-row source -----------------------------------------------------------------------------
LV_ROW_SRC = r"""
// Examples/Predator_Prey_Example.jl:6-11,56-65 written by a user: lane 0 integrates, in the operation order of csrc/demc_ode.hpp
// (contraction off: the library's own kernels are built that way); the other lanes contribute 0
#pragma clang fp contract(off)
__device__ void lv_rhs(double x, double y, const double* p, double* fx, double* fy) {
    double a = p[1] * y; a = p[0] - a; *fx = a * x;
    double b = p[3] * x; b = b - p[2]; *fy = b * y;
}
__device__ double demc_user_loglike_row(const double* th, int D, const double* Y, const long long* dims, int ndims,
                                        const double* hyper, int nhyper, int lane, int n_lanes) {
    if (lane != 0) return 0.0;
    const int T = (int)dims[0], substeps = (int)hyper[3];
    const double h = hyper[2] / hyper[3], h2 = 0.5 * h, h6 = h / 6.0, sigma = th[4];
    double x = hyper[0], y = hyper[1], ss = 0.0;
    for (int j = 0; j < T; ++j) {
        const double rx = Y[2 * j] - x; const double qx = rx * rx; ss = ss + qx;
        const double ry = Y[2 * j + 1] - y; const double qy = ry * ry; ss = ss + qy;
        if (j + 1 < T)
            for (int s = 0; s < substeps; ++s) {
                double k1x, k1y, k2x, k2y, k3x, k3y, k4x, k4y, v, wx, wy;
                lv_rhs(x, y, th, &k1x, &k1y);
                v = h2 * k1x; wx = x + v; v = h2 * k1y; wy = y + v;
                lv_rhs(wx, wy, th, &k2x, &k2y);
                v = h2 * k2x; wx = x + v; v = h2 * k2y; wy = y + v;
                lv_rhs(wx, wy, th, &k3x, &k3y);
                v = h * k3x; wx = x + v; v = h * k3y; wy = y + v;
                lv_rhs(wx, wy, th, &k4x, &k4y);
                double t = 2.0 * k2x; t = k1x + t; double t3 = 2.0 * k3x; t = t + t3; t = t + k4x; t = h6 * t; x = x + t;
                t = 2.0 * k2y; t = k1y + t; t3 = 2.0 * k3y; t = t + t3; t = t + k4y; t = h6 * t; y = y + t;
            }
    }
    double l = log(sigma); l = 2.0 * l; l = 1.8378770664093454835606594728112 + l; l = (double)T * l;
    double v = sigma * sigma; v = 2.0 * v;
    const double e = ss / v;
    const double ll = (-l) - e;
    const bool bad = !(sigma > 0.0) || !(sigma < INFINITY) || !(ss < INFINITY) || !(ll == ll);
    return bad ? -INFINITY : ll;
}
"""


def test_whole_row_source_makes_the_same_run(D, data):
    """a yardstick independent of numpy: 200 free iterations of the registered family and of the user's source under the same seed
    -- the same accept flags and ids, theta AND the weights bit for bit (the two kernels are compiled separately, the library's with
    contraction off and the source under the same pragma; the log of sigma, the one function call, comes out the same in both)"""
    G, Np, n_it, substeps = 3, 12, 200, 2
    rng = np.random.default_rng(77)
    th0 = start_rows(rng, G * Np)
    cfg = dict(n_groups=G, Np=Np, D=5, n_rows=n_it, seed=90210, burnin=100, alpha=0.1, beta=0.1, schedule=2)
    a, b = D.HipEngine(**cfg), D.HipEngine(**cfg)
    try:
        setup(a, data, substeps=substeps)
        b.set_model_source_row(LV_ROW_SRC, data, [data.shape[0], 2], [1.0, 1.0, 0.1, substeps])
        setup_pri = lambda e: (e.set_priors([TRUNCNORMAL] * 4 + [LOGNORMAL], [p[0] for p in PRIORS] + [SIGMA_PRIOR[0]],  # noqa: E731
                                            [p[1] for p in PRIORS] + [SIGMA_PRIOR[1]]), e.set_bounds(LO, HI))
        setup_pri(b)
        la, lb = a.logpost(th0), b.logpost(th0)
        assert np.array_equal(lb, la)
        for e in (a, b):
            e.set_state(th0)
            e.step(1, n_it)
        assert "k_ode_loglike<lv>" in a.last_kernels() and "k_user_row" in b.last_kernels(), (a.last_kernels(), b.last_kernels())
        ha, hb = a.get_history(0, n_it), b.get_history(0, n_it)
        sa, sb = a.get_state(), b.get_state()
    finally:
        a.close()
        b.close()
    assert np.array_equal(ha[1], hb[1]) and np.array_equal(ha[3], hb[3])        # accept flags, ids
    assert np.array_equal(ha[0], hb[0]) and np.array_equal(sa[0], sb[0]) and np.array_equal(sa[2], sb[2])  # theta: bit for bit
    assert 0.02 < ha[1].mean() < 0.98
    dw = np.abs(hb[2] - ha[2]) / np.abs(ha[2])
    print(f"whole-row source: {ha[1].size} decisions, acceptance {ha[1].mean():.3f}, weights bit-equal: {np.array_equal(ha[2], hb[2])}, "
          f"largest relative difference {dw.max():.3g}")
    assert np.array_equal(hb[2], ha[2]) and np.array_equal(sb[1], sa[1])


# ---- (d) determinism, shards, geometry --------------------------------------------------------------------------------------------
def _run(make, n_it, th0, Y, sharded=False):
    e = make()
    try:
        e.each(lambda s: setup(s, Y, substeps=2)) if sharded else setup(e, Y, substeps=2)
        e.set_state(th0)
        e.step(1, n_it)
        return e.get_history(0, n_it) + e.get_state()
    finally:
        e.close()


def test_same_seed_same_bits_sharded_or_not(D, data):
    G, Np, n_it = 4, 6, 25
    th0 = start_rows(np.random.default_rng(44), G * Np)
    cfg = dict(n_groups=G, Np=Np, D=5, n_rows=n_it, seed=31338, burnin=10, alpha=0.3, beta=0.1)
    ref = _run(lambda: D.HipEngine(**cfg), n_it, th0, data)
    assert np.isfinite(ref[2]).all() and ref[1].sum() > 0
    for name, out in (("again", _run(lambda: D.HipEngine(**cfg), n_it, th0, data)),
                      ("geometry_groups", _run(lambda: D.HipEngine(geometry_groups=64, **cfg), n_it, th0, data)),
                      ("two shards", _run(lambda: D.MultiEngine(2, device_ids=[0, 0], **cfg), n_it, th0, data, sharded=True))):
        for x, y in zip(ref, out):
            assert np.array_equal(x, y), name


# ---- (e) the truncated Normal on the device ---------------------------------------------------------------------------------------
def test_truncated_normal_prior_on_the_device(D, data):
    """lp of a step = the restated truncated-Normal priors + likelihood at 1e-9, with the example's four priors and bounds, whichever
    of priors and bounds came first (the same bits); narrower bounds set AFTER the priors move lp by the restated change of the
    normalisers -- to a few roundings of lp itself, which is all a difference of two stored doubles can show"""
    G, Np, substeps = 2, 6, 2
    rng = np.random.default_rng(5)
    th0 = start_rows(rng, G * Np)
    cfg = dict(n_groups=G, Np=Np, D=5, n_rows=4, seed=11, burnin=2, trace=1, schedule=2)
    e, f = D.HipEngine(**cfg), D.HipEngine(**cfg)
    try:
        setup(e, data, substeps=substeps)                       # priors, then bounds
        setup(f, data, substeps=substeps, bounds_first=True)    # bounds, then priors
        for h in (e, f):
            h.set_state(th0)
            h.step(1, 1)
        tr, trf = e.get_trace(), f.get_trace()
        assert np.array_equal(tr["w_prop"], trf["w_prop"]) and np.array_equal(tr["accepted"], trf["accepted"])
        ll = O.lv_loglike(tr["proposal"], data, substeps=substeps)
        n_in = 0
        for s in range(G * Np):
            prop = tr["proposal"][s]
            want = log_prior(prop) + ll[s] if in_bounds(prop) else -INF
            n_in += in_bounds(prop)
            assert rel(tr["w_prop"][s], want) <= 1e-9, (s, tr["w_prop"][s], want)
        assert n_in >= G * Np // 2
        # the normaliser follows the bounds
        lp_wide = e.logpost(th0)
        lo2, hi2 = [1.0, 0.5, 2.0, 0.5, 0.0], [2.0, 1.5, 4.0, 1.5, INF]
        e.set_bounds(lo2, hi2)
        lp_narrow = e.logpost(th0)
        delta = sum(O.truncnormal_log_mass_erf(m, s, LO[i], HI[i]) - O.truncnormal_log_mass_erf(m, s, lo2[i], hi2[i]) for i, (m, s) in enumerate(PRIORS))
        assert delta > 0.1
        n_cmp = 0
        for s in range(G * Np):
            if in_bounds(th0[s], lo2, hi2):
                n_cmp += 1
                assert rel(lp_narrow[s], log_prior(th0[s], lo2, hi2) + O.lv_loglike([th0[s]], data, substeps=substeps)[0]) <= 1e-9
                assert abs((lp_narrow[s] - lp_wide[s]) - delta) <= 8 * np.spacing(abs(lp_wide[s])), (s, lp_narrow[s] - lp_wide[s], delta)
            else:
                assert lp_narrow[s] == -INF
        assert n_cmp >= 3
        # refusals: empty bounds, no mass between them; the table stays as it was
        for lo_bad, hi_bad in (([2.5] + lo2[1:], [2.5] + hi2[1:]), ([60.0] + lo2[1:], [61.0] + hi2[1:])):
            with pytest.raises(D.DemcError) as err:
                e.set_bounds(lo_bad, hi_bad)
            assert err.value.code == D._ffi.EINVAL and "DEMC_PRIOR_TRUNCNORMAL" in str(err.value) and "scalar 0" in str(err.value)
        assert np.array_equal(e.logpost(th0), lp_narrow)
        with pytest.raises(D.DemcError) as err:
            e.set_priors([TRUNCNORMAL] + [0] * 4, [100.0] + [0.0] * 4, [0.5] + [1.0] * 4)
        assert err.value.code == D._ffi.EINVAL and "mass" in str(err.value)
        assert np.array_equal(e.logpost(th0), lp_narrow)
    finally:
        e.close()
        f.close()


# ---- refusals of demc_set_model ---------------------------------------------------------------------------------------------------
def test_refusals(D, data):
    Y = np.ascontiguousarray(data[:5])
    ok = dict(family=FAM_ODE_LV, data=Y, dims=[5, 2], hyper=[1.0, 1.0, 0.1, 4])
    bad_Y = Y.copy()
    bad_Y[2, 1] = np.nan
    e, e4 = D.HipEngine(n_groups=1, Np=4, D=5, seed=1), D.HipEngine(n_groups=1, Np=4, D=4, seed=1)
    try:
        with pytest.raises(D.DemcError) as err:
            e4.set_model(**ok)
        assert err.value.code == D._ffi.EINVAL and "D = 5" in str(err.value)
        for kw, text in ((dict(ok, data=np.zeros(15), dims=[5, 3]), "dims[1]"),
                         (dict(ok, dims=[0, 2]), "T = dims[0]"),
                         (dict(ok, data=np.zeros(2 * 4097), dims=[4097, 2]), "T = dims[0]"),
                         (dict(ok, hyper=[1.0, 1.0, 0.1, 0]), "substeps"),
                         (dict(ok, hyper=[1.0, 1.0, 0.1, 2.5]), "substeps"),
                         (dict(ok, hyper=[1.0, 1.0, 0.1, 1025]), "substeps"),
                         (dict(ok, hyper=[1.0, 1.0, 0.0, 4]), "dt"),
                         (dict(ok, hyper=[1.0, 1.0, -0.1, 4]), "dt"),
                         (dict(ok, hyper=[1.0, 1.0, INF, 4]), "dt"),
                         (dict(ok, hyper=[1.0, np.nan, 0.1, 4]), "u0"),
                         (dict(ok, hyper=[INF, 1.0, 0.1, 4]), "u0"),
                         (dict(ok, hyper=[1.0, 1.0, 0.1]), "hyper"),
                         (dict(ok, data=bad_Y), "data value 5")):
            with pytest.raises(D.DemcError) as err:
                e.set_model(**kw)
            assert err.value.code == D._ffi.EINVAL and text in str(err.value), (text, str(err.value))
            with pytest.raises(D.DemcError):  # the handle is left without a model, not with half of one
                e.logpost(np.zeros((1, 5)))
        e.set_model(FAM_ODE_LV, np.zeros((4096, 2)), [4096, 2], [1.0, 1.0, 0.01, 1])  # the cap itself is accepted, and runs
        assert np.isfinite(e.logpost(np.array([list(O.TRUTH) + [1.0]]))[0])
    finally:
        e.close()
        e4.close()


# ---- (f) the example's run -------------------------------------------------------------------------------------------------------
def test_the_example_runs(D, data):
    """Examples/Predator_Prey_Example.jl's settings (Np = 12, n_groups = 3, burnin = 1000, 3000 iterations, truth (1.5, 1, 3, 1),
    noise 0.5) under a fixed seed: acceptance strictly between 0 and 1, finite means; mean, sd and truth per parameter are printed
    for DESIGN.md 5.4.  No recovery tolerance: there is no closed-form posterior to measure against, and the tests above carry the
    precision."""
    rng = np.random.default_rng(68541)

    def tn(mu, sd, lo, hi):
        while True:
            v = rng.normal(mu, sd)
            if lo <= v <= hi:
                return v

    prior = lambda: [tn(1.5, 0.5, 0.5, 2.5), tn(1.2, 0.5, 0.0, 2.0), tn(3.0, 0.5, 1.0, 4.0), tn(1.0, 0.5, 0.0, 2.0),  # noqa: E731
                     float(rng.lognormal(*SIGMA_PRIOR))]
    model = D.DEModel(sample_prior=prior, names=("α", "β", "γ", "δ", "σ"), data=data.T, loglike=D.LotkaVolterraLikelihood(),
                      prior_loglike=D.Priors(α=D.TruncatedNormal(1.5, 0.5), β=D.TruncatedNormal(1.2, 0.5), γ=D.TruncatedNormal(3.0, 0.5),
                                             δ=D.TruncatedNormal(1.0, 0.5), σ=D.LogNormal(*SIGMA_PRIOR)))
    de = D.DE(sample_prior=prior, bounds=tuple(zip(LO, HI)), burnin=1000, Np=12, n_groups=3)
    chains = D.sample(model, de, D.HIPBackend(seed=2026), 3000)
    acc = float(np.mean(chains["acceptance"]))
    desc = chains.describe()
    print(f"predator-prey: acceptance rate {acc:.4f}")
    for nm, truth in zip(("α", "β", "γ", "δ", "σ"), list(O.TRUTH) + [0.5]):
        print(f"predator-prey {nm}: mean {desc[nm]['mean']:.4f} sd {desc[nm]['std']:.4f} truth {truth}")
        assert math.isfinite(desc[nm]["mean"])
    assert 0.0 < acc < 1.0
