"""demc_bridge (include/demc_bridge.h, csrc/demc_bridge.{hpp,cpp}; the definition is DESIGN.md 5.10) on the GPU.  Engines are filled by
set_history_rows; nothing is stepped unless a test says so.

1. stage by stage with diagnostics=True, each stage against the numpy twin fed with the device's own previous stage: the fit, the draws,
   the two evaluations (against eng.logpost), the iteration; everything at loo_cases.BAR = 1e-9 of max(1, |ref|), the -Inf pattern and the
   counts exactly, n_iter within one.
2. the closed forms, 3. repeatability and side effects, 4. the refusals, summarize(..., bridge=True), compare_bridge.
5. the same stage-by-stage check past one workgroup of every kernel: each case first asserts, through bridge_cases.geometry (held to the
   planner by tests/test_bridge_host.py), the plan numbers it is there for.
6. the iteration where it is slow, at its limit, where an iterate is not a positive finite number, and where the logs are not finite:
   the split windows of bridge_cases.WINDOWS, each meeting its condition again on the device's own logs."""
import ctypes as C
import math

import numpy as np
import pytest

import bridge_cases as BC
import test_gpu_pointwise as TP
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu
BAR = BC.BAR


def check_stages(demc, eng, prob, row0, row1, label, n_prop=0, seed=11, keep=None):
    """every stage of the call against its twin -> (out, prop, post, (m, L)); keep: a dict that receives got and ref (the device's record
    and the twin's on the device's own logs), trace (the twin's iterates, as bridge_from_logs gives them) and worst (bars per stage)"""
    D, P = eng.D, eng.P
    lo, hi = np.asarray(prob["lo"], dtype=np.float64), np.asarray(prob["hi"], dtype=np.float64)
    out, prop, post, (m, L) = eng.bridge(row0, row1, n_prop, seed, diagnostics=True)
    rows = eng.get_history(row0, row1)[0]  # [R][P][D] by slot: the order of post_out
    R = row1 - row0
    rmid = R // 2
    fit, est = rows[:rmid].reshape(-1, D), rows[rmid:].reshape(-1, D)
    N1 = est.shape[0]
    N2 = n_prop or N1
    assert prop.shape == (N2, D + 3) and post.shape == (N1, 3) and (out[5], out[6], out[7]) == (fit.shape[0], N1, N2), label
    worst = {}
    # the fit
    m_ref, L_ref = demc.bridge_fit(demc.bridge_transform(fit, lo, hi)[0])
    worst["m"], worst["L"] = BC.err_in_bars(m, m_ref), BC.err_in_bars(L, L_ref)
    assert (np.triu(L, 1) == 0).all()
    # the draws, from the device's own m and L
    th2, lj2, lg2 = demc.bridge_draws(m, L, N2, seed, lo, hi)
    worst["theta"], worst["logJ2"], worst["logg2"] = BC.err_in_bars(prop[:, :D], th2), BC.err_in_bars(prop[:, D + 1], lj2), BC.err_in_bars(prop[:, D + 2], lg2)
    # the two evaluations, on the device's own rows
    lp2 = eng.logpost(prop[:, :D])
    assert np.array_equal(np.isneginf(prop[:, D]), np.isneginf(lp2)), label
    worst["lp2"] = BC.err_in_bars(prop[:, D], lp2)
    lp1 = eng.logpost(est)
    assert np.array_equal(np.isneginf(post[:, 0]), np.isneginf(lp1)), label
    worst["lp1"] = BC.err_in_bars(post[:, 0], lp1)
    xi1, lj1 = demc.bridge_transform(est, lo, hi)
    worst["logJ1"], worst["logg1"] = BC.err_in_bars(post[:, 1], lj1), BC.err_in_bars(post[:, 2], demc.chains.bridge_logg(xi1, m, L))
    # the iteration and the error terms, from the device's own logs
    l1 = (post[:, 0] + post[:, 1]) - post[:, 2]
    l2 = (prop[:, D] + prop[:, D + 1]) - prop[:, D + 2]
    trace = []
    ref = demc.bridge_from_logs(l1, l2, n_fit=fit.shape[0], lp2=prop[:, D], trace=trace)
    got = demc.Bridge(out)
    if keep is not None:
        keep.update(got=got, ref=ref, trace=trace, worst=worst)
    for name in ("logml", "re2_prop", "re2_post_iid"):
        worst[name] = BC.err_in_bars(np.array([getattr(got, name)]), np.array([getattr(ref, name)]))
    assert math.isnan(got.rel_change) == math.isnan(ref.rel_change), (label, got.rel_change, ref.rel_change)
    assert got.l_star == ref.l_star or (math.isnan(got.l_star) and math.isnan(ref.l_star)), (label, got.l_star, ref.l_star)
    assert (got.n_zero_prop, got.n_nonfinite, got.converged) == (ref.n_zero_prop, ref.n_nonfinite, ref.converged), label
    assert abs(got.n_iter - ref.n_iter) <= 1, (label, got.n_iter, ref.n_iter)
    if got.converged:
        assert got.rel_change <= 1e-10
    print(f"{label}: N_fit={fit.shape[0]} N1={N1} N2={N2} D={D} logml={got.logml:.6f} iterations={int(got.n_iter)}; in units of the bar: " +
          " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (label, worst)
    return out, prop, post, (m, L)


def posterior_like(rng, prob, n, P, spread=0.05):
    """rows around a point inside the bounds: close enough together for a proposal that covers them, all strictly inside"""
    centre = np.median(prob["init"](101), axis=0)
    return centre + spread * np.abs(centre).clip(0.1) * rng.normal(0, 1, (n, P, prob["D"]))


CASES = {
    "binomial D=1, both bounds": ("binomial", dict(N=5), 6, 13, {}, None),
    "gaussian D=2, none and lower": ("gaussian", dict(N=50), 6, 13, {}, None),
    "gaussian, mu bounded above only": ("gaussian", dict(N=50), 6, 13, {}, dict(hi=[6.0, np.inf])),
    "lba D=6, two groups": ("lba", dict(N=60), 6, 13, dict(n_groups=2), None),
    "mvn_full d=3 direct": ("mvn_full", dict(N=30, d=3), 6, 13, dict(loglike_mode=2), None),
    "mvn_full d=3 default": ("mvn_full", dict(N=30, d=3), 6, 13, {}, None),
    "mvn_full d=8 direct": ("mvn_full", dict(N=30, d=8), 4, 13, dict(loglike_mode=2), None),
    "mvn_full d=8 default": ("mvn_full", dict(N=30, d=8), 4, 13, {}, None),
    "hier_gaussian S=3 (demc_loo refuses it)": ("hier_gaussian", dict(S=3, n=7), 6, 13, {}, None),
    "Np=3, R=2, N_fit = D + 1": ("gaussian", dict(N=50), 2, 3, {}, None),
    "binomial Np=3, R=3 (odd)": ("binomial", dict(N=5), 3, 3, {}, None),
}


# ---- 1. stage by stage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_stage_by_stage(demc, case):
    family, kw, n, P, ekw, patch = CASES[case]
    rng = np.random.default_rng(31000 + len(case))
    prob = make_problem(family, rng, **kw)
    if patch:
        prob.update(patch)
    G = ekw.get("n_groups", 1)
    eng, _ = TP.engine(demc, prob, n, P, rows=posterior_like(rng, prob, n, G * P), **ekw)
    check_stages(demc, eng, prob, 0, n, case)
    eng.close()


def test_padded_cells_and_a_window_that_starts_late(demc):
    """LNR D = 3 with partners from the history: cells 4 doubles apart; the window starts behind three initial rows"""
    from test_quantile_host import hist_ld
    assert hist_ld(3, True) == 4
    rng = np.random.default_rng(31100)
    prob = make_problem("lnr", rng, N=65, na=2)
    n, P = 6, 13
    eng, _ = TP.engine(demc, prob, n, P, rows=posterior_like(rng, prob, n, P), n_initial=3, partner_kind=1)
    eng.set_history_rows(0, np.stack([prob["init"](P) for _ in range(3)]))
    a = check_stages(demc, eng, prob, 3, 3 + n, "lnr padded cells, rows 3..9")
    b = check_stages(demc, eng, prob, 4, 9, "lnr padded cells, rows 4..9 (R = 5)")
    assert a[0][0] != b[0][0] and b[0][5] == 2 * P and b[0][6] == 3 * P
    eng.close()


@pytest.mark.parametrize("which", ["one", "P-1", "P+1", "zero"])
def test_proposal_counts(demc, which):
    rng = np.random.default_rng(31200)
    prob = make_problem("gaussian", rng, N=50)
    n, P = 6, 13
    n_prop = {"one": 1, "P-1": P - 1, "P+1": P + 1, "zero": 0}[which]
    eng, _ = TP.engine(demc, prob, n, P, rows=posterior_like(rng, prob, n, P))
    out = check_stages(demc, eng, prob, 0, n, f"n_prop = {which}", n_prop=n_prop)[0]
    assert out[7] == (n_prop or 3 * P)
    if n_prop == 1:
        assert math.isnan(out[1]) and math.isfinite(out[0])  # the variance of one draw
    eng.close()


def test_a_proposal_draw_outside_the_support_counts_and_contributes_zero(demc):
    """LNR: tau is bounded by the data's fastest time only through the likelihood once the upper bound is lifted, so some proposal draws
    have lp = -Inf"""
    rng = np.random.default_rng(31300)
    prob = make_problem("lnr", rng, N=65, na=2)
    rt_min = float(np.asarray(prob["data"][65:]).min())
    prob["hi"] = [np.inf] * 3
    prob["pk"], prob["pa"], prob["pb"] = [1, 1, 1], [0, 0, 0.0], [3, 3, 3.0]  # (a prior that does not end at the fastest time either)
    n, P = 6, 13
    rows = posterior_like(rng, prob, n, P)
    rows[..., 2] = rt_min * rng.uniform(0.55, 0.99, (n, P))
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    out = check_stages(demc, eng, prob, 0, n, "lnr, tau above the fastest time in some proposal draws", n_prop=200)[0]
    assert 0 < out[9] < 200 and out[10] == 0 and math.isfinite(out[0])
    eng.close()


# ---- 2. closed forms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["binomial", "mvn_full"])
def test_closed_forms(demc, family):
    prob, exact, rows, _ = BC.closed_problem(family)
    eng, _ = TP.engine(demc, prob, BC.CLOSED_ROWS, BC.CLOSED_P, rows=rows)
    b = demc.Bridge(eng.bridge(0, BC.CLOSED_ROWS, 0, 5))
    print(f"{family}: logml {b.logml:.6f} exact {exact:.6f} difference {b.logml - exact:.2e} = {abs(b.logml - exact) / b.se(1.0):.2f} se (se {b.se(1.0):.2e}), "
          f"{int(b.n_iter)} iterations")
    assert b.converged and b.n_nonfinite == 0 and b.n1 == 1024 and b.n2 == 1024 and b.n_fit == 1024
    assert abs(b.logml - exact) <= 5 * b.se(1.0)
    eng.close()


# ---- 3. repeatability and side effects ------------------------------------------------------------------------------------------------
def test_equal_bits_seeds_and_unchanged_state(demc):
    rng = np.random.default_rng(31400)
    prob = make_problem("gaussian", rng, N=50)
    n, P = 8, 16
    rows = posterior_like(rng, prob, n, P)

    def fresh():
        eng, _ = TP.engine(demc, prob, n + 3, P, rows=np.concatenate([rows, rows[:3]]))
        eng.set_state(rows[-1])
        return eng

    eng = fresh()
    before = (eng.get_history(0, n), eng.get_state())
    a = eng.bridge(0, n, 0, 3, diagnostics=True)
    b = eng.bridge(0, n, 0, 3, diagnostics=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()  # no floating-point atomics
    assert eng.bridge(0, n, 0, 3).tobytes() == a[0].tobytes()
    c = eng.bridge(0, n, 0, 4, diagnostics=True)
    assert c[1].tobytes() != a[1].tobytes() and c[2].tobytes() == a[2].tobytes() and c[3][1].tobytes() == a[3][1].tobytes()
    assert abs(c[0][0] - a[0][0]) < 1.0 and c[0][0] != a[0][0]
    after = (eng.get_history(0, n), eng.get_state())
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert x.tobytes() == y.tobytes()  # history, acceptance, lp, ids, state, weights
    eng.step(n + 1, 3)  # rows n .. n + 2 are written by three steps that follow the calls
    with_calls = (eng.get_history(0, n + 3), eng.get_state())
    eng.close()
    other = fresh()
    other.step(n + 1, 3)
    without = (other.get_history(0, n + 3), other.get_state())
    other.close()
    for x, y in zip(with_calls[0] + with_calls[1], without[0] + without[1]):
        assert x.tobytes() == y.tobytes()


# ---- 4. refusals, summarize, compare ----------------------------------------------------------------------------------------------------
def test_refusals(demc):
    E, U = demc._ffi.EINVAL, demc._ffi.EUNSUPPORTED
    rng = np.random.default_rng(6)
    prob = make_problem("gaussian", rng, N=20)
    eng, rows = TP.engine(demc, prob, 6, 4, rows=posterior_like(rng, prob, 6, 4))
    dp = C.POINTER(C.c_double)
    buf = np.empty(12)
    for r0, r1 in ((-1, 3), (2, 2), (2, 3), (3, 2), (0, 7)):
        TP._refused(demc, lambda: eng.bridge(r0, r1), E, "bad rows: demc_bridge needs at least two rows of the history")
    assert eng.L.demc_bridge(eng.h, 0, 6, 0, 0, None, None, None, None) == E
    assert eng.L.demc_last_error(eng.h).decode() == "demc_bridge: out is NULL"
    assert eng.L.demc_bridge(eng.h, 0, 7, 0, 0, None, None, None, None) == E  # ... and the rows rank before the output
    assert eng.L.demc_last_error(eng.h).decode() == "bad rows: demc_bridge needs at least two rows of the history"
    assert eng.L.demc_bridge(None, 0, 6, 0, 0, buf.ctypes.data_as(dp), None, None, None) == E
    TP._refused(demc, lambda: eng.bridge(0, 6, n_prop=-1), E, "demc_bridge: n_prop must be >= 0")
    TP._refused(demc, lambda: eng.bridge(0, 6, n_prop=(1 << 22) + 1), E, "demc_bridge: N1 = 12 and N2 = 4194305 draws: one is above the cap of 4194304")
    bad = rows.copy()
    bad[1, 2, 1] = 0.0   # sigma on its lower bound, in the fit half
    bad[4, 3, 1] = -1.0  # ... and outside it, in the estimate half
    bad[5, 0, 0] = np.nan
    eng.set_history_rows(0, bad)
    TP._refused(demc, lambda: eng.bridge(0, 6), E, "demc_bridge: 3 scalar(s) of the window lie on or outside a finite bound or are NaN (the first: row 1, slot 2, scalar 1)")
    TP._refused(demc, lambda: eng.bridge(2, 6), E, "demc_bridge: 2 scalar(s)", "(the first: row 4, slot 3, scalar 1)")
    const = rows.copy()
    const[:3, :, 0] = 0.25  # mu constant over the fit half: the first pivot is 0
    eng.set_history_rows(0, const)
    TP._refused(demc, lambda: eng.bridge(0, 6), E, "demc_bridge: the covariance of the fit half is not positive definite (pivot 0 of 2 is not positive)")
    eng.close()
    bare = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=0, store_history=0)
    setup_engine(bare, prob)
    TP._refused(demc, lambda: bare.bridge(0, 2), E, "history is not stored on this handle")
    bare.close()
    nomodel = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4)
    TP._refused(demc, lambda: nomodel.bridge(0, 4), E, "demc_bridge: no model is set on this handle")
    TP._refused(demc, nomodel.bridge_served, E, "demc_bridge: no model is set on this handle")
    nomodel.close()
    shard = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4, n_groups_total=2, group_offset=1)
    setup_engine(shard, prob)
    TP._refused(demc, lambda: shard.bridge(0, 4), E, "sharded handle: demc_bridge reads the whole history of one handle")
    TP._refused(demc, shard.bridge_served, E, "demc_bridge: sharded handle")
    shard.close()
    sim = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4)
    sim.set_model_sim(0, 0, 64, rng.normal(0, 1, 10), [0.0])
    TP._refused(demc, lambda: sim.bridge(0, 4), U, "demc_bridge: a simulation likelihood (demc_set_model_sim) gives a noisy log posterior")
    TP._refused(demc, sim.bridge_served, U, "demc_bridge: a simulation likelihood")
    sim.close()
    from demc_amd import families as F
    wide = demc.HipEngine(n_groups=1, Np=4, D=65, n_rows=4)
    wide.set_model(F.FAM_RASTRIGIN, None, [])
    TP._refused(demc, lambda: wide.bridge(0, 4), E, "demc_bridge: D = 65 is above the cap of 64 (DEMC_BRIDGE_MAX_D")
    TP._refused(demc, wide.bridge_served, E, "demc_bridge: D = 65 is above the cap of 64")
    wide.close()
    p8 = make_problem("mvn_full", rng, N=10, d=8)
    few, _ = TP.engine(demc, p8, 4, 4)
    TP._refused(demc, lambda: few.bridge(0, 4), E, "demc_bridge: the fit half holds N_fit = 8 draws, the covariance of the proposal needs more than D = 8")
    few.close()


def _binomial_model(demc, rng, prior):
    n_trials = np.array([12.0, 9.0, 15.0, 11.0, 8.0])
    k = np.array([9.0, 7.0, 12.0, 8.0, 7.0])
    sp = lambda: [rng.uniform(0.05, 0.95)]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, names=("θ",), data=dict(N=n_trials, k=k), prior_loglike=demc.Priors(θ=prior), loglike=demc.BinomialLikelihood())
    de = demc.DE(sample_prior=sp, bounds=((0.0, 1.0),), burnin=200, Np=8, n_groups=2)
    lbeta = lambda p, q: math.lgamma(p) + math.lgamma(q) - math.lgamma(p + q)  # noqa: E731
    lc = sum(math.lgamma(a + 1) - math.lgamma(b + 1) - math.lgamma(a - b + 1) for a, b in zip(n_trials, k))
    return model, de, lambda a, b: lc + lbeta(a + k.sum(), b + (n_trials - k).sum()) - lbeta(a, b)


def test_summarize_with_bridge_and_compare(demc):
    rng = np.random.default_rng(50515)
    kept = {}

    class Keeping(demc.HipEngine):  # the same engine, remembering what the call answered for the kept rows
        def bridge(self, row0, row1, n_prop=0, seed=0, diagnostics=False):
            kept["args"] = (row0, row1, n_prop, seed)
            kept["direct"] = demc.HipEngine.bridge(self, row0, row1, n_prop, seed)
            return demc.HipEngine.bridge(self, row0, row1, n_prop, seed, diagnostics)

    fits, exact = {}, {}
    for name, (a, b) in (("flat", (1.0, 1.0)), ("sceptical", (2.0, 8.0))):
        model, de, closed = _binomial_model(demc, rng, demc.Beta(a, b))
        fits[name] = demc.summarize(model, de, demc.HIPBackend(seed=2), 1200, bridge=dict(n_prop=4000, seed=9), engine_factory=Keeping)
        exact[name] = closed(a, b)
        br = fits[name].bridge
        assert kept["args"] == (200, 1200, 4000, 9) and br.out.tobytes() == kept["direct"].tobytes()
        assert br.converged and br.n2 == 4000 and br.n1 == 500 * 16 and br.rho >= 1.0
        print(f"{name}: {br}, exact {exact[name]:.4f}, rho {br.rho:.2f}")
        assert abs(br.logml - exact[name]) <= 5 * br.se(br.rho)
    cmp = demc.compare_bridge(fits["flat"].bridge, fits["sceptical"].bridge)
    want = exact["flat"] - exact["sceptical"]
    assert abs(cmp["log_bf"] - want) <= 5 * cmp["se"] and cmp["log_bf"] > 0 and abs(cmp["prob_a"] + cmp["prob_b"] - 1) < 1e-15
    assert abs(cmp["prob_a"] - 1 / (1 + math.exp(-cmp["log_bf"]))) < 1e-12
    model, de, _ = _binomial_model(demc, rng, demc.Beta(1.0, 1.0))
    assert demc.summarize(model, de, demc.HIPBackend(seed=2), 300).bridge is None
    assert demc.summarize(model, de, demc.HIPBackend(seed=2), 300, bridge=True).bridge.n2 == 100 * 16 - 50 * 16


# ---- 5. past one workgroup: every case first asserts, through bridge_cases.geometry, the path it is there for -----------------------------
def _gaussian_engine(demc, seed, n, P):
    rng = np.random.default_rng(seed)
    prob = make_problem("gaussian", rng, N=50)
    eng, _ = TP.engine(demc, prob, n, P, rows=BC.spread_rows(rng, prob, n, P))
    return eng, prob


@pytest.mark.parametrize("n_prop", [0, 2049, 257])
def test_two_reduction_workgroups(demc, n_prop):
    """N_fit = N1 = 1040: two workgroups of k_bridge_part on the posterior side, and on the proposal side two (n_prop = 0), three with one
    element in the ninth workgroup of k_bridge_logs / k_bridge_exp (2049), or one with the grid sized by N1 (257); seventeen blocks of the
    solve; three chunks of the covariance"""
    R, P = BC.WIN_R, BC.WIN_P
    label = f"two reduction workgroups, n_prop = {n_prop}"
    want = {0: dict(N2=1040, W2=2, logs_blocks=5), 2049: dict(N2=2049, W2=3, logs_blocks=9), 257: dict(N2=257, W2=1, logs_blocks=5)}[n_prop]
    g = BC.asserted_geometry(label, R, P, 2, n_prop, n_fit=1040, N1=1040, W1=2, solve_blocks=17, cov_chunks=3, **want)
    if n_prop == 2049:
        assert g["N2"] - (g["logs_blocks"] - 1) * BC.BRIDGE_WG == 1
    if n_prop == 257:
        assert g["logs_blocks"] == -(-g["N1"] // BC.BRIDGE_WG) > -(-g["N2"] // BC.BRIDGE_WG)
    eng, prob = _gaussian_engine(demc, 32000, R, P)
    out = check_stages(demc, eng, prob, 0, R, label, n_prop=n_prop)[0]
    assert out[4] == 1 and (out[5], out[6], out[7]) == (1040, 1040, g["N2"])
    eng.close()


@pytest.mark.parametrize("n_prop", [63, 64, 65, 128])
def test_draw_blocks_and_padding(demc, n_prop):
    """N2 against pad2 and the 64 lanes of a block of k_bridge_draw: at N2 = 64 the second block holds the one padding row only"""
    R, P = 6, 13
    label = f"draw blocks and padding, n_prop = {n_prop}"
    want = {63: dict(chunks2=5, pad2=65, last2=11, draw_blocks=2), 64: dict(chunks2=5, pad2=65, last2=12, draw_blocks=2),
            65: dict(chunks2=5, pad2=65, last2=13, draw_blocks=2), 128: dict(chunks2=10, pad2=130, last2=11, draw_blocks=3)}[n_prop]
    BC.asserted_geometry(label, R, P, 2, n_prop, N2=n_prop, **want)
    eng, prob = _gaussian_engine(demc, 32100, R, P)
    check_stages(demc, eng, prob, 0, R, label, n_prop=n_prop)
    eng.close()


@pytest.mark.parametrize("R,P", [(64, 16), (54, 19)])
def test_covariance_chunk_edge(demc, R, P):
    """cov_run through the one-cell HistView of the xi buffer at one full chunk of 512 cells and at one cell past it"""
    n_fit = (R // 2) * P
    label = f"covariance chunk edge, N_fit = {n_fit}"
    g = BC.asserted_geometry(label, R, P, 2, 0, n_fit=n_fit, cov_chunks=-(-n_fit // 512), cov_workers=-(-n_fit // 512))
    assert n_fit in (512, 513) and g["cov_chunks"] == n_fit - 511
    eng, prob = _gaussian_engine(demc, 32200 + P, R, P)
    keep = {}
    check_stages(demc, eng, prob, 0, R, label, keep=keep)
    assert keep["worst"]["m"] <= 1.0 and keep["worst"]["L"] <= 1.0
    eng.close()


@pytest.mark.parametrize("D,R", [(63, 2), (63, 8), (64, 2), (64, 8)])
def test_widest_proposal(demc, D, R):
    """D = 63 and 64 (the cap: 32 KB of LDS in the draw and the solve), the four kinds of bounds assigned cyclically, at N_fit = D + 1 --
    the least the plan admits; the estimate half then lies so far out in g that r_1 = 0 and the rule of the stopped iterate applies --
    and at N_fit = 4 (D + 1).  Odd D: block 31 gives z_62 alone, its sine is unused (theta is held to the twin's draws at the bar)."""
    P = D + 1
    label = f"widest proposal, D = {D}, N_fit = {(R // 2) * P}"
    g = BC.asserted_geometry(label, R, P, D, 0, n_fit=(R // 2) * P, lds_bytes=D * 64 * 8, draw_blocks=-(-(R // 2) * P // 64), solve_blocks=-(-(R // 2) * P // 64))
    assert g["lds_bytes"] <= 32768 and (D + 1) // 2 == 32 and g["n_fit"] > D
    prob, centre = BC.wide_problem(D)
    rng = np.random.default_rng(53000 + D + R)
    eng, _ = TP.engine(demc, prob, R, P, rows=centre + 0.05 * rng.normal(0, 1, (R, P, D)))
    keep = {}
    check_stages(demc, eng, prob, 0, R, label, keep=keep)
    got, ref = keep["got"], keep["ref"]
    assert got.n_iter == ref.n_iter or R == 8
    if R == 2:
        assert ref.n_iter == 1 and got.converged == 0 and got.n_nonfinite == 0 and all(math.isnan(v) for v in (got.logml, got.re2_prop, got.re2_post_iid, got.rel_change))
    else:
        assert got.converged == 1
    eng.close()


def test_the_cap_of_the_reduction(demc):
    """N2 = 262 145 = 256 * 256 * 4 + 1: kBridgeMaxW binds and thread 0 of workgroup 0 takes a fifth element; 513 chunks of P = 512"""
    R, P, n_prop = 2, BC.CAP_P, BC.CAP_N2
    label = "the cap of the reduction"
    g = BC.asserted_geometry(label, R, P, 2, n_prop, N2=n_prop, W2=256, W1=1, chunks2=513, pad2=513 * 512, last2=1, n_fit=512, N1=512)
    assert -(-g["N2"] // (g["W2"] * BC.BRIDGE_WG)) == 5 and BC.geometry(R, P, 2, n_prop - 1)["W2"] == 256 and -(-(n_prop - 1) // (256 * BC.BRIDGE_WG)) == 4
    eng, prob = _gaussian_engine(demc, 32300, R, P)
    out = check_stages(demc, eng, prob, 0, R, label, n_prop=n_prop)[0]
    assert out[7] == n_prop and out[4] == 1
    eng.close()


# ---- 6. the iteration where it is slow, where it runs to its limit, where r stops, and where the logs are not finite ------------------------
@pytest.mark.parametrize("name", list(BC.WINDOWS))
def test_iteration_on_split_windows(demc, name):
    """the windows of bridge_cases.WINDOWS, each meeting its condition again on the device's own logs.  slow: converged within one
    iteration of the twin after more than one batch of eight.  iteration limit: 1000 iterations and not converged on both sides; the
    window's sequence is stable (tests/test_bridge_host.py: 40 digits and FP64 end on the same value), so logml and the error terms are
    held to the bar as everywhere.  r stops: r_1 = 0; the outputs follow DESIGN.md 5.10 step 5 field by field."""
    w = BC.WINDOWS[name]
    R, P = w["R"], w["P"]
    prob, rows = BC.split_window(name)
    g = BC.asserted_geometry(name, R, P, 2, w["n_prop"], N1=(R - R // 2) * P, N2=w["n_prop"] or (R - R // 2) * P,
                             **(dict(W1=2, W2=3 if w["n_prop"] else 2) if R == BC.WIN_R else dict(W1=1, W2=1)))
    eng, _ = TP.engine(demc, prob, R, P, rows=rows)
    keep = {}
    out = check_stages(demc, eng, prob, 0, R, name, n_prop=w["n_prop"], seed=BC.WINDOW_DRAW_SEED, keep=keep)[0]
    got, ref, trace = keep["got"], keep["ref"], keep["trace"]
    BC.window_condition(name, ref, trace)
    print(f"{name}: device {int(got.n_iter)} iterations, twin {int(ref.n_iter)}; the twin's last changes {[f'{t[1]:.3g}' for t in trace[-3:]]}")
    if w["kind"] == "slow":
        assert got.converged == 1 and abs(got.n_iter - ref.n_iter) <= 1 and got.n_iter > BC.BRIDGE_BATCH and math.isfinite(got.logml)
    elif w["kind"] == "limit":
        assert got.n_iter == ref.n_iter == 1000 and got.converged == 0 and all(math.isfinite(v) for v in out[[0, 1, 2, 8, 11]]) and got.rel_change > 1e-10
    else:
        assert got.n_iter == ref.n_iter and got.converged == 0 and got.n_nonfinite == 0 and got.l_star == ref.l_star and math.isfinite(got.l_star)
        assert np.isnan(out[[0, 1, 2, 11]]).all() and (out[5], out[6], out[7]) == (g["n_fit"], g["N1"], g["N2"]) and out[9] == ref.n_zero_prop
        same = np.array_equal(np.isnan(out), np.isnan(ref.out)) and np.array_equal(out[~np.isnan(out)], ref.out[~np.isnan(ref.out)])
        assert same, (out, ref.out)  # device and twin agree field by field
    eng.close()


@pytest.mark.parametrize("which", ["a few", "all"])
def test_minus_inf_among_l1(demc, which):
    """LNR with the upper bound of tau lifted (the recipe of the proposal-side test): tau above the data's fastest time in a few draws of
    the estimate half -- their l1 is -Inf, the term 1 / (s2 r), logml finite and at the bar -- then in all of them: no l1 is finite,
    l* = -Inf, no iteration runs, nothing is counted as not finite, and the outputs are NaN"""
    rng = np.random.default_rng(31500)
    prob = make_problem("lnr", rng, N=65, na=2)
    rt_min = float(np.asarray(prob["data"][65:]).min())
    prob["hi"] = [np.inf] * 3
    prob["pk"], prob["pa"], prob["pb"] = [1, 1, 1], [0, 0, 0.0], [3, 3, 3.0]
    n, P = 6, 13
    BC.asserted_geometry(f"-Inf among l1, {which}", n, P, 3, 0, n_fit=39, N1=39, N2=39, W1=1, W2=1)
    rows = posterior_like(rng, prob, n, P)
    rows[..., 2] = rt_min * rng.uniform(0.55, 0.99, (n, P))
    outside = [(3, 0), (4, 7), (5, 12)] if which == "a few" else [(r, s) for r in range(3, 6) for s in range(P)]
    for r, s in outside:
        rows[r, s, 2] = rt_min * rng.uniform(1.01, 1.2)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    keep = {}
    out, prop, post, _ = check_stages(demc, eng, prob, 0, n, f"lnr, tau above the fastest time in {which} of the estimate half", keep=keep)
    got = keep["got"]
    assert np.isneginf(post[:, 0]).sum() == len(outside) and np.isfinite(post[:, 1:]).all() and got.n_nonfinite == 0
    if which == "a few":
        assert math.isfinite(got.logml) and got.converged == 1 and math.isfinite(got.l_star)
    else:
        assert got.l_star == -math.inf and got.n_iter == 0 and got.converged == 0 and np.isnan(out[[0, 1, 2, 11]]).all()
    eng.close()


def test_a_nan_observation_makes_every_log_ratio_nan(demc):
    """demc_set_model takes Gaussian data as it comes: one NaN observation makes every lp NaN, so the rule of DESIGN.md 5.10 step 5 for
    a NaN among l1 or l2 is reachable through the C surface: all N1 + N2 are counted, no iteration runs, l* is NaN (no l1 but NaNs)"""
    rng = np.random.default_rng(31600)
    prob = make_problem("gaussian", rng, N=50)
    prob["data"] = np.array(prob["data"], dtype=np.float64)
    n, P = 6, 13
    rows = BC.spread_rows(rng, prob, n, P)
    prob["data"][7] = np.nan
    BC.asserted_geometry("a NaN observation", n, P, 2, 0, N1=39, N2=39, W1=1, W2=1)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    keep = {}
    out, prop, post, _ = check_stages(demc, eng, prob, 0, n, "gaussian with a NaN observation", keep=keep)
    got = keep["got"]
    assert np.isnan(post[:, 0]).all() and np.isnan(prop[:, 2]).all() and np.isfinite(prop[:, :2]).all()
    assert got.n_nonfinite == 39 + 39 and got.n_iter == 0 and got.converged == 0 and math.isnan(got.l_star) and np.isnan(out[[0, 1, 2, 11]]).all() and got.n_zero_prop == 0
    eng.close()
