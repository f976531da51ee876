"""demc_pointwise_loglik and demc_waic (include/demc_pointwise.h, csrc/demc_pointwise.{hpp,cpp}; the definition is DESIGN.md 5.8) on
the GPU.  Engines are filled by set_history_rows; nothing is stepped unless a test says so.

1. the terms l_is against the CPU oracle evaluated on the one-observation data set {y_i}: |d| <= 1e-9 max(1, |ref|) -- the project's lp
   bar; a single term cannot be worse conditioned than the sums it already holds.  LBA: 1e-5 max(1, |sum_j l_j|) per term, the
   absolute error tests/test_gpu_parity.py:16-23 already grants one tail trial.
2. the statistics against the definition (chains.waic_from_loglik, sums in np.longdouble) applied to pointwise_loglik of the
   exported rows -- the same bits as the kernel's terms, so this isolates the reductions: lppd_i and mean_i at 1e-9 max(1, |ref|),
   p_waic_i at 1e-9 var_ref (any summation order is within about S 2^-53 (var + shift^2): S <= 2^20 and draws with sd_s(l_i) >=
   1e-3 max_s |l_is|, asserted), totals at 1e-9 of sum |terms|, the two counts exactly.
3. end to end without the device's terms: numpy closed forms on the raw data and the exported chains, same bars, |l| / sd <= 1e4
   asserted (a few-ulp difference in log / exp then moves the variance by about 1e-11 relative).
4. the edge rules, 5. the refusals, 6. summarize(..., waic=True).

tests/test_gpu_pointwise_edges.py goes on from here with references no device kernel produced: every <family, X> instance, observation
indices past the first tile, the edges of the plan, badly conditioned columns, and non-finite patterns across chunks."""
import ctypes as C
import math

import numpy as np
import pytest

import test_pwplan_host as PL
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu
BAR = 1e-9
LBA_BAR = 1e-5


def engine(demc, prob, n, P, rows=None, n_groups=1, **kw):
    """n_groups groups of P particles each with n history rows written by set_history_rows (the draws of the prior's init when rows
    is None); a row of the history holds the n_groups P cells of all groups"""
    kw.setdefault("schedule", 1 if P < 4 else 2)
    eng = demc.HipEngine(n_groups=n_groups, Np=P, D=prob["D"], n_rows=n + kw.get("n_initial", 0), seed=1, **kw)
    setup_engine(eng, prob)
    if rows is None:
        rows = np.stack([prob["init"](n_groups * P) for _ in range(n)])
    eng.set_history_rows(kw.get("n_initial", 0), rows)
    return eng, np.asarray(rows, dtype=np.float64).reshape(n, n_groups * P, prob["D"])


def one_observation(prob, i):
    """the model spec of the data set {y_i}"""
    from demc_amd import families as F
    fam, data, N = prob["fam"], np.asarray(prob["data"], dtype=np.float64), prob["dims"][0]
    if fam == F.FAM_GAUSSIAN:
        return data[i:i + 1], [1]
    if fam == F.FAM_BINOMIAL:
        return np.array([data[i], data[N + i]]), [1]
    if fam in (F.FAM_MVN_ISO, F.FAM_MVN_FULL):
        return data.reshape(N, -1)[i:i + 1], [1, prob["dims"][1]]
    raise KeyError(fam)


def oracle_terms(orc, prob, theta):
    """ref[s][i] = log p(y_i | theta_s) by the oracle: orc_lnr_logpdf / orc_lba_logpdf per trial, else orc_loglike of a fresh oracle
    handle that holds observation i alone"""
    from demc_amd import families as F
    theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1, prob["D"])
    N, fam = prob["dims"][0], prob["fam"]
    ref = np.empty((theta.shape[0], N))
    if fam in (F.FAM_LBA, F.FAM_LNR):
        na, L = prob["dims"][1], orc.lib()
        data = np.asarray(prob["data"], dtype=np.float64)
        for s, th in enumerate(theta):
            nu = np.ascontiguousarray(th[:na])
            nup = nu.ctypes.data_as(C.POINTER(C.c_double))
            for i in range(N):
                if fam == F.FAM_LBA:
                    ref[s, i] = L.orc_lba_logpdf(nup, na, th[na], th[na + 1], th[na + 2], int(data[i]), data[N + i])
                else:
                    ref[s, i] = L.orc_lnr_logpdf(nup, na, float(prob["hyper"][0]), th[na], int(data[i]), data[N + i])
        return ref
    for i in range(N):
        o = orc.Oracle(n_groups=1, Np=4, D=prob["D"])
        data, dims = one_observation(prob, i)
        o.set_model(fam, data, dims, prob["hyper"])
        ref[:, i] = o.loglike(theta)
        o.close()
    return ref


def draws_of(value, D):
    """the exported rows [n][D+2][P] as the pool of draws [n P][D]"""
    return np.ascontiguousarray(np.transpose(value[:, :D, :], (0, 2, 1))).reshape(-1, D)


# ---- 1. the terms against the oracle ----------------------------------------------------------------------------------------------
def _check_terms(demc, orc, prob, eng, label):
    from demc_amd import families as F
    N = prob["dims"][0]
    worst = 0.0
    for n in (1, 3, 70):
        theta = prob["init"](n)
        got = eng.pointwise_loglik(theta)
        assert got.shape == (n, N)
        ref = oracle_terms(orc, prob, theta)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin), label
        assert np.array_equal(got[~fin], ref[~fin]), label  # (-Inf where the oracle has -Inf)
        if prob["fam"] == F.FAM_LBA:
            scale = LBA_BAR * np.maximum(1.0, np.abs(np.where(fin, ref, 0.0).sum(axis=1)))[:, None] * np.ones_like(ref)
        else:
            scale = BAR * np.maximum(1.0, np.abs(ref))
        err = np.abs(got - ref)[fin] / scale[fin]
        worst = max(worst, float(err.max()) if err.size else 0.0)
        # the sum over the observations and the prior are demc_logpost
        lp, prior = eng.logpost(theta), None
        o = orc.Oracle(n_groups=1, Np=4, D=prob["D"])
        setup_engine(o, prob)
        prior = o.prior(theta)
        o.close()
        total = got.sum(axis=1) + prior
        ok = np.isfinite(lp)
        assert np.array_equal(np.isfinite(total), ok), label
        rel = LBA_BAR if prob["fam"] == F.FAM_LBA else BAR
        assert (np.abs(total - lp)[ok] <= rel * np.maximum(1.0, np.abs(lp[ok]))).all(), (label, n, np.abs(total - lp)[ok].max())
    print(f"{label}: worst term error {worst:.3g} of its bar")
    assert worst <= 1.0, (label, worst)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("family", ["gaussian", "binomial", "lnr", "lba"])
def test_terms_against_the_oracle(demc, orc, family, N):
    rng = np.random.default_rng(1000 + N)
    prob = make_problem(family, rng, N=N)  # (LBA: the trials arrive unsorted, so a lost permutation cannot pass)
    if family == "lba" and N > 1:
        ch, rt = prob["data"][:N], prob["data"][N:]
        assert not np.array_equal(np.lexsort((rt, ch)), np.arange(N)), "the trials are already in the library's order"
    eng, _ = engine(demc, prob, 1, 4)
    _check_terms(demc, orc, prob, eng, f"{family} N={N}")
    eng.close()


@pytest.mark.parametrize("d", [2, 8, 31])
@pytest.mark.parametrize("family", ["mvn_iso", "mvn_full"])
def test_mvn_terms_against_the_oracle(demc, orc, family, d):
    """DIRECT mode: an observation is a data row; the whitened rows are padded to 8 / 8 / 32 scalars"""
    prob = make_problem(family, np.random.default_rng(2000 + d), N=65, d=d)
    eng, _ = engine(demc, prob, 1, 4, loglike_mode=2)
    _check_terms(demc, orc, prob, eng, f"{family} d={d}")
    eng.close()


# ---- 2. the statistics against the definition -------------------------------------------------------------------------------------
def check_waic(demc, eng, prob, row0, row1, label, ll=None, guard=True):
    """device against chains.waic_from_loglik of the terms of the exported rows -> (totals, pointwise) of the device"""
    D, N = prob["D"], prob["dims"][0]
    if ll is None:
        ll = eng.pointwise_loglik(draws_of(eng.export_chains(row0, row1), D))
    S = ll.shape[0]
    assert S == (row1 - row0) * eng.P and S <= 1 << 20 and ll.shape[1] == N
    ref = demc.waic_from_loglik(ll)
    tot, pt = eng.waic(row0, row1, pointwise=True)
    assert pt.shape == (N, 4) and tot.shape == (8,)
    fin = np.isfinite(ref.pointwise)
    assert np.array_equal(np.isfinite(pt), fin), label
    assert np.array_equal(np.isnan(pt), np.isnan(ref.pointwise)) and np.array_equal(pt[~fin & ~np.isnan(pt)], ref.pointwise[~fin & ~np.isnan(pt)]), label
    var = ref.pointwise[:, 1]
    if guard:  # the conditioning the bars were derived for, and a penalty that is there to be got wrong
        with np.errstate(all="ignore"):
            sd = ll.std(axis=0, ddof=1)
            assert (sd >= 1e-3 * np.abs(ll).max(axis=0)).all(), (label, (sd / np.abs(ll).max(axis=0)).min())
        assert (var > 0).all(), label
    scale = np.stack([np.maximum(1.0, np.abs(ref.pointwise[:, 0])), np.abs(var), np.maximum(1.0, np.abs(ref.pointwise[:, 2])),
                      np.maximum(1.0, np.abs(ref.pointwise[:, 0])) + np.abs(var)], axis=1)
    with np.errstate(all="ignore"):
        err = np.where(fin, np.abs(pt - ref.pointwise) / scale, 0.0)
    worst = err.max(axis=0)
    # totals: relative to the sum of the absolute terms
    p = ref.pointwise
    sums = dict(elpd_waic=np.abs(p[:, 3]).sum(), p_waic=np.abs(p[:, 1]).sum(), lppd=np.abs(p[:, 0]).sum(), waic=2 * np.abs(p[:, 3]).sum(),
                dbar=2 * np.abs(p[:, 2]).sum())
    t_err = {}
    for j, name in enumerate(demc.chains.WAIC_TOTALS):
        want = getattr(ref, name)
        if name in ("n_high", "n_nonfinite"):
            assert tot[j] == want, (label, name, tot[j], want)
        elif not math.isfinite(want):
            assert (math.isnan(want) and math.isnan(tot[j])) or tot[j] == want, (label, name, tot[j], want)
        elif name == "se_elpd":
            t_err[name] = abs(tot[j] - want) / max(want, 1e-300)
        else:
            t_err[name] = abs(tot[j] - want) / sums[name]
    print(f"{label}: S={S} N={N} lppd {worst[0]:.3g} p_waic {worst[1]:.3g} mean {worst[2]:.3g} elpd {worst[3]:.3g}; totals " +
          " ".join(f"{k} {v:.3g}" for k, v in t_err.items()))
    assert (worst <= BAR).all(), (label, worst)
    assert all(v <= BAR for v in t_err.values()), (label, t_err)
    return tot, pt


SHAPES = {  # name: (family, N, n, P, what geometry() must say)
    "S3": ("gaussian", 65, 1, 3, dict(chunks=1, chunk_len=3)),                       # the smallest pool: Np >= 3
    "one_chunk": ("gaussian", 65, 8, 8, dict(chunks=1, chunk_len=64)),
    "one_chunk_plus_1": ("binomial", 40, 13, 5, dict(chunks=2, chunk_len=33, last_chunk=32)),
    "three_chunks_ragged": ("lnr", 130, 10, 13, dict(chunks=3, chunk_len=44, last_chunk=42)),
    "tile_edge_below": ("gaussian", 256, 5, 13, dict(tiles=1, chunks=2)),
    "tile_edge_above": ("gaussian", 257, 5, 13, dict(tiles=2, chunks=2)),
    "lba_two_tiles": ("lba", 300, 10, 13, dict(tiles=2, chunks=3)),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_statistics_against_the_definition(demc, name):
    family, N, n, P, want = SHAPES[name]
    g = PL.geometry(N, n * P)
    for k, v in want.items():
        assert g[k] == v, f"{name}: {k} is {g[k]}, the case was chosen for {v} -- the constants of csrc/demc_pwplan.hpp moved"
    prob = make_problem(family, np.random.default_rng(3000 + N + n), N=N)
    eng, _ = engine(demc, prob, n, P)
    check_waic(demc, eng, prob, 0, n, name)
    eng.close()


def test_padded_history_and_a_window_that_starts_late(demc):
    """partners from the history: cells of D = 3 are 4 doubles apart, and the kept rows start behind the initial ones; then a window
    with row0 > 0 inside them"""
    from test_quantile_host import hist_ld
    assert hist_ld(3, True) == 4
    prob = make_problem("lnr", np.random.default_rng(77), N=65, na=2)
    assert prob["D"] == 3
    n, P = 20, 8
    eng, rows = engine(demc, prob, n, P, n_initial=3, partner_kind=1)
    eng.set_history_rows(0, np.stack([prob["init"](P) for _ in range(3)]))
    tot, pt = check_waic(demc, eng, prob, 3, 3 + n, "padded cells, rows 3..23")
    ll = eng.pointwise_loglik(rows.reshape(-1, 3))  # the rows as they were written: the padding is not a value
    check_waic(demc, eng, prob, 3, 3 + n, "padded cells against the rows written", ll=ll)
    tot2, _ = check_waic(demc, eng, prob, 9, 17, "rows 9..17")
    assert tot2[0] != tot[0]
    eng.close()


@pytest.mark.parametrize("family,d", [("mvn_iso", 8), ("mvn_full", 31)])
def test_mvn_statistics(demc, family, d):
    prob = make_problem(family, np.random.default_rng(4000 + d), N=65, d=d)
    eng, _ = engine(demc, prob, 10, 13, loglike_mode=2)
    check_waic(demc, eng, prob, 0, 10, f"{family} d={d}")
    eng.close()


# ---- 3. end to end without the device's terms --------------------------------------------------------------------------------------
def _posterior_like_rows(rng, n, P, centre, spread):
    return centre + spread * rng.normal(0, 1, (n, P, len(centre)))


@pytest.mark.parametrize("family", ["gaussian", "binomial", "mvn_full"])
def test_end_to_end_against_numpy(demc, family):
    rng = np.random.default_rng(5000)
    n, P = 10, 13
    if family == "gaussian":
        prob = make_problem(family, rng, N=130)
        x = np.asarray(prob["data"])
        rows = _posterior_like_rows(rng, n, P, np.array([x.mean(), x.std()]), 0.1)
        eng, _ = engine(demc, prob, n, P, rows=rows)
        th = draws_of(eng.export_chains(0, n), 2)
        ll = -0.5 * ((x[None, :] - th[:, :1]) / th[:, 1:]) ** 2 - np.log(th[:, 1:]) - 0.5 * math.log(2 * math.pi)
    elif family == "binomial":
        prob = make_problem(family, rng, N=65)
        nn, kk = np.asarray(prob["data"][:65]), np.asarray(prob["data"][65:])
        rows = np.clip(_posterior_like_rows(rng, n, P, np.array([kk.sum() / nn.sum()]), 0.05), 0.05, 0.95)
        eng, _ = engine(demc, prob, n, P, rows=rows)
        th = draws_of(eng.export_chains(0, n), 1)
        lgc = np.array([math.lgamma(a + 1) - math.lgamma(b + 1) - math.lgamma(a - b + 1) for a, b in zip(nn, kk)])
        ll = lgc[None, :] + kk[None, :] * np.log(th) + (nn - kk)[None, :] * np.log1p(-th)
    else:
        d = 8
        prob = make_problem(family, rng, N=65, d=d)
        X, Sigma = np.asarray(prob["data"]).reshape(65, d), prob["Sigma"]
        rows = _posterior_like_rows(rng, n, P, X.mean(axis=0), 0.2)
        eng, _ = engine(demc, prob, n, P, rows=rows, loglike_mode=2)
        th = draws_of(eng.export_chains(0, n), d)
        Lc = np.linalg.cholesky(Sigma)
        z = np.linalg.solve(Lc, (X[None, :, :] - th[:, None, :]).reshape(-1, d).T).T.reshape(th.shape[0], 65, d)
        ll = -0.5 * (z ** 2).sum(axis=2) - 0.5 * (d * math.log(2 * math.pi) + 2 * np.log(np.diag(Lc)).sum())
    assert (np.abs(ll).max(axis=0) / ll.std(axis=0, ddof=1) <= 1e4).all(), "badly conditioned draws: the bars do not hold for them"
    check_waic(demc, eng, prob, 0, n, f"end to end {family}", ll=ll)
    eng.close()


# ---- 4. edge rules -----------------------------------------------------------------------------------------------------------------
def _lnr_with_late_tau(demc, every_draw):
    prob = make_problem("lnr", np.random.default_rng(88), N=65, na=2)
    rt = np.asarray(prob["data"][65:])
    late = int(np.argmin(rt))  # the fastest trial: the first to fall behind tau
    n, P = 4, 5
    rows = np.stack([prob["init"](P) for _ in range(n)])
    tau = (rt[late] + np.sort(rt)[1]) / 2  # above the fastest decision time only
    if every_draw:
        rows[:, :, 2] = tau
    else:
        rows[1, 2, 2] = rows[3, 0, 2] = tau
    prob["hi"] = [np.inf] * 3  # (history draws are evaluated as stored; the matrix call would refuse tau above the bound)
    eng, _ = engine(demc, prob, n, P, rows=rows)
    return eng, prob, late


def test_lnr_tau_above_a_decision_time_in_some_draws(demc):
    eng, prob, late = _lnr_with_late_tau(demc, False)
    tot, pt = check_waic(demc, eng, prob, 0, 4, "tau late in 2 of 20 draws", guard=False)
    assert math.isfinite(pt[late, 0]) and np.isnan(pt[late, 1:]).all()  # lppd finite, the moments and elpd NaN
    others = np.delete(np.arange(65), late)
    assert np.isfinite(pt[others]).all()
    assert tot[7] == 1 and math.isfinite(tot[3]) and math.isnan(tot[0]) and math.isnan(tot[2]) and math.isnan(tot[4]) and math.isnan(tot[5])
    eng.close()


def test_lnr_tau_above_a_decision_time_in_every_draw(demc):
    eng, prob, late = _lnr_with_late_tau(demc, True)
    tot, pt = check_waic(demc, eng, prob, 0, 4, "tau late in every draw", guard=False)
    assert pt[late, 0] == -np.inf and np.isnan(pt[late, 1:3]).all() and np.isnan(pt[late, 3])
    assert tot[7] == 1 and tot[3] == -np.inf
    eng.close()


def test_nan_cell_and_unchanged_state_and_equal_bits(demc, orc):
    prob = make_problem("gaussian", np.random.default_rng(99), N=130)
    n, P = 10, 13
    eng, rows = engine(demc, prob, n, P)
    eng.set_state(rows[0])
    before = (eng.get_history(0, n), eng.get_state())
    a = eng.waic(0, n, pointwise=True)
    b = eng.waic(0, n, pointwise=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()  # no floating-point atomics
    only_totals = eng.waic(0, n)
    assert only_totals[1] is None and only_totals[0].tobytes() == a[0].tobytes()
    pt_only = np.empty((130, 4))
    assert eng.L.demc_waic(eng.h, 0, n, None, pt_only.ctypes.data_as(C.POINTER(C.c_double))) == 0 and pt_only.tobytes() == a[1].tobytes()
    m1 = eng.pointwise_loglik(rows[2])
    m2 = eng.pointwise_loglik(rows[2])
    assert m1.tobytes() == m2.tobytes()
    after = (eng.get_history(0, n), eng.get_state())
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert x.tobytes() == y.tobytes()  # history, acceptance, lp, ids, state, weights
    # a NaN theta cell: every term of that draw is NaN, and so are all four values of every observation
    rows[4, 6, 0] = np.nan
    eng.set_history_rows(0, rows)
    tot, pt = check_waic(demc, eng, prob, 0, n, "a NaN cell", guard=False)
    assert np.isnan(pt).all() and tot[7] == 130 and np.isnan(tot[:6]).all() and tot[6] == 0
    tot, pt = check_waic(demc, eng, prob, 5, n, "rows behind the NaN cell")
    assert np.isfinite(pt).all() and tot[7] == 0
    # demc_pointwise_loglik: a row outside the bounds in force, or with a NaN in it, is a row of NaN
    th = np.array([[0.1, 1.0], [0.1, -1.0], [np.nan, 1.0], [0.2, 2.0]])
    m = eng.pointwise_loglik(th)
    assert np.isfinite(m[0]).all() and np.isnan(m[1]).all() and np.isnan(m[2]).all() and np.isfinite(m[3]).all()
    # a row exactly ON a bound is evaluated, not flagged (in_bounds is inclusive), one just beyond it is a row of NaN; the finite / NaN
    # pattern of the row sum plus the prior is demc_logpost's
    eng.set_bounds([-0.5, 0.25], [0.5, 3.0])
    th = np.array([[0.5, 1.0], [-0.5, 0.25], [0.2, 3.0], [np.nextafter(0.5, 1.0), 1.0], [0.2, np.nextafter(0.25, 0.0)], [0.1, 1.0]])
    m = eng.pointwise_loglik(th)
    assert np.isfinite(m[[0, 1, 2, 5]]).all() and np.isnan(m[[3, 4]]).all()
    x = np.asarray(prob["data"])
    want = -0.5 * ((x[None, :] - th[:3, :1]) / th[:3, 1:]) ** 2 - np.log(th[:3, 1:]) - 0.5 * math.log(2 * math.pi)
    assert (np.abs(m[:3] - want) <= BAR * np.maximum(1.0, np.abs(want))).all()
    lp = eng.logpost(th)
    o = orc.Oracle(n_groups=1, Np=4, D=2)
    setup_engine(o, prob)
    total = m.sum(axis=1) + o.prior(th)
    o.close()
    assert np.array_equal(np.isfinite(total), np.isfinite(lp)), (total, lp)
    assert np.isfinite(lp[[0, 1, 2, 5]]).all() and (np.abs(total - lp)[[0, 1, 2, 5]] <= BAR * np.maximum(1.0, np.abs(lp[[0, 1, 2, 5]]))).all()
    eng.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def _refused(demc, fn, code, *words):
    with pytest.raises(demc.DemcError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals(demc):
    from demc_amd import families as F
    E, U = demc._ffi.EINVAL, demc._ffi.EUNSUPPORTED
    rng = np.random.default_rng(5)
    prob = make_problem("gaussian", rng, N=20)
    eng, rows = engine(demc, prob, 6, 4)
    dp = C.POINTER(C.c_double)
    buf = np.empty(8)
    for r0, r1 in ((-1, 3), (2, 2), (3, 2), (0, 7)):
        _refused(demc, lambda: eng.waic(r0, r1), E, "bad rows: demc_waic needs at least one row of the history")
    assert eng.L.demc_waic(eng.h, 0, 6, None, None) == E
    assert eng.L.demc_last_error(eng.h).decode() == "demc_waic: total_out and pointwise_out are both NULL"
    assert eng.L.demc_waic(eng.h, 0, 7, None, None) == E  # ... and the rows rank before the outputs
    assert eng.L.demc_last_error(eng.h).decode() == "bad rows: demc_waic needs at least one row of the history"
    assert eng.L.demc_waic(None, 0, 6, buf.ctypes.data_as(dp), None) == E
    _refused(demc, lambda: eng.pointwise_loglik(np.empty((0, 2))), E, "demc_pointwise_loglik: n < 1")
    assert eng.L.demc_pointwise_loglik(eng.h, None, 1, buf.ctypes.data_as(dp)) == E
    # the cell cap is refused before anything is read or allocated: n N = (2^27 / 20 + 1) x 20
    th = np.zeros((1, 2))
    assert eng.L.demc_pointwise_loglik(eng.h, th.ctypes.data_as(dp), (1 << 27) // 20 + 1, buf.ctypes.data_as(dp)) == E
    assert "above the cap of 134217728 cells" in eng.L.demc_last_error(eng.h).decode()
    eng.close()
    # no history on the handle; no model
    bare = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=0, store_history=0)
    setup_engine(bare, prob)
    _refused(demc, lambda: bare.waic(0, 1), E, "history is not stored on this handle")
    bare.close()
    nomodel = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4)
    nomodel.n_obs = 1
    _refused(demc, lambda: nomodel.waic(0, 4), E, "demc_waic: no model is set on this handle")
    _refused(demc, lambda: nomodel.pointwise_loglik(np.zeros((1, 2))), E, "demc_pointwise_loglik: no model is set on this handle")
    nomodel.close()
    # a race model without a trial: demc_set_model accepts dims = [0, n_acc]; both calls refuse it (nothing to divide the launch by)
    for fam, D in ((F.FAM_LBA, 6), (F.FAM_LNR, 4)):
        empty = demc.HipEngine(n_groups=1, Np=4, D=D, n_rows=4)
        empty.set_model(fam, np.empty(0), [0, 3], [1.0] if fam == F.FAM_LNR else None)
        assert empty.n_obs == 0
        _refused(demc, lambda: empty.waic(0, 4), E, "demc_waic: the model holds no observations (N < 1)")
        _refused(demc, lambda: empty.pointwise_loglik(np.ones((2, D))), E, "demc_pointwise_loglik: the model holds no observations (N < 1)")
        empty.close()
    # a sharded handle
    shard = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4, n_groups_total=2, group_offset=1)
    setup_engine(shard, prob)
    _refused(demc, lambda: shard.waic(0, 4), E, "sharded handle")
    shard.close()
    # MvNormal outside DIRECT mode: the message names the way in
    for fam, mode in (("mvn_iso", 0), ("mvn_full", 0), ("mvn_full", 1)):
        p = make_problem(fam, rng, N=30, d=4)
        e, _ = engine(demc, p, 3, 4, loglike_mode=mode)
        _refused(demc, lambda: e.waic(0, 3), U, "loglike_mode = direct")
        _refused(demc, lambda: e.pointwise_loglik(p["init"](2)), U, "loglike_mode = direct")
        e.close()
    # families without a per-observation term: the message names the family
    for fam, name in (("hier_binomial", "DEMC_FAM_HIER_BINOMIAL"), ("hier_gaussian", "DEMC_FAM_HIER_GAUSSIAN")):
        p = make_problem(fam, rng)
        e, _ = engine(demc, p, 3, 4)
        _refused(demc, lambda: e.waic(0, 3), U, name)
        _refused(demc, lambda: e.pointwise_loglik(p["init"](2)), U, name)
        e.close()
    from demc_amd import families as F
    e = demc.HipEngine(n_groups=1, Np=4, D=3, n_rows=3)
    e.set_model(F.FAM_RASTRIGIN, None, [])
    _refused(demc, lambda: e.waic(0, 3), U, "DEMC_FAM_RASTRIGIN")
    e.close()
    e = demc.HipEngine(n_groups=1, Np=4, D=5, n_rows=3)
    e.set_model(F.FAM_ODE_LV, rng.uniform(1, 2, (6, 2)), [6, 2], [1.0, 1.0, 0.1, 4])
    _refused(demc, lambda: e.waic(0, 3), U, "DEMC_FAM_ODE_LV")
    e.close()
    e = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=3)
    e.set_model_sim(0, 0, 64, rng.normal(0, 1, 10), [0.0])
    _refused(demc, lambda: e.waic(0, 3), U, "simulation likelihood")
    e.close()
    e = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=3)
    e.set_model_source("__device__ double demc_user_obs(const double* theta, int D, const double* data, long long N, long long i, "
                       "const double* hyper, int nhyper) { return -0.5 * (data[i] - theta[0]) * (data[i] - theta[0]); }", rng.normal(0, 1, 10), [10])
    _refused(demc, lambda: e.waic(0, 3), U, "hiprtc plug-in")
    e.close()


# ---- 6. summarize(..., waic=True) -----------------------------------------------------------------------------------------------------
def test_summarize_with_waic(demc):
    rng = np.random.default_rng(50514)
    data = rng.normal(0.0, 1.0, 50)
    sp = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy()) + 0.2]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, names=("μ", "σ"), data=data, prior_loglike=demc.Priors(μ=demc.Normal(0, 1), σ=demc.TruncatedCauchy(0, 1)),
                         loglike=demc.GaussianLikelihood())
    de = demc.DE(sample_prior=sp, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
    kept = {}

    class Keeping(demc.HipEngine):  # the same engine, remembering what waic answered for the kept rows
        def waic(self, row0, row1, pointwise=False):
            kept["rows"] = (row0, row1)
            kept["direct"] = demc.HipEngine.waic(self, row0, row1, True)
            return demc.HipEngine.waic(self, row0, row1, pointwise)

    s = demc.summarize(model, de, demc.HIPBackend(seed=1), 300, waic="pointwise", engine_factory=Keeping)
    assert kept["rows"] == (100, 300) and s.waic is not None
    assert s.waic.totals.tobytes() == kept["direct"][0].tobytes() and s.waic.pointwise.tobytes() == kept["direct"][1].tobytes()
    assert s.waic.pointwise.shape == (50, 4) and math.isfinite(s.waic.elpd_waic) and 0 < s.waic.p_waic < 50 and s.waic.n_nonfinite == 0
    assert math.isfinite(s["μ"]["mean"])  # the other tables of the same run are there too
    assert demc.summarize(model, de, demc.HIPBackend(seed=1), 300).waic is None

    # a free LNR run: finite totals, an effective number of parameters inside (0, N)
    N = 80
    nu_true, tau_true = np.array([-1.0, -0.4, -0.2]), 0.3
    t = np.exp(nu_true[None, :] + rng.normal(0, 1, (N, 3)))
    lnr_data = (np.argmin(t, axis=1) + 1.0, t.min(axis=1) + tau_true)
    min_rt = lnr_data[1].min()
    spl = lambda: demc.as_union([rng.normal(0, 1, 3), rng.uniform(0, min_rt)])  # noqa: E731
    lmodel = demc.DEModel(sample_prior=spl, names=("ν", "τ"), data=lnr_data,
                          prior_loglike=demc.Priors(ν=demc.Normal(0, 3), τ=demc.Uniform(0, min_rt)), loglike=demc.LNRLikelihood(sigma=1.0))
    lde = demc.DE(sample_prior=spl, bounds=((-np.inf, np.inf), (0.0, min_rt)), burnin=200, Np=8)
    w = demc.summarize(lmodel, lde, demc.HIPBackend(seed=2), 400, waic=True).waic
    print(w)
    assert np.isfinite(w.totals).all() and 0 < w.p_waic < N and w.pointwise is None and w.n_nonfinite == 0


def test_summarize_refuses_before_the_run_what_waic_would_refuse_after_it(demc):
    """an MvNormal model outside DIRECT mode: summarize(..., waic=True) ends before the first step, with the reason demc_waic would give"""
    rng = np.random.default_rng(7)
    d, N = 3, 40
    Sigma = np.eye(d)
    X = rng.normal(0, 1, (d, N))
    sp = lambda: [rng.normal(0, 1, d)]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, names=("μ",), data=X, prior_loglike=demc.Priors(μ=demc.Normal(0, 1)), loglike=demc.MvNormalFullLikelihood(Sigma))
    de = demc.DE(sample_prior=sp, bounds=((-np.inf, np.inf),), burnin=10, Np=6)
    steps = []

    class Counting(demc.HipEngine):
        def step(self, iter0, n_iters=1):
            steps.append(n_iters)
            return demc.HipEngine.step(self, iter0, n_iters)

    with pytest.raises(demc.DemcError) as e:
        demc.summarize(model, de, demc.HIPBackend(seed=1, loglike_mode="streaming"), 30, waic=True, engine_factory=Counting)
    assert e.value.code == demc._ffi.EUNSUPPORTED and "loglike_mode = direct" in str(e.value) and not steps
    s = demc.summarize(model, de, demc.HIPBackend(seed=1, loglike_mode="direct"), 30, waic=True, engine_factory=Counting)
    assert steps and math.isfinite(s.waic.elpd_waic) and s.waic.n_nonfinite == 0
