"""demc_loo (include/demc_loo.h, csrc/demc_loo.{hpp,cpp}; the definition is DESIGN.md 5.9) on the GPU.  Engines are filled by
set_history_rows; nothing is stepped unless a test says so.

1. the statistics against the definition on the device's own terms: chains.loo_from_loglik(pointwise_loglik(exported rows)).  Device
   and reference select from the same bits, so n_tail_i and l_cut_i are equal exactly; the other columns at 1e-9 max(1, |ref|), the
   totals at 1e-9 of sum |terms|, the counts exactly.
2. end to end without the device's terms: closed_terms of tests/pointwise_cases.py; the reference columns have no gap below
   1e-9 |l| at the cutoff (asserted on the reference alone, first), so n_tail is still exact and l_cut agrees to the terms' own error.
3. the non-finite patterns, 4. repeatability and side effects, 5. the refusals, 6. lppd against demc_waic, 7. summarize(..., loo=True).
8. tied, crowded and narrow columns (the families of tests/loo_cases.py) and a sampler-made history, as in 1.; each test first
   proves with LC.select_path, on the device's own terms, that the branches of the radix select it is there for are reached.

A handle needs Np >= 3, so the shortest window the device can be given holds S = 3 draws: S = 1 of the definition is checked on
the host (tests/test_loo_host.py) and S = 3 stands in for it here."""
import ctypes as C
import math

import numpy as np
import pytest

import loo_cases as LC
import test_gpu_pointwise as TP
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu
BAR = LC.BAR


def check_loo(demc, eng, row0, row1, label, ll=None, exact_tail=True, cols=None, khat=True):
    """device against chains.loo_from_loglik of ll (the device's own terms of the exported rows when None) -> (totals, pointwise).
    khat=False (the narrow family alone, which says why): the size of khat is printed, not held to the bar -- its finite / infinite
    pattern still is -- the two counts taken from khat are held to the device's own column, and the total of p_loo, a sum of
    differences that cancel to 1e-18 there, is held to its bar plus the rounding of the terms it is formed from."""
    if ll is None:
        ll = eng.pointwise_loglik(TP.draws_of(eng.export_chains(row0, row1), eng.D))
    assert ll.shape[0] == (row1 - row0) * eng.P
    ref = demc.loo_from_loglik(ll)
    tot, pt = eng.loo(row0, row1, pointwise=True)
    assert pt.shape == (eng.n_obs, 6) and tot.shape == (8,)
    sub = pt if cols is None else pt[cols]
    worst = LC.check_table(sub, ref.pointwise, label, exact_tail)
    if not exact_tail:  # the terms differ in their last bits: l_cut to the terms' own bar
        f = np.isfinite(ref.pointwise[:, 5])
        assert (np.abs(sub[f, 5] - ref.pointwise[f, 5]) <= BAR * np.maximum(1.0, np.abs(ref.pointwise[f, 5]))).all(), label
    t_err = {}
    if cols is None:
        p = ref.pointwise
        sums = dict(elpd_loo=np.abs(p[:, 0]).sum(), p_loo=np.abs(p[:, 1]).sum(), lppd=np.abs(p[:, 3]).sum(), looic=2 * np.abs(p[:, 0]).sum())
        for j, name in enumerate(demc.chains.LOO_TOTALS):
            want = getattr(ref, name)
            if name in ("n_k_high", "n_k_bad") and not khat:
                assert tot[j] == (pt[:, 2] > (0.7 if name == "n_k_high" else 1.0)).sum(), (label, name, tot[j])
            elif name in ("n_k_high", "n_k_bad", "n_nonfinite"):
                assert tot[j] == want, (label, name, tot[j], want)
            elif not math.isfinite(want):
                assert (math.isnan(want) and math.isnan(tot[j])) or tot[j] == want, (label, name, tot[j], want)
            elif name == "se_elpd":
                t_err[name] = abs(tot[j] - want) / max(want, 1e-300) / BAR
            elif name == "p_loo" and not khat:  # (narrow columns, p_loo_i far under an ulp of lppd_i: the bar gets the floor that
                # the roundings of lppd_i and elpd_loo_i, four ulps each at the most, leave in their difference)
                t_err[name] = abs(tot[j] - want) / (BAR * sums[name] + 2.0 ** -50 * sums["lppd"])
            else:
                t_err[name] = abs(tot[j] - want) / max(sums[name], 1e-300) / BAR
    print(f"{label}: S={ll.shape[0]} N={eng.n_obs} in units of the bar: " + " ".join(f"{k} {v:.3g}" for k, v in {**worst, **t_err}.items()) +
          f"; n_tail {int(np.nanmin(sub[:, 4])) if np.isfinite(sub[:, 4]).any() else -1}..{int(np.nanmax(sub[:, 4])) if np.isfinite(sub[:, 4]).any() else -1}")
    if not khat:
        f = np.isfinite(ref.pointwise[:, 2])
        print(f"{label}: khat is not compared; largest gap {np.abs(sub[f, 2] - ref.pointwise[f, 2]).max():.3g} absolute, {worst.pop('khat'):.3g} bars")
    assert all(v <= 1.0 for v in worst.values()), (label, worst)
    assert all(v <= 1.0 for v in t_err.values()), (label, t_err)
    return tot, pt


def gaussian_problem(rng, N):
    prob = make_problem("gaussian", rng, N=N)
    prob["data"][0] = 50.0  # beside ordinary points: its ratios span more than 708 log units, the floor is active
    return prob


GAUSS_S = {3: (1, 3), 20: (5, 4), 21: (7, 3), 26: (2, 13), 130: (10, 13), 2000: (20, 100)}  # S: (rows, particles)


# ---- 1. the statistics against the definition, on the device's own terms ------------------------------------------------------------
@pytest.mark.parametrize("S", list(GAUSS_S))
@pytest.mark.parametrize("N", [1, 5, 65])
def test_gaussian_against_the_definition(demc, N, S):
    rng = np.random.default_rng(9000 + 7 * N + S)
    n, P = GAUSS_S[S]
    prob = gaussian_problem(rng, N)
    eng, _ = TP.engine(demc, prob, n, P, rows=LC.gaussian_draws(rng, S).reshape(n, P, 2))
    tot, pt = check_loo(demc, eng, 0, n, f"gaussian N={N} S={S}")
    M = LC.plan(N, S)["M"]
    if S <= 20:
        assert (pt[:, 4] == 0).all() and np.isnan(pt[:, 5]).all() and np.isposinf(pt[:, 2]).all()
    else:
        assert (pt[:, 4] <= M).all()
        if S >= 130:
            assert pt[0, 4] < M, "y = 50 was chosen for an active floor"
        if N > 1:
            assert (pt[1:, 4] == M).all()
    eng.close()


def test_a_window_that_starts_late_and_padded_cells(demc):
    """S = 130 behind three initial rows; Gaussian cells (D = 2) are dense, LNR cells of D = 3 are 4 doubles apart"""
    from test_quantile_host import hist_ld
    rng = np.random.default_rng(9100)
    prob = gaussian_problem(rng, 65)
    n, P = 10, 13
    eng, _ = TP.engine(demc, prob, n, P, rows=LC.gaussian_draws(rng, 130).reshape(n, P, 2), n_initial=3, partner_kind=1)
    eng.set_history_rows(0, LC.gaussian_draws(rng, 39).reshape(3, P, 2))
    a, _ = check_loo(demc, eng, 3, 3 + n, "gaussian rows 3..13")
    b, _ = check_loo(demc, eng, 5, 11, "gaussian rows 5..11")
    assert a[0] != b[0]
    eng.close()
    assert hist_ld(3, True) == 4
    prob = make_problem("lnr", rng, N=65, na=2)
    eng, rows = TP.engine(demc, prob, n, P, n_initial=3, partner_kind=1)
    eng.set_history_rows(0, np.stack([prob["init"](P) for _ in range(3)]))
    check_loo(demc, eng, 3, 3 + n, "lnr padded cells, rows 3..13")
    check_loo(demc, eng, 3, 3 + n, "lnr padded cells against the rows written", ll=eng.pointwise_loglik(rows.reshape(-1, 3)))
    eng.close()


def _long_engine(demc, prob, rng, n_rows=256, rows=None):
    """the 16 x 16 x 256 handle: S = 65 536 (n_rows = 36: S = 9216)"""
    eng = demc.HipEngine(n_groups=16, Np=16, D=2, n_rows=n_rows, seed=1)
    setup_engine(eng, prob)
    rows = (LC.gaussian_draws(rng, 256 * n_rows) if rows is None else rows).reshape(n_rows, 256, 2)
    eng.set_history_rows(0, rows)
    return eng, rows


def test_long_window(demc):
    """S = 65 536, M = 768: 128 strides of the column kernel per read"""
    rng = np.random.default_rng(9200)
    prob = gaussian_problem(rng, 5)
    assert LC.plan(5, 65536) == dict(M=768, Nb=5, blocks=1, cuts=[(0, 5)], tiles=1, chunks=2048, chunk_len=32)
    eng, _ = _long_engine(demc, prob, rng)
    tot, pt = check_loo(demc, eng, 0, 256, "long window")
    assert pt[0, 4] < 768 and (pt[1:, 4] == 768).all()
    eng.close()


def test_more_than_one_observation_block(demc):
    """S = 65 536 and N = 2049: one cell over 2^27, so the last observation is a block of its own"""
    rng = np.random.default_rng(9300)
    N = 2049
    pl = LC.plan(N, 65536)
    assert pl["Nb"] == 2048 and pl["blocks"] == 2 and pl["cuts"] == [(0, 2048), (2048, 2049)]
    prob = gaussian_problem(rng, N)
    eng, rows = _long_engine(demc, prob, rng)
    tot, pt = eng.loo(0, 256, pointwise=True)
    cols = np.unique(np.concatenate([[0, 1, 63, 64, 65, 1023, 1024, 2046, 2047, 2048], rng.choice(N, 38, replace=False)]))[:48]
    assert {0, 2047, 2048} <= set(cols.tolist())  # the first and last column of each block
    # the device's own terms of those columns: the same draws on a handle that holds those observations alone (a term reads its own
    # observation and the draw, nothing else)
    few = dict(prob, data=np.asarray(prob["data"])[cols], dims=[len(cols)])
    small = demc.HipEngine(n_groups=16, Np=16, D=2, n_rows=1, seed=1)
    setup_engine(small, few)
    ll = small.pointwise_loglik(TP.draws_of(eng.export_chains(0, 256), 2))
    small.close()
    ref = demc.loo_from_loglik(ll).pointwise
    worst = LC.check_table(pt[cols], ref, "two blocks")
    print("two blocks, 48 columns, in units of the bar:", worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    ld = np.longdouble
    e = pt[:, 0].astype(ld)
    want = [e.sum(), np.sqrt(N * (((e - e.sum() / N) ** 2).sum() / ld(N - 1))), pt[:, 1].astype(ld).sum(), pt[:, 3].astype(ld).sum(), -2 * e.sum()]
    scale = [np.abs(pt[:, 0]).sum(), float(want[1]), np.abs(pt[:, 1]).sum(), np.abs(pt[:, 3]).sum(), 2 * np.abs(pt[:, 0]).sum()]
    for j in range(5):
        assert abs(tot[j] - float(want[j])) <= BAR * scale[j], (j, tot[j], want[j])
    assert tot[5] == (pt[:, 2] > 0.7).sum() and tot[6] == (pt[:, 2] > 1.0).sum() and tot[7] == 0
    eng.close()


def test_lba_in_the_callers_order(demc):
    rng = np.random.default_rng(9400)
    N = 257
    prob = make_problem("lba", rng, N=N)
    ch, rt = prob["data"][:N], prob["data"][N:]
    assert not np.array_equal(np.lexsort((rt, ch)), np.arange(N)), "the trials are already in the library's order"
    assert LC.plan(N, 130)["tiles"] == 5
    eng, _ = TP.engine(demc, prob, 10, 13)
    check_loo(demc, eng, 0, 10, "lba N=257")
    eng.close()


@pytest.mark.parametrize("family,kw", [("lnr", {}), ("binomial", {}), ("mvn_iso", dict(d=9)), ("mvn_iso", dict(d=33)), ("mvn_full", dict(d=9)), ("mvn_full", dict(d=33))])
def test_other_families(demc, family, kw):
    rng = np.random.default_rng(9500 + kw.get("d", 0))
    prob = make_problem(family, rng, N=65, **kw)
    eng, _ = TP.engine(demc, prob, 10, 13, **(dict(loglike_mode=2) if kw else {}))
    check_loo(demc, eng, 0, 10, f"{family} {kw}")
    eng.close()


# ---- 2. end to end without the device's terms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["gaussian", "binomial", "mvn_full"])
def test_end_to_end_against_closed_forms(demc, family):
    import pointwise_cases as PC
    rng = np.random.default_rng(9600)
    n, P = 10, 13
    if family == "gaussian":
        prob = make_problem(family, rng, N=130)
        x = np.asarray(prob["data"])
        rows = TP._posterior_like_rows(rng, n, P, np.array([x.mean(), x.std()]), 0.1)
        kw = {}
    elif family == "binomial":
        prob = make_problem(family, rng, N=65)
        nn, kk = np.asarray(prob["data"][:65]), np.asarray(prob["data"][65:])
        rows = np.clip(TP._posterior_like_rows(rng, n, P, np.array([kk.sum() / nn.sum()]), 0.05), 0.05, 0.95)
        kw = {}
    else:
        prob = make_problem(family, rng, N=65, d=8)
        rows = TP._posterior_like_rows(rng, n, P, np.asarray(prob["data"]).reshape(65, 8).mean(axis=0), 0.2)
        kw = dict(loglike_mode=2)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows, **kw)
    ll = PC.closed_terms(prob, TP.draws_of(eng.export_chains(0, n), prob["D"]))
    assert LC.cutoff_gap_ok(ll).all(), "a reference column has a gap below 1e-9 |l| at its cutoff: choose other draws"
    check_loo(demc, eng, 0, n, f"end to end {family}", ll=ll, exact_tail=False)
    ref = demc.loo_from_loglik(ll).pointwise
    assert np.array_equal(eng.loo(0, n, pointwise=True)[1][:, 4], ref[:, 4])  # n_tail is exact all the same
    eng.close()


# ---- 3. non-finite patterns -------------------------------------------------------------------------------------------------------
def test_lnr_tau_above_a_decision_time_in_three_draws(demc):
    prob = make_problem("lnr", np.random.default_rng(88), N=65, na=2)
    rt = np.asarray(prob["data"][65:])
    late = int(np.argmin(rt))
    n, P = 10, 13
    rows = np.stack([prob["init"](P) for _ in range(n)])
    rows[1, 2, 2] = rows[3, 0, 2] = rows[9, 12, 2] = (rt[late] + np.sort(rt)[1]) / 2  # above the fastest decision time only
    prob["hi"] = [np.inf] * 3
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    tot, pt = check_loo(demc, eng, 0, n, "tau late in 3 of 130 draws")
    assert pt[late, 0] == -np.inf and pt[late, 1] == np.inf and pt[late, 2] == np.inf and math.isfinite(pt[late, 3]) and pt[late, 4] == 0 and pt[late, 5] == -np.inf
    assert np.isfinite(np.delete(pt, late, axis=0)[:, [0, 1, 3, 4, 5]]).all()
    assert tot[7] == 1 and tot[0] == -np.inf and tot[2] == np.inf and math.isfinite(tot[3]) and tot[4] == np.inf and tot[5] >= 1 and tot[6] >= 1
    eng.close()


def test_nan_cell(demc):
    rng = np.random.default_rng(99)
    prob = gaussian_problem(rng, 130)
    n, P = 10, 13
    rows = LC.gaussian_draws(rng, 130).reshape(n, P, 2)
    rows[4, 6, 0] = np.nan
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    tot, pt = check_loo(demc, eng, 0, n, "a NaN cell")
    assert np.isnan(pt).all() and tot[7] == 130 and np.isnan(tot[:5]).all() and tot[5] == 0 and tot[6] == 0
    tot, pt = check_loo(demc, eng, 5, n, "rows behind the NaN cell")
    assert np.isfinite(pt[:, [0, 1, 3, 4, 5]]).all() and tot[7] == 0
    eng.close()


# ---- 4. repeatability and side effects --------------------------------------------------------------------------------------------
def test_equal_bits_and_unchanged_state(demc):
    rng = np.random.default_rng(9700)
    prob = gaussian_problem(rng, 130)
    n, P = 20, 100
    rows = LC.gaussian_draws(rng, 2000).reshape(n, P, 2)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    eng.set_state(rows[0])
    before = (eng.get_history(0, n), eng.get_state())
    a = eng.loo(0, n, pointwise=True)
    b = eng.loo(0, n, pointwise=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()  # no floating-point atomics
    only_totals = eng.loo(0, n)
    assert only_totals[1] is None and only_totals[0].tobytes() == a[0].tobytes()
    pt_only = np.empty((130, 6))
    assert eng.L.demc_loo(eng.h, 0, n, None, pt_only.ctypes.data_as(C.POINTER(C.c_double))) == 0 and pt_only.tobytes() == a[1].tobytes()
    after = (eng.get_history(0, n), eng.get_state())
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert x.tobytes() == y.tobytes()  # history, acceptance, lp, ids, state, weights
    eng.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(demc):
    from demc_amd import families as F
    E, U = demc._ffi.EINVAL, demc._ffi.EUNSUPPORTED
    rng = np.random.default_rng(5)
    prob = make_problem("gaussian", rng, N=20)
    eng, rows = TP.engine(demc, prob, 6, 4)
    dp = C.POINTER(C.c_double)
    buf = np.empty(8)
    for r0, r1 in ((-1, 3), (2, 2), (3, 2), (0, 7)):
        TP._refused(demc, lambda: eng.loo(r0, r1), E, "bad rows: demc_loo needs at least one row of the history")
    assert eng.L.demc_loo(eng.h, 0, 6, None, None) == E
    assert eng.L.demc_last_error(eng.h).decode() == "demc_loo: total_out and pointwise_out are both NULL"
    assert eng.L.demc_loo(eng.h, 0, 7, None, None) == E  # ... and the rows rank before the outputs
    assert eng.L.demc_last_error(eng.h).decode() == "bad rows: demc_loo needs at least one row of the history"
    assert eng.L.demc_loo(None, 0, 6, buf.ctypes.data_as(dp), None) == E
    eng.close()
    bare = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=0, store_history=0)
    setup_engine(bare, prob)
    TP._refused(demc, lambda: bare.loo(0, 1), E, "history is not stored on this handle")
    bare.close()
    nomodel = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4)
    nomodel.n_obs = 1
    TP._refused(demc, lambda: nomodel.loo(0, 4), E, "demc_loo: no model is set on this handle")
    nomodel.close()
    for fam, D in ((F.FAM_LBA, 6), (F.FAM_LNR, 4)):
        empty = demc.HipEngine(n_groups=1, Np=4, D=D, n_rows=4)
        empty.set_model(fam, np.empty(0), [0, 3], [1.0] if fam == F.FAM_LNR else None)
        TP._refused(demc, lambda: empty.loo(0, 4), E, "demc_loo: the model holds no observations (N < 1)")
        empty.close()
    shard = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=4, n_groups_total=2, group_offset=1)
    setup_engine(shard, prob)
    TP._refused(demc, lambda: shard.loo(0, 4), E, "sharded handle: demc_loo reads the whole history of one handle")
    shard.close()
    for fam, mode in (("mvn_iso", 0), ("mvn_full", 0), ("mvn_full", 1)):
        p = make_problem(fam, rng, N=30, d=4)
        e, _ = TP.engine(demc, p, 3, 4, loglike_mode=mode)
        TP._refused(demc, lambda: e.loo(0, 3), U, "demc_loo: the MvNormal families keep sums over the data in this likelihood mode", "loglike_mode = direct")
        e.close()
    for fam, name in (("hier_binomial", "DEMC_FAM_HIER_BINOMIAL"), ("hier_gaussian", "DEMC_FAM_HIER_GAUSSIAN")):
        p = make_problem(fam, rng)
        e, _ = TP.engine(demc, p, 3, 4)
        TP._refused(demc, lambda: e.loo(0, 3), U, "demc_loo: " + name + " has no per-observation log-density on the device")
        e.close()
    e = demc.HipEngine(n_groups=1, Np=4, D=3, n_rows=3)
    e.set_model(F.FAM_RASTRIGIN, None, [])
    TP._refused(demc, lambda: e.loo(0, 3), U, "demc_loo: DEMC_FAM_RASTRIGIN has no per-observation log-density on the device")
    e.close()
    e = demc.HipEngine(n_groups=1, Np=4, D=5, n_rows=3)
    e.set_model(F.FAM_ODE_LV, rng.uniform(1, 2, (6, 2)), [6, 2], [1.0, 1.0, 0.1, 4])
    TP._refused(demc, lambda: e.loo(0, 3), U, "demc_loo: DEMC_FAM_ODE_LV has no per-observation log-density on the device")
    e.close()
    e = demc.HipEngine(n_groups=1, Np=4, D=2, n_rows=3)
    e.set_model_sim(0, 0, 64, rng.normal(0, 1, 10), [0.0])
    TP._refused(demc, lambda: e.loo(0, 3), U, "demc_loo: a simulation likelihood (demc_set_model_sim) has no per-observation log-density on the device")
    e.close()


# ---- 6. lppd against demc_waic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["gaussian", "lba"])
def test_lppd_is_demc_waics(demc, family):
    rng = np.random.default_rng(9800)
    prob = gaussian_problem(rng, 65) if family == "gaussian" else make_problem("lba", rng, N=65)
    n, P = 20, 100
    rows = LC.gaussian_draws(rng, 2000).reshape(n, P, 2) if family == "gaussian" else None
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    lt, lp = eng.loo(0, n, pointwise=True)
    wt, wp = eng.waic(0, n, pointwise=True)
    assert (np.abs(lp[:, 3] - wp[:, 0]) <= 1e-12 * np.abs(wp[:, 0])).all(), np.abs(lp[:, 3] / wp[:, 0] - 1).max()
    assert abs(lt[3] - wt[3]) <= 1e-12 * np.abs(wp[:, 0]).sum()
    eng.close()


# ---- 7. summarize(..., loo=True) ----------------------------------------------------------------------------------------------------
def test_summarize_with_loo(demc):
    rng = np.random.default_rng(50514)
    data = rng.normal(0.0, 1.0, 50)
    sp = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy()) + 0.2]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, names=("μ", "σ"), data=data, prior_loglike=demc.Priors(μ=demc.Normal(0, 1), σ=demc.TruncatedCauchy(0, 1)),
                         loglike=demc.GaussianLikelihood())
    de = demc.DE(sample_prior=sp, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
    kept = {}

    class Keeping(demc.HipEngine):  # the same engine, remembering what loo answered for the kept rows
        def loo(self, row0, row1, pointwise=False):
            kept["rows"] = (row0, row1)
            kept["direct"] = demc.HipEngine.loo(self, row0, row1, True)
            return demc.HipEngine.loo(self, row0, row1, pointwise)

    s = demc.summarize(model, de, demc.HIPBackend(seed=1), 300, waic=True, loo="pointwise", engine_factory=Keeping)
    assert kept["rows"] == (100, 300) and s.loo is not None and s.waic is not None
    assert s.loo.totals.tobytes() == kept["direct"][0].tobytes() and s.loo.pointwise.tobytes() == kept["direct"][1].tobytes()
    assert s.loo.pointwise.shape == (50, 6) and math.isfinite(s.loo.elpd_loo) and 0 < s.loo.p_loo < 50 and s.loo.n_nonfinite == 0
    assert abs(s.loo.elpd_loo - s.waic.elpd_waic) < 1.0  # a well-specified Gaussian: the two criteria agree closely
    assert abs(s.loo.lppd - s.waic.lppd) <= 1e-12 * 50 * abs(s.waic.lppd)
    assert demc.summarize(model, de, demc.HIPBackend(seed=1), 300).loo is None
    plain = demc.summarize(model, de, demc.HIPBackend(seed=1), 300, loo=True).loo
    assert plain.pointwise is None and np.isfinite(plain.totals).all()


# ---- 8. tied, crowded and narrow columns ------------------------------------------------------------------------------------------------
FAMILY_SHAPE = {9216: (36, 16, 16), 2000: (20, 1, 100), 130: (10, 1, 13), 26: (2, 1, 13)}  # S: (rows, groups, particles a group)
MIN_COLS = 4  # a path counts as reached when at least this many columns take it


def check_family(demc, y, th, label, khat=True):
    """the handle that holds the draws th[S][2] and the data y; the device's own terms; the paths its columns take (the two
    restatements agreeing, LC.select_paths); the device against the twin on those terms; a second call, equal in every byte
    -> (paths, ll, totals, pointwise)"""
    S = th.shape[0]
    n, G, P = FAMILY_SHAPE[S]
    prob = dict(make_problem("gaussian", np.random.default_rng(1), N=len(y)), data=np.asarray(y, dtype=np.float64))
    if G == 16:
        eng, _ = _long_engine(demc, prob, None, n_rows=n, rows=th)
    else:
        eng, _ = TP.engine(demc, prob, n, P, rows=th.reshape(n, P, 2))
    draws = TP.draws_of(eng.export_chains(0, n), 2)
    assert np.array_equal(np.sort(draws.view(np.uint64), axis=0), np.sort(np.ascontiguousarray(th).view(np.uint64), axis=0))
    ll = eng.pointwise_loglik(draws)
    paths = LC.select_paths(ll)
    print(f"{label}: S={S} columns by stop digit {LC.reach(paths)}; nc > 4096 in {sum(p['nc'] > 4096 for p in paths)}, nc == 0 in "
          f"{sum(p['nc'] == 0 for p in paths)}; digits skipped {sorted({p['skipped'] for p in paths})}")
    tot, pt = check_loo(demc, eng, 0, n, label, ll=ll, khat=khat)
    print(f"{label}: n_tail <= 4 in {(pt[:, 4] <= 4).sum()} columns, khat finite in {np.isfinite(pt[:, 2]).sum()}")
    again = eng.loo(0, n, pointwise=True)
    assert again[0].tobytes() == tot.tobytes() and again[1].tobytes() == pt.tobytes(), label  # whatever order the threads arrived in
    eng.close()
    return paths, ll, tot, pt


CROWD_REACH = {12: (1, 2), 24: (2, 3), 34: (3, 4), 45: (4, 5), 51: (5, "u"), 52: (5, "u")}  # the stops each k is there for


@pytest.mark.parametrize("k", LC.CROWD_K)
def test_crowd(demc, k):
    """three draws 2^-k apart, 3000 times each: the select has to count down to the digit where they part (every digit 1..5 over
    the cases), sorts more than 4096 keys, and at k = 51 and 52 cannot part them at all in some columns"""
    y, th = LC.crowd(k)
    paths, ll, tot, pt = check_family(demc, y, th, f"crowd k={k}")
    got = LC.reach(paths)
    for stop in CROWD_REACH[k]:
        assert got.get(stop, 0) >= MIN_COLS, (k, stop, got)
    if k != 51:  # (at k = 51 the device's terms crowd past 4096 keys in two columns only; the other five cases carry this reach)
        assert sum(p["nc"] > 4096 for p in paths) >= MIN_COLS, "no bitonic sort over 8192 places"
    assert pt[:, 4].max() == 216 and (pt[:, 4] <= 4).sum() >= MIN_COLS and np.isfinite(pt[:, 2]).sum() >= MIN_COLS


def test_one_draw_8500_times(demc):
    """more than 8192 equal keys: the unresolved branch, and where the repeated draw is the column's minimum nothing is compacted"""
    y, th = LC.one_draw()
    paths, ll, tot, pt = check_family(demc, y, th, "one draw 8500 times")
    assert sum(not p["early"] for p in paths) >= 8 and sum(p["nc"] == 0 for p in paths) >= 1
    for i, p in enumerate(paths):
        if not p["early"]:  # the cutoff is the repeated term; what lies below it is the tail, unless the floor cuts it
            assert pt[i, 5] == ll[:, i][np.argsort(LC.keys_of(ll[:, i]))[LC.tail_len(9216)]] and pt[i, 4] <= p["nc"]
        if p["nc"] == 0:
            assert pt[i, 4] == 0 and pt[i, 5] == ll[:, i].min() and np.isposinf(pt[i, 2])
    assert pt[:, 4].max() == LC.tail_len(9216)


def test_every_draw_four_times(demc):
    y, th = LC.four_times()
    paths, ll, tot, pt = check_family(demc, y, th, "every draw four times")
    assert LC.tail_len(2000) == 135 and (pt[1:, 4] == 132).all() and 4 < pt[0, 4] < 132  # inside a run; y = 50: the floor besides


def test_two_values(demc):
    y, th = LC.two_values()
    paths, ll, tot, pt = check_family(demc, y, th, "two values")
    assert (pt[:, 4] == 0).all() and np.isposinf(pt[:, 2]).all() and np.array_equal(pt[:, 5], ll.min(axis=0))  # x_cut = 0
    assert tot[5] == 65 and tot[6] == 65


@pytest.mark.parametrize("S", [130, 26])
def test_constant_columns(demc, S):
    y, th = LC.constant(S)
    paths, ll, tot, pt = check_family(demc, y, th, f"constant S={S}")
    assert all(not p["early"] and p["nc"] == 0 for p in paths)
    assert (ll == ll[0]).all()
    assert np.array_equal(pt[:, 0], ll[0]) and np.array_equal(pt[:, 3], ll[0]) and np.array_equal(pt[:, 5], ll[0])  # == the term
    assert (pt[:, 1] == 0).all() and (pt[:, 4] == 0).all() and np.isposinf(pt[:, 2]).all()
    assert tot[2] == 0 and tot[5] == 65 and tot[6] == 65 and tot[7] == 0 and tot[0] == tot[3]


def test_mixed_sign(demc):
    """columns that hold terms of both signs: the first digit (sign and exponent) is counted and the select stops there"""
    y, th = LC.mixed_sign()
    paths, ll, tot, pt = check_family(demc, y, th, "mixed sign")
    both = [(ll[:, i] < 0).any() and (ll[:, i] > 0).any() for i in range(ll.shape[1])]
    assert sum(p["early"] and p["stop_digit"] == 0 and b for p, b in zip(paths, both)) >= MIN_COLS, LC.reach(paths)


def test_narrow(demc):
    """draws 1e-12 apart: two or three digits skipped ahead of the counted one.  exp(x) - exp(x_cut) cancels here (x about 1e-9): one
    ulp between the device's exp and libm's moves an excess, and khat with it, by far more than 1e-9 relative -- a property of the
    definition, not an error of the kernel -- so khat's size is printed and not compared, in this family alone.  Every quartile
    excess is at least 2^-40 (asserted on the reference's side), so an ulp cannot switch a fit off and the finite / infinite pattern
    of khat is still compared exactly."""
    y, th = LC.narrow()
    assert np.nanmin(LC.quartile_excess(LC.gaussian_terms(y, th))) >= 2.0 ** -40
    paths, ll, tot, pt = check_family(demc, y, th, "narrow", khat=False)
    eq = LC.quartile_excess(ll)
    assert np.isfinite(eq).all() and eq.min() >= 2.0 ** -40, eq.min()
    assert sum(p["skipped"] >= 2 for p in paths) >= MIN_COLS and np.isfinite(pt[:, 2]).all()
    assert (pt[:, 4] >= 134).all()


def test_sampler_made_history(demc):
    """a DE-MC history as the sampler leaves it: a rejected proposal repeats the row, so ties are the normal case"""
    import test_gpu_summary as TS
    n0, n1 = 100, 400
    eng = TS.gaussian_engine(demc, 2, 4, n1, 21)
    eng.step(1, n1)
    draws = TP.draws_of(eng.export_chains(n0, n1), 2)
    S = draws.shape[0]
    M = LC.tail_len(S)
    distinct = len(np.unique(draws, axis=0))
    assert S == 2400 and distinct < S, "no rejected proposal in 300 iterations"
    ll = eng.pointwise_loglik(draws)
    paths = LC.select_paths(ll)
    tot, pt = check_loo(demc, eng, n0, n1, "sampler-made", ll=ll)
    x_cut = ll.min(axis=0) - pt[:, 5]
    tied = (pt[:, 4] < M) & (x_cut > LC.LOG_MIN)
    print(f"sampler-made: S={S}, {distinct} distinct draws, M={M}; ties at the cutoff in {tied.sum()} of {ll.shape[1]} columns, n_tail "
          f"{int(pt[:, 4].min())}..{int(pt[:, 4].max())}; stop digits {LC.reach(paths)}")
    assert tied.any(), "no column with a tie at its cutoff: choose another seed"
    again = eng.loo(n0, n1, pointwise=True)
    assert again[0].tobytes() == tot.tobytes() and again[1].tobytes() == pt.tobytes()
    eng.close()
