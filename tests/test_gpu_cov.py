"""demc_covariance (include/demc_cov.h, csrc/demc_cov.hpp; the definition is DESIGN.md 5.7) on the GPU.  The reference is always
export_chains of the same rows -- existing, tested code -- fed to the restatement of tests/test_cov_host.py (sums in np.longdouble).

Bars: with d = sqrt(diag S_ref), |cov - cov_ref|_ij <= 1e-9 d_i d_j / (N - 1) and |cor - cor_ref| <= 1e-9 -- the project's bar, as in
test_gpu_summary.py; the worst-case rounding bound of any summation order is about N 2^-53 d_i d_j, 1.2e-10 relative at N = 2^20, and
the correction term makes the error of the first mean second order, so every case keeps N <= 2^20 and |mean| / sd <= 1e7.  mean at
rtol 1e-9.  The NaN pattern, exact zeros, the unit diagonal and symmetry exactly.  Integer inputs (the known answers): equal bits.

A handle holds Np >= 3 particles, so the smallest pool a call can see is N = 3: the rules for N = 1 (and a pool of 2) are held on
the host definition (tests/test_cov_host.py); the ragged k-steps here start at 3."""
import numpy as np
import pytest

import test_cov_host as R
import test_gpu_summary as S  # gaussian_engine, synthetic_engine: the engines of the summary's GPU tests
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu
BAR = 1e-9


def check(eng, row0, row1, cols=None, value=None, label="", bits=False):
    """device against the restatement of the exported rows -> (mean, cov, cor) of the device"""
    if value is None:
        value = eng.export_chains(row0, row1)
    N = value.shape[0] * value.shape[2]
    assert N <= 1 << 20
    want = R.restate(value, cols)
    got = eng.covariance(row0, row1, cols)
    K = value.shape[1] if cols is None else len(cols)
    assert got[0].shape == (K,) and got[1].shape == got[2].shape == (K, K)
    e_mean, e_cov, e_cor = R.scaled_errors(got, want, N)
    print(f"{label}: N={N} K={K} mean {e_mean:.3g} rel, cov {e_cov:.3g} scaled, cor {e_cor:.3g}")
    assert e_mean <= BAR and e_cov <= BAR and e_cor <= BAR, (label, e_mean, e_cov, e_cor)
    for m in got[1:]:  # symmetric to the bit
        assert m.tobytes() == m.T.copy().tobytes(), label
    dg, rdg = np.diag(got[2]), np.diag(want[2])
    assert (dg[~np.isnan(rdg)] == 1.0).all(), label  # the unit diagonal, exactly
    if bits:
        for a, b, what in zip(got, want, ("mean", "cov", "cor")):
            assert R.same_bits(a, b), f"{label}: {what} differs in bits\n{a}\n{b}"
    return got


def check_geometry(n, P, D, ld, K, **want):
    g = R.geometry(n, P, D, ld, K)
    for k, v in want.items():
        assert g[k] == v, f"n={n} P={P} D={D} ld={ld} K={K}: {k} is {g[k]}, the case was chosen for {v} -- the constants of csrc/demc_cov.hpp moved"
    return g


def plain_engine(demc, n, P, D, rows, **kw):
    """nothing stepped: theta written by set_history_rows, acceptance and lp as they were created"""
    eng = demc.HipEngine(n_groups=1, Np=P, D=D, n_rows=n, seed=1, **kw)
    eng.set_history_rows(0, rows)
    return eng


# ---- exact integers: a wrong lane map or tile index cannot pass ---------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(24, 8), (2051, 7)], ids=["N24", "N2051"])
@pytest.mark.parametrize("K", [4, 17, 34, 64])
def test_known_answers_to_the_bit(demc, K, N, P):
    """K = 4: one partial tile; 17: a second block of one column; 34: three blocks; 64: all ten tiles.  N = 24: one workgroup, six
    k-steps for eight waves; N = 2051 = 4 chunks + 3 cells: five workers, the last with one ragged k-step"""
    n = N // P
    blocks = -(-K // 16)
    if N == 24:
        check_geometry(n, P, K, K, K, blocks=blocks, tiles=blocks * (blocks + 1) // 2, chunks=1, workers=1, ksteps=6, idle_waves=2)
    else:
        check_geometry(n, P, K, K, K, blocks=blocks, chunks=5, workers=5, ragged_chunk=True, ragged_kstep=True, idle_waves=7)
    v = R.kat(N, K, 100 + K)  # [N][K][1]
    eng = plain_engine(demc, n, P, K, v[:, :, 0].reshape(n, P, K))
    cols = [int(c) for c in np.random.default_rng(K).permutation(K)]
    value = eng.export_chains(0, n)
    assert np.array_equal(np.transpose(value[:, :K, :], (0, 2, 1)).reshape(N, K), v[:, :, 0])
    mean, cov, cor = check(eng, 0, n, cols, value=value, label=f"known answers K={K} N={N}", bits=True)
    x = v[:, cols, 0]
    m = x.sum(axis=0) / N
    Sint = (x - m).T @ (x - m)  # integers: exact
    assert R.same_bits(mean, m) and R.same_bits(cov, Sint / (N - 1))
    eng.close()


# ---- ragged k-steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,P", [(1, 3), (1, 5), (1, 7), (8, 8), (13, 5)], ids=["N3", "N5", "N7", "N64", "N65"])
def test_ragged_ksteps(demc, n, P):
    N = n * P
    check_geometry(n, P, 2, 2, 4, cells=N, chunks=1, workers=1, ragged_kstep=N % 4 != 0, ksteps=-(-N // 4))
    rows = np.random.default_rng(N).normal(1.0, 2.0, (n, P, 2))
    rows[:, :, 1] += 0.7 * rows[:, :, 0]
    eng = plain_engine(demc, n, P, 2, rows, schedule=1 if P < 4 else 2)
    mean, cov, cor = check(eng, 0, n, label=f"ragged N={N}")
    assert np.isfinite(cov[:2, :2]).all() and np.isfinite(cor[:2, :2]).all()
    check(eng, 0, n, [1, 0], label=f"ragged N={N}, parameters only")
    eng.close()


# ---- sampler-made history ------------------------------------------------------------------------------------------------------
N_ROWS = 129


@pytest.fixture(scope="module", params=[(2, 4, 11), (3, 23, 12)], ids=["8chains", "69chains"])
def stepped(request, demc):
    G, Np, seed = request.param
    eng = S.gaussian_engine(demc, G, Np, N_ROWS, seed)
    eng.step(1, N_ROWS)
    idh = eng.get_history(0, N_ROWS)[3]
    assert any(not np.array_equal(row, np.arange(G * Np)) for row in idh), "ids never left their slots"
    value = eng.export_chains(0, N_ROWS)
    value.setflags(write=False)
    yield eng, value
    eng.close()


@pytest.mark.parametrize("n", [2, 7, 129])
def test_sampler_made_history(stepped, n):
    eng, value = stepped
    mean, cov, cor = check(eng, 0, n, value=value[:n], label=f"sampler-made n={n} P={value.shape[2]}")
    assert set(np.unique(value[:n, 2, :])) <= {0.0, 1.0}  # acceptance: a pool of ties
    assert np.isfinite(mean).all() and np.isfinite(cov).all()


def test_rows_need_not_start_at_zero(stepped):
    eng, value = stepped
    _, _, cor = check(eng, 40, 129, value=value[40:129], label="rows 40..129")
    assert np.isfinite(cor).all() and (np.abs(cor) <= 1.0).all()


def test_cols_select_and_order(stepped):
    eng, value = stepped
    full = check(eng, 0, 50, value=value[:50], label="all four series")
    sub = check(eng, 0, 50, [3, 0, 2], value=value[:50], label="lp, a parameter, acceptance")
    idx = [3, 0, 2]
    assert np.allclose(sub[0], full[0][idx], rtol=1e-9, atol=0) and np.allclose(np.diag(sub[1]), np.diag(full[1])[idx], rtol=1e-9, atol=0)
    one = check(eng, 0, 50, [1], value=value[:50], label="K = 1")
    assert one[2][0, 0] == 1.0 and one[1].shape == (1, 1)
    # each output may be NULL, not all three
    L, C, h = eng.L, __import__("ctypes"), eng.h
    cov_only = np.empty((4, 4))
    assert L.demc_covariance(h, 0, 50, None, 4, None, cov_only.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
    assert cov_only.tobytes() == full[1].tobytes()


# ---- padded cells -----------------------------------------------------------------------------------------------------------------
def test_history_partners_pad_the_cells(demc):
    """D = 9 with partners from the history: cells are 16 doubles apart and the padding must not enter"""
    n = 20
    from test_quantile_host import hist_ld
    assert hist_ld(9, True) == 16
    check_geometry(n, 8, 9, 16, 11, blocks=1, chunks=1)
    eng, value = S.synthetic_engine(demc, n, 2, 4, 9, 0.5, 1, n_initial=3, partner_kind=1, scale=True)
    check(eng, 3, 3 + n, value=value, label="history partners D=9")
    eng.close()


# ---- cols over wide cells, and the widest call ------------------------------------------------------------------------------------------
def test_columns_spread_over_a_cell_wider_than_a_workgroup(demc):
    n, P, D = 3, 4, 600
    check_geometry(n, P, D, D, 64, tiles=10, chunks=1, idle_waves=5)
    rng = np.random.default_rng(600)
    rows = rng.normal(0.0, 1.0, (n, P, D)) * (1.0 + np.arange(D) / 64.0) + np.arange(D) % 7
    eng = plain_engine(demc, n, P, D, rows)
    cols = [int(c) for c in rng.permutation(np.linspace(0, D - 1, 63).astype(int))] + [D + 1]
    assert len(set(cols)) == 64 and 0 in cols and D - 1 in cols
    check(eng, 0, n, cols, label="64 of 602 series")
    eng.close()


def test_all_series_of_the_widest_handle_and_one_more(demc):
    n, P = 16, 8
    check_geometry(n, P, 62, 62, 64, tiles=10, chunks=1, workers=1)
    rng = np.random.default_rng(62)
    rows = rng.normal(0.0, 1.0, (n, P, 62))
    rows[:, :, 40] = 0.6 * rows[:, :, 3] - 0.8 * rows[:, :, 40]
    eng = plain_engine(demc, n, P, 62, rows)
    check(eng, 0, n, label="D + 2 = 64, cols = NULL")
    eng.close()
    eng = plain_engine(demc, n, P, 63, rng.normal(0.0, 1.0, (n, P, 63)))
    with pytest.raises(demc.DemcError) as e:
        eng.covariance(0, n)
    assert e.value.code == demc._ffi.EINVAL
    check(eng, 0, n, list(range(64)), label="64 of 65 series")
    eng.close()


# ---- launch geometry ------------------------------------------------------------------------------------------------------------------
GEOMETRY = {  # case: (n, P, D, what it is the smallest shape for)
    "one_full_chunk": (64, 8, 2, dict(chunks=1, workers=1, ragged_chunk=False, idle_waves=0)),
    "second_workgroup_ragged": (65, 8, 2, dict(chunks=2, workers=2, chunks_per_worker_max=1, ragged_chunk=True, idle_waves=6)),
    # the pool just past kCovMaxWorkers chunks: worker 0 walks a second chunk, and that chunk is ragged
    "second_chunk_D7": (32769, 8, 7, dict(chunks=513, workers=512, chunks_per_worker_max=2, ragged_chunk=True, blocks=1)),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_launch_geometry(demc, case):
    n, P, D, geo = GEOMETRY[case]
    check_geometry(n, P, D, D, D + 2, **geo)
    rng = np.random.default_rng(len(case))
    rows = rng.normal(0.0, 1.0, (n, P, D)) * (1.0 + np.arange(D) / 8.0) + np.arange(D) % 3
    rows[:, :, D - 1] += 0.9 * rows[:, :, 0]
    eng = plain_engine(demc, n, P, D, rows)
    got = check(eng, 0, n, label=case)
    again = eng.covariance(0, n)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    eng.close()


# ---- non-finite and constant ------------------------------------------------------------------------------------------------------------
def test_sign_and_edges(demc):
    """the layout of test_gpu_quantile.py's test of the same name, one more live series: a NaN in one series, both infinities in
    another, a constant 2.5 -- each confined to its row and column"""
    D, P, n = 5, 8, 16
    rng = np.random.default_rng(4)
    rows = np.empty((n, P, D))
    rows[:, :, 0] = rng.normal(0.0, 1.0, (n, P))
    edge = np.array([0.0, -0.0, 5e-324, -5e-324, np.inf, -np.inf, 1.0])
    rows[:, :, 1] = edge[np.arange(n * P) % len(edge)].reshape(n, P)
    rows[:, :, 2] = 2.5
    rows[:, :, 3] = rng.normal(0.0, 1.0, (n, P))
    rows[5, 3, 3] = np.nan
    rows[:, :, 4] = 0.5 * rows[:, :, 0] + rng.normal(0.0, 1.0, (n, P))
    eng = plain_engine(demc, n, P, D, rows)
    mean, cov, cor = check(eng, 0, n, list(range(D)), label="sign and edges")
    nanrow = np.zeros((D, D), bool)
    nanrow[[1, 3], :] = nanrow[:, [1, 3]] = True
    assert np.array_equal(np.isnan(cov), nanrow)
    nanrow[2, :] = nanrow[:, 2] = True
    assert np.array_equal(np.isnan(cor), nanrow)
    assert (cov[2, [0, 2, 4]] == 0.0).all() and (cov[[0, 2, 4], 2] == 0.0).all() and mean[2] == 2.5
    assert cor[0, 0] == cor[4, 4] == 1.0 and 0.2 < cor[0, 4] < 0.7 and np.isnan(mean[[1, 3]]).all()
    # one infinity alone, of either sign
    for bad in (np.inf, -np.inf):
        rows[:, :, 1] = rng.normal(0.0, 1.0, (n, P))
        rows[9, 2, 1] = bad
        eng.set_history_rows(0, rows)
        _, cov, _ = check(eng, 0, n, [4, 1, 0], label=f"a single {bad}")
        assert np.array_equal(np.isnan(cov), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool))
    eng.close()


def test_lp_that_never_becomes_finite(demc):
    """the configuration of test_gpu_quantile.py's test of the same name: four of twelve chains keep lp = -inf for the whole run, so
    lp has NaN in its row and column, and every other entry is finite and within the bar"""
    G, Np, n = 3, 4, 40
    prob = make_problem("gaussian", np.random.default_rng(7), N=50)
    eng = demc.HipEngine(n_groups=G, Np=Np, D=2, n_rows=n, schedule=2, seed=31, alpha=0.0, burnin=0)
    setup_engine(eng, prob)
    th = np.stack([np.random.default_rng(31).normal(0.3, 0.2, G * Np), np.random.default_rng(32).uniform(1.0, 1.5, G * Np)], 1)
    th[:Np, 1] = -1.0
    eng.set_state(th)
    eng.step(1, n)
    value = eng.export_chains(0, n)
    assert (value[:, 3, :Np] == -np.inf).all() and np.isfinite(value[:, 3, Np:]).all()
    mean, cov, cor = check(eng, 0, n, value=value, label="lp = -inf in four chains")
    want = np.zeros((4, 4), bool)
    want[3, :] = want[:, 3] = True
    assert np.array_equal(np.isnan(cov), want) and np.isnan(cor[3]).all() and np.isnan(mean[3]) and np.isfinite(mean[:3]).all()
    assert cor[0, 0] == cor[1, 1] == 1.0 and np.isfinite(cor[0, 1])
    eng.close()


# ---- invariants and errors --------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_history_stays(stepped):
    eng, _ = stepped
    before = list(eng.get_history(0, N_ROWS)) + list(eng.get_state())
    a = eng.covariance(0, N_ROWS)
    b = eng.covariance(0, N_ROWS)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    after = list(eng.get_history(0, N_ROWS)) + list(eng.get_state())
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_covariance_between_steps_changes_nothing(demc):
    states = []
    for split in (False, True):
        eng = S.gaussian_engine(demc, 3, 8, 40, 21)
        if split:
            eng.step(1, 20)
            eng.covariance(0, 20)
            eng.step(21, 20)
        else:
            eng.step(1, 40)
        states.append(list(eng.get_state()) + list(eng.get_history(0, 40)))
        eng.close()
    for x, y in zip(*states):
        assert x.tobytes() == y.tobytes()


def test_error_cases(demc):
    import ctypes as C
    E = demc._ffi.EINVAL
    eng = S.gaussian_engine(demc, 2, 4, 10, 1)
    eng.step(1, 10)
    for rows in ((-1, 5), (0, 11), (5, 5), (6, 5)):
        with pytest.raises(demc.DemcError) as e:
            eng.covariance(*rows)
        assert e.value.code == E, rows
    for cols in ([], list(range(4)) * 17, [4], [-1], [0, 1, 0], [0, 1, 2, 3, 3]):
        with pytest.raises(demc.DemcError) as e:
            eng.covariance(0, 10, cols)
        assert e.value.code == E, cols
    dp = C.POINTER(C.c_double)
    buf = np.empty(16)
    assert eng.L.demc_covariance(eng.h, 0, 10, None, 3, buf.ctypes.data_as(dp), None, None) == E  # cols == NULL: n_cols must be D + 2
    assert eng.L.demc_covariance(eng.h, 0, 10, None, 4, None, None, None) == E  # every output NULL
    assert eng.L.demc_covariance(eng.h, 0, 10, None, 4, buf.ctypes.data_as(dp), None, None) == 0
    assert eng.covariance(0, 10, [3, 2, 1, 0])[1].shape == (4, 4)
    eng.close()
    eng = S.gaussian_engine(demc, 2, 4, 10, 1, store_history=0)
    with pytest.raises(demc.DemcError) as e:
        eng.covariance(0, 5)
    assert e.value.code == E and "history" in str(e.value)
    eng.close()
    eng = S.gaussian_engine(demc, 2, 4, 10, 1, n_groups_total=4)
    with pytest.raises(demc.DemcError) as e:
        eng.covariance(0, 5)
    assert e.value.code == E and "sharded" in str(e.value)
    eng.close()


# ---- the public surface -----------------------------------------------------------------------------------------------------------
def test_summarize_with_cor_equals_sample_then_cor(demc):
    D = demc
    data = np.random.default_rng(50514).normal(0.0, 1.0, 50)

    def run(fn, **kw):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("μ", "σ"), data=data, prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)),
                          loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
        return fn(model, de, D.HIPBackend(seed=3), 300, **kw)

    summary = run(D.summarize, cor=True)
    plain = run(D.summarize)
    wide = run(D.summarize, cor=("lp", "μ", "acceptance"), quantiles=D.chains.DEFAULT_QUANTILES)
    chains = run(D.sample)
    N = chains.value.shape[0] * chains.value.shape[2]
    assert len(chains) == 200 and summary.cor()[0] == summary.cov()[0] == chains.cor()[0] == ["μ", "σ"]
    for s, names in ((summary, None), (wide, ("lp", "μ", "acceptance"))):
        cols = chains._cols(names)[1]
        want = R.restate(chains.value, cols)
        got = (want[0], s.cov()[1], s.cor()[1])  # (the Summary's means are demc_summarize's)
        errs = R.scaled_errors(got, want, N)
        print(f"summarize(cor={names or True}) against sample(): cov {errs[1]:.3g} scaled, cor {errs[2]:.3g}")
        assert max(errs) <= BAR
        host = (want[0], chains.cov(names)[1], chains.cor(names)[1])
        assert max(R.scaled_errors(host, want, N)) <= BAR
    assert wide.cor()[0] == ["lp", "μ", "acceptance"] and wide.quantiles.shape == (4, 5)
    assert summary.values.tobytes() == plain.values.tobytes() and plain.cor_matrix is None
    assert abs(summary.cor()[1][0, 1]) < 0.5 and summary.cor()[1][0, 0] == 1.0
