"""demc_quantiles (include/demc_quantile.h, csrc/demc_quantile.hpp; the definition is DESIGN.md 5.6) on the GPU.  The reference is always
export_chains of the same rows -- existing, tested code -- flattened per series and fed to the plain-loop restatement of
tests/test_quantile_host.py.  The bar is equality of bits, the NaN pattern included: the selection is exact and the interpolation
is the expression of the definition.  Default probs plus 0, 1 and 1/3 unless a case says otherwise."""
import math

import numpy as np
import pytest

import test_gpu_summary as S  # gaussian_engine, synthetic_engine: the engines of the summary's GPU tests
import test_quantile_host as R
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu
PROBS = R.PROBS


def check(eng, row0, row1, probs=PROBS, label="", value=None):
    """device against the restatement of the exported rows, bit for bit -> (device table, reference table)"""
    if value is None:
        value = eng.export_chains(row0, row1)
    want = R.restate_all(value, probs)
    got = eng.quantiles(row0, row1, probs)
    assert got.shape == want.shape == (value.shape[1], len(probs))
    bad = [(j, k, got[j, k], want[j, k]) for j in range(got.shape[0]) for k in range(got.shape[1]) if not R.same_bits(got[j, k], want[j, k])]
    assert not bad, f"{label}: {len(bad)} of {got.size} differ, first (series, prob, device, restatement): {bad[:4]}"
    return got, want


def check_geometry(n, P, D, ld, probs=PROBS, **want):
    g = R.geometry(n, P, D, ld, probs)
    for k, v in want.items():
        assert g[k] == v, f"n={n} P={P} D={D} ld={ld}: {k} is {g[k]}, the case was chosen for {v} -- the constants of csrc/demc_quantile.hpp moved"
    return g


def plain_engine(demc, n, P, D, rows, **kw):
    """nothing stepped: theta written by set_history_rows, acceptance and lp as they were created"""
    eng = demc.HipEngine(n_groups=1, Np=P, D=D, n_rows=n, seed=1, **kw)
    eng.set_history_rows(0, rows)
    return eng


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


@pytest.mark.parametrize("n", [1, 2, 3, 7, 129])
def test_sampler_made_history(stepped, n):
    eng, value = stepped
    got, _ = check(eng, 0, n, value=value[:n], label=f"sampler-made n={n} P={value.shape[2]}")
    assert np.isfinite(got).all()
    acc = value[:n, 2, :]
    assert set(np.unique(acc)) <= {0.0, 1.0}  # acceptance: a pool of ties
    assert set(np.unique(got[2, [5, 6]])) <= {0.0, 1.0} and got[2, 5] == acc.min() and got[2, 6] == acc.max()


def test_rows_need_not_start_at_zero(stepped):
    eng, value = stepped
    check(eng, 40, 129, value=value[40:129], label="rows 40..129")


# ---- every digit position -------------------------------------------------------------------------------------------------------
def test_targets_part_at_every_bit(demc):
    """series s holds the four values bits = 0x0010000000000000 ^ (k << s), k = 0 .. 3, with seeded random multiplicities: the keys
    of a series agree above bit s + 1, so adjacent targets share their prefix through every digit above and part at bit s or
    s + 1 -- for every s = 0 .. 61, i.e. inside every digit and across every digit boundary.  D + 2 = 64 series: one LDS table each."""
    D, P, n = 62, 8, 16
    check_geometry(n, P, D, D, first_pass_slots=64, first_pass_direct=0, cells_per_chunk=8, chunks=16, workgroups=16)
    rng = np.random.default_rng(62)
    rows = np.empty((n, P, D), dtype=np.uint64)
    for s in range(D):
        mult = 1 + rng.multinomial(n * P - 4, [0.25] * 4)
        ks = rng.permutation(np.repeat(np.arange(4, dtype=np.uint64), mult))
        rows[:, :, s] = (np.uint64(0x0010000000000000) ^ (ks << np.uint64(s))).reshape(n, P)
    rows = rows.view(np.float64)
    assert np.isfinite(rows).all()
    eng = plain_engine(demc, n, P, D, rows)
    value = eng.export_chains(0, n)
    assert np.array_equal(np.transpose(value[:, :D, :], (0, 2, 1)).view(np.uint64), rows.view(np.uint64))
    got, want = check(eng, 0, n, value=value, label="every digit position")
    for s in range(D):  # the selected values differ: the targets did part
        assert len(set(got[s, [5, 6]].view(np.uint64).tolist())) == 2, s
    eng.close()


# ---- sign and edges -------------------------------------------------------------------------------------------------------------
def test_sign_and_edges(demc):
    D, P, n = 4, 8, 16
    rng = np.random.default_rng(4)
    rows = np.empty((n, P, D))
    rows[:, :, 0] = rng.normal(0.0, 1.0, (n, P))
    edge = np.array([0.0, -0.0, 5e-324, -5e-324, np.inf, -np.inf, 1.0])
    rows[:, :, 1] = edge[np.arange(n * P) % len(edge)].reshape(n, P)
    rows[:, :, 2] = 2.5
    rows[:, :, 3] = rng.normal(0.0, 1.0, (n, P))
    rows[5, 3, 3] = np.nan
    eng = plain_engine(demc, n, P, D, rows)
    got, want = check(eng, 0, n, label="sign and edges")
    assert (got[0] < 0).any() and (got[0] > 0).any() and np.isfinite(got[0]).all()
    assert not np.isnan(got[:3]).any() and np.isnan(got[3]).all() and not np.isnan(got[4:]).any()
    assert got[1, 5] == -np.inf and got[1, 6] == np.inf and (got[2] == 2.5).all()
    zeros = eng.quantiles(0, n, [0.45, 0.55])[1]  # the pool's middle: the signed zeros and the subnormals keep their bits
    assert R.same_bits(zeros, R.restate(rows[:, :, 1].reshape(-1).tolist(), [0.45, 0.55]))
    # a NaN with the sign set sorts before -inf: the same rule
    rows[5, 3, 3] = R.from_bits(0xFFF8000000000001)
    rows[2, 1, 0] = R.from_bits(0xFFF8000000000001)
    eng.set_history_rows(0, rows)
    got, _ = check(eng, 0, n, label="negative NaN")
    assert np.isnan(got[0]).all() and np.isnan(got[3]).all() and not np.isnan(got[1:3]).any()
    eng.close()


def test_lp_that_never_becomes_finite(demc):
    """the configuration of test_gpu_summary.py's test of the same name: four of twelve chains keep lp = -inf for the whole run, so
    the low quantiles of lp are -inf, the upper ones finite, none NaN"""
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
    got, _ = check(eng, 0, n, R.DEFAULT, value=value, label="lp = -inf in four chains")
    assert (got[3, :2] == -np.inf).all() and np.isfinite(got[3, 2:]).all() and not np.isnan(got).any()
    assert np.isfinite(got[:3]).all()
    eng.close()


def test_history_partners_pad_the_cells(demc):
    """D = 9 with partners from the history: cells are 16 doubles apart and the padding must not enter a pool"""
    n = 20
    assert R.hist_ld(9, True) == 16
    check_geometry(n, 8, 9, 16, cells_per_chunk=32, busy_lanes=512)
    eng, value = S.synthetic_engine(demc, n, 2, 4, 9, 0.5, 1, n_initial=3, partner_kind=1)
    check(eng, 3, 3 + n, value=value, label="history partners D=9")
    eng.close()


# ---- geometry -------------------------------------------------------------------------------------------------------------------
GEOMETRY = {  # case: (n, P, D, what it is the smallest shape for)
    # 128 cells of 7 doubles: two chunks of 73 cells (one idle lane), the second ragged; two workgroups add into every histogram
    "two_workgroups_D7": (16, 8, 7, dict(cells_per_chunk=73, busy_lanes=511, chunks=2, workgroups=2, chunks_per_wg_max=1, ragged=True)),
    # 15 cells of 33 doubles per chunk (17 idle lanes); 513 chunks: workgroup 0 walks a second chunk, and that chunk is ragged
    "second_chunk_D33": (961, 8, 33, dict(cells_per_chunk=15, busy_lanes=495, chunks=513, workgroups=512, chunks_per_wg_max=2, ragged=True)),
    # 72 series for 64 tables: at least eight are counted in the global table in the first pass, and later passes hold 64 of 72 T groups
    "more_series_than_tables_D70": (4, 8, 70, dict(first_pass_slots=64, first_pass_direct=8, later_slots=64, chunks=5, ragged=True)),
    # a cell wider than the workgroup: two blocks of columns
    "column_blocks_D600": (3, 4, 600, dict(cells_per_chunk=1, busy_lanes=512, chunks=12, workgroups=12, first_pass_direct=538)),
    # one workgroup, one full chunk
    "one_chunk_D2": (32, 8, 2, dict(cells_per_chunk=256, chunks=1, workgroups=1, ragged=False, first_pass_slots=4, later_slots=64)),
}


@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_launch_geometry(demc, case):
    n, P, D, geo = GEOMETRY[case]
    check_geometry(n, P, D, D, **geo)
    rng = np.random.default_rng(len(case))
    rows = rng.normal(0.0, 1.0, (n, P, D)) * (1.0 + np.arange(D) / 8.0) + np.arange(D) % 3
    rows[:, :, D // 2] = np.round(rows[:, :, D // 2])  # ties
    eng = plain_engine(demc, n, P, D, rows)
    got, _ = check(eng, 0, n, label=case)
    if case == "second_chunk_D33":
        again = eng.quantiles(0, n, PROBS)
        assert got.tobytes() == again.tobytes()
    eng.close()


# ---- probs ----------------------------------------------------------------------------------------------------------------------
def test_one_prob_and_sixteen(stepped):
    eng, value = stepped
    for p in (0.5, 0.0, 1.0):
        check(eng, 0, 50, [p], value=value[:50], label=f"n_probs=1 p={p}")
    probs = [0.975, 0.9, 0.75, 0.75, 0.5, 0.5, 0.5, 0.25, 0.1, 0.025, 1.0, 0.0, 0.0, 1.0 / 3.0, 0.999, 0.001]
    assert len(probs) == 16
    got, _ = check(eng, 0, 50, probs, value=value[:50], label="n_probs=16")
    assert R.same_bits(got[:, 2], got[:, 3]) and R.same_bits(got[:, 4], got[:, 6]) and R.same_bits(got[:, 11], got[:, 12])


# ---- invariants and errors --------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_history_stays(stepped):
    eng, _ = stepped
    before = eng.get_history(0, N_ROWS)
    a = eng.quantiles(0, N_ROWS, PROBS)
    b = eng.quantiles(0, N_ROWS, PROBS)
    assert a.tobytes() == b.tobytes()
    after = eng.get_history(0, N_ROWS)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_quantiles_between_steps_changes_nothing(demc):
    states = []
    for split in (False, True):
        eng = S.gaussian_engine(demc, 3, 8, 40, 21)
        if split:
            eng.step(1, 20)
            eng.quantiles(0, 20, PROBS)
            eng.step(21, 20)
        else:
            eng.step(1, 40)
        states.append(list(eng.get_state()) + list(eng.get_history(0, 40)))
        eng.close()
    for x, y in zip(*states):
        assert x.tobytes() == y.tobytes()


def test_error_cases(demc):
    E = demc._ffi.EINVAL
    eng = S.gaussian_engine(demc, 2, 4, 10, 1)
    eng.step(1, 10)
    for rows in ((-1, 5), (0, 11), (5, 5), (6, 5)):
        with pytest.raises(demc.DemcError) as e:
            eng.quantiles(*rows, R.DEFAULT)
        assert e.value.code == E, rows
    for probs in ([], [0.5] * 17, [-0.1], [0.5, 1.1], [0.5, math.nan]):
        with pytest.raises(demc.DemcError) as e:
            eng.quantiles(0, 10, probs)
        assert e.value.code == E, probs
    assert eng.quantiles(0, 10, [0.5] * 16).shape == (4, 16)
    eng.close()
    eng = S.gaussian_engine(demc, 2, 4, 10, 1, store_history=0)
    with pytest.raises(demc.DemcError) as e:
        eng.quantiles(0, 5, R.DEFAULT)
    assert e.value.code == E and "history" in str(e.value)
    eng.close()
    eng = S.gaussian_engine(demc, 2, 4, 10, 1, n_groups_total=4)
    with pytest.raises(demc.DemcError) as e:
        eng.quantiles(0, 5, R.DEFAULT)
    assert e.value.code == E and "sharded" in str(e.value)
    eng.close()


# ---- the public surface -----------------------------------------------------------------------------------------------------------
def test_summarize_with_quantiles_equals_sample_then_quantile(demc):
    D = demc
    data = np.random.default_rng(50514).normal(0.0, 1.0, 50)

    def run(fn, **kw):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("μ", "σ"), data=data, prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)),
                          loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
        return fn(model, de, D.HIPBackend(seed=3), 300, **kw)

    probs = D.chains.DEFAULT_QUANTILES
    summary = run(D.summarize, quantiles=probs)
    plain = run(D.summarize)
    chains = run(D.sample)
    assert len(chains) == 200 and summary.names == ["μ", "σ", "acceptance", "lp"] and summary.probs == probs
    assert summary.quantile() == chains.quantile() and set(summary.quantile()) == {"μ", "σ"}
    for j in range(4):  # the internals too, and against the restatement
        assert R.same_bits(summary.quantiles[j], R.restate(chains.value[:, j, :].reshape(-1).tolist(), probs)), j
    assert summary.values.tobytes() == plain.values.tobytes() and plain.quantiles is None
    lo, mid, hi = (summary.quantile()["μ"][q] for q in (0.025, 0.5, 0.975))
    assert lo < mid < hi and lo < chains.mean()["μ"] < hi
