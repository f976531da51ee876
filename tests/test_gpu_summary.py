"""demc_summarize (include/demc_summary.h, csrc/demc_summary.hpp; the definition is DESIGN.md 5.5) on the GPU.  The reference input is always
export_chains of the same rows -- existing, tested code -- fed to the plain-loop restatement of tests/test_summary_host.py, or,
where plain loops would take minutes, to its vectorised form restate_np, which the host file holds to the plain loops at 1e-12.

Bars: rtol 1e-9 on mean / std / rhat / ess / mcse (the project's log-posterior bar), atol 1e-9 on rho_t, `pairs` and the NaN
pattern exactly.  With centred sums, h <= 1000 and |mean| / sd <= 100 the rounding bound is of order h eps 100 = 1e-11.  Every
reference series is also held to the margin condition of the host file (no pair within 1e-6 of zero): a failure there asks for
another seed, not for a skip.  Each test prints the maxima it saw."""
import math

import numpy as np
import pytest

import test_summary_host as R
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu
COLS = ("mean", "std", "rhat", "ess", "mcse")
RTOL, ATOL_RHO = 1e-9, 1e-9


def compare(out, rho, value, max_lag=0, label="", restate=R.restate):
    """device (out[D+2][6], rho[D+2][rho_len] or None) against the restatement of value[n][D+2][P]; returns the restatements"""
    rho_len = 0 if rho is None else rho.shape[1]
    refs = [restate(value[:, j, :], max_lag, rho_len) for j in range(value.shape[1])]
    worst, worst_rho = 0.0, 0.0
    for j, r in enumerate(refs):
        for k, col in enumerate(COLS):
            got, want = float(out[j, k]), r[col]
            assert math.isnan(got) == math.isnan(want), (label, j, col, got, want)
            if not math.isnan(want):
                err = 0.0 if got == want else abs(got - want) / abs(want)
                worst = max(worst, err)
                assert err <= RTOL, (label, j, col, got, want)
        assert out[j, 5] == r["pairs"], (label, j, out[j, 5], r["pairs"])
        if r["pmin"] is not None:
            assert r["pmin"] >= R.MARGIN, f"{label}: series {j} has a pair {r['pmin']:.3g} from zero -- choose another seed"
        if rho is not None:
            want = np.array(r["rho"])
            assert np.array_equal(np.isnan(rho[j]), np.isnan(want)), (label, j, rho[j], want)
            ok = ~np.isnan(want)
            if ok.any():
                worst_rho = max(worst_rho, float(np.abs(rho[j][ok] - want[ok]).max()))
            assert worst_rho <= ATOL_RHO, (label, j)
    print(f"{label}: max relative error {worst:.3g}, max |rho error| {worst_rho:.3g}")
    return refs


def gaussian_engine(demc, G, Np, n_rows, seed, alpha=0.5, **kw):
    prob = make_problem("gaussian", np.random.default_rng(7), N=50)
    eng = demc.HipEngine(n_groups=G, Np=Np, D=2, n_rows=n_rows, schedule=2, seed=seed, alpha=alpha, burnin=0, **kw)
    setup_engine(eng, prob)
    eng.set_state(np.stack([np.random.default_rng(seed).normal(0.3, 0.2, G * Np), np.random.default_rng(seed + 1).uniform(1.0, 1.5, G * Np)], 1))
    return eng


# ---- sampler-made history ------------------------------------------------------------------------------------------------------
N_EDGES = [1, 2, 3, 7, 8, 9, 65, 129]


@pytest.fixture(scope="module", params=[(2, 4, 11), (3, 23, 12)], ids=["8chains", "69chains"])
def stepped(request, demc):
    G, Np, seed = request.param
    eng = gaussian_engine(demc, G, Np, max(N_EDGES), seed)
    eng.step(1, max(N_EDGES))
    idh = eng.get_history(0, max(N_EDGES))[3]
    assert any(not np.array_equal(row, np.arange(G * Np)) for row in idh), "ids never left their slots: the re-key is not exercised"
    value = eng.export_chains(0, max(N_EDGES))
    value.setflags(write=False)
    yield eng, value
    eng.close()


@pytest.mark.parametrize("n", N_EDGES)
def test_sampler_made_history(stepped, n):
    eng, value = stepped
    out, rho = eng.summarize(0, n, rho_len=70)
    compare(out, rho, value[:n], label=f"sampler-made n={n} P={value.shape[2]}")
    h = n // 2
    for j in range(value.shape[1]):  # NaNs where the definition says, and nowhere else (no series of these runs is constant)
        assert np.isfinite(out[j, 0])
        assert np.isfinite(out[j, 1]) == (n * value.shape[2] > 1)
        assert np.isfinite(out[j, 2]) == (h >= 2), (j, out[j])
        assert np.isfinite(out[j, 3]) == (h >= 4) and np.isfinite(out[j, 4]) == (h >= 4), (j, out[j])
        assert np.isnan(rho[j]).all() == (h < 2)


def test_rows_need_not_start_at_zero(stepped):
    eng, value = stepped
    out, rho = eng.summarize(40, 129, rho_len=10)
    compare(out, rho, value[40:129], label="rows 40..129")


# ---- synthetic theta written over the stepped rows ------------------------------------------------------------------------------
def synthetic_engine(demc, n, G, Np, D, phi, seed, const_col=None, n_initial=0, scale=False, **kw):
    """an engine stepped n times with ids away from their slots, its theta history then overwritten so that CHAIN (id) c of
    parameter j is the AR(1) input of the host file with seed (seed + j) % 3 -> (engine, first row).  scale: series j times
    (1 + j / 8), so that series j and j + 3, fed by the same seed, have a mean and a std of their own"""
    P = G * Np
    rng = np.random.default_rng(100 + seed)
    fam = {1: "binomial", 2: "gaussian"}.get(D, "mvn_iso")
    prob = make_problem(fam, rng, **({"d": D - 1} if fam == "mvn_iso" else {}))
    eng = demc.HipEngine(n_groups=G, Np=Np, D=D, n_rows=n + n_initial, seed=40 + seed, alpha=0.5, burnin=0, n_initial=n_initial,
                         schedule=2 if Np >= 4 else 1, **kw)
    setup_engine(eng, prob)
    if n_initial:
        eng.set_history_rows(0, np.stack([prob["init"](P) for _ in range(n_initial)]))
    eng.set_state(prob["init"](P), ids=(np.arange(P) + 1) % P)  # even a single group keeps its ids away from their slots
    eng.step(1 + n_initial, n)
    idh = eng.get_history(n_initial, n_initial + n)[3]
    assert any(not np.array_equal(row, np.arange(P)) for row in idh)
    base = [R.ar1(n, P, phi, (seed + j) % 3) for j in range(min(D, 3))]
    by_id = np.stack([R.scaled(base[j % 3], j) if scale else base[j % 3] for j in range(D)], axis=2)  # [n][id][D]
    if const_col is not None:
        by_id[:, :, const_col] = 2.5
    eng.set_history_rows(n_initial, np.take_along_axis(by_id, idh[:, :, None], axis=1))  # slot-keyed: row i, slot s holds id idh[i][s]
    value = eng.export_chains(n_initial, n_initial + n)
    assert np.array_equal(value[:, :D, :], np.transpose(by_id, (0, 2, 1)))
    return eng, value


SYNTH = [  # the AR(1) cases of the host file: (n, m, phi) with m = G Np chains, and the D that goes with each
    (64, 1, 4, 1, 0.0), (65, 1, 4, 5, 0.9), (129, 1, 3, 33, -0.5), (200, 2, 4, 2, 0.5)]


@pytest.mark.parametrize("n,G,Np,D,phi", SYNTH)
def test_synthetic_ar1(demc, n, G, Np, D, phi):
    assert (n, G * Np, phi) in R.AR1_CASES
    const = 1 if D == 2 else None
    eng, value = synthetic_engine(demc, n, G, Np, D, phi, 0, const_col=const)
    out, rho = eng.summarize(0, n, rho_len=70)
    compare(out, rho, value, label=f"AR(1) n={n} m={G * Np} phi={phi} D={D}")
    if const is not None:  # the constant column: std 0, rhat / ess / mcse NaN
        assert out[const, 0] == 2.5 and out[const, 1] == 0.0 and np.isnan(out[const, 2:5]).all() and out[const, 5] == 0.0
    eng.close()


def test_history_partners_pad_the_cells(demc):
    """D = 9 with partners from the history: cells are 16 doubles apart, not 9, and the kept rows start behind the initial ones"""
    eng, value = synthetic_engine(demc, 200, 2, 4, 9, 0.5, 1, n_initial=3, partner_kind=1)
    out, rho = eng.summarize(3, 203, rho_len=70)
    compare(out, rho, value, label="history partners D=9")
    eng.close()


@pytest.fixture(scope="module")
def slow_mixing(demc):
    """(1000, 16, 0.95): the case whose sequence runs over more than one block of lags"""
    eng, value = synthetic_engine(demc, 1000, 4, 4, 1, 0.95, 0)
    value.setflags(write=False)
    yield eng, value
    eng.close()


def test_synthetic_ar1_slow_mixing(slow_mixing):
    eng, value = slow_mixing
    out, rho = eng.summarize(0, 1000, rho_len=200)
    refs = compare(out, rho, value, label="AR(1) n=1000 m=16 phi=0.95")
    assert refs[0]["pairs"] > 32, "the sequence was meant to cross a block of 64 lags"


def test_max_lag(slow_mixing):
    eng, value = slow_mixing
    out, rho = eng.summarize(0, 1000, max_lag=16, rho_len=40)
    refs = compare(out, rho, value, max_lag=16, label="max_lag=16")
    assert out[0, 5] == 8.0 and refs[0]["pairs"] == 8.0  # cut by the cap: K == (L + 1) // 2
    assert not np.isnan(rho[0, :17]).any() and np.isnan(rho[:, 17:]).all()
    full = eng.summarize(0, 1000, max_lag=0, rho_len=200)
    for cap in (499, 500, 10**6):  # max_lag >= h - 1 is no cap
        other = eng.summarize(0, 1000, max_lag=cap, rho_len=200)
        assert np.array_equal(full[0], other[0], equal_nan=True) and np.array_equal(full[1], other[1], equal_nan=True)
    assert out[0, 3] != full[0][0, 3]


# ---- series that leave the small LDS tile -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8064, 8065, 18304, 18305])
def test_long_series(demc, n):
    """n = 8064 is the longest series that fits the 64 KiB tile, 18304 the longest that is staged in LDS at all; one row more
    takes the next path (a 144 KiB tile, a global one).  Nothing is stepped: the rows hold what they were created with
    (acceptance and lp are constant: NaN), theta is AR(1)."""
    P = 4
    eng = demc.HipEngine(n_groups=1, Np=P, D=1, n_rows=n, seed=1)
    eng.set_history_rows(0, R.ar1(n, P, 0.5, 1)[:, :, None])
    value = eng.export_chains(0, n)
    out, rho = eng.summarize(0, n, rho_len=8)
    compare(out, rho, value, label=f"long series n={n}")
    assert np.isfinite(out[0]).all() and np.isnan(out[1:, 2:5]).all()
    eng.close()


# ---- past the smallest launch geometry: a worker's second chain, ragged series tiles, strides of the reducing kernels -------------
def check_geometry(n, P, D, **want):
    g = R.geometry(n, P, D)
    for k, v in want.items():
        assert g[k] == v, f"n={n} P={P} D={D}: {k} is {g[k]}, the case was chosen for {v} -- the constants of csrc/demc_summary.hpp moved"
    return g


LARGE = {  # case: (n, G, Np, D, phi, the geometry it is the smallest shape for, the reference)
    # workers = P exactly; M = 2048 and 1024 workers make k_sum_means stride over both
    "a": (16, 32, 32, 2, 0.5, dict(mode="lds64", JT=4, tiles=[4], workers=1024, chains_per_worker_max=1, lag_blocks=1), R.restate),
    # worker 0 takes two chains, the others one; tiles of 8 and 1 series
    "b": (16, 41, 25, 7, 0.5, dict(mode="lds64", JT=8, tiles=[8, 1], workers=1024, chains_per_worker_max=2, lag_blocks=1), R.restate),
    # the same with h = 65, L = 64: block 1 holds lag 64 alone and no pair
    "c": (130, 41, 25, 7, 0.9, dict(mode="lds64", JT=8, tiles=[8, 1], workers=1024, chains_per_worker_max=2, lag_blocks=2), R.restate_np),
    # four chains per worker, at the population DESIGN.md 5.5 times
    "d": (130, 64, 64, 7, 0.9, dict(mode="lds64", JT=8, tiles=[8, 1], workers=1024, chains_per_worker_max=4, lag_blocks=2), R.restate_np),
    "e": (2000, 2, 4, 2, 0.5, dict(mode="lds64", JT=3, tiles=[3, 1], workers=8, chains_per_worker_max=1, lag_blocks=16), R.restate),
    "f": (3900, 2, 4, 3, 0.5, dict(mode="lds64", JT=2, tiles=[2, 2, 1], workers=8, chains_per_worker_max=1, lag_blocks=31), R.restate),
}


@pytest.mark.parametrize("case", sorted(LARGE))
def test_beyond_one_chain_per_worker_and_one_tile(demc, case):
    """Each case asserts the geometry it was chosen for (R.geometry restates summary_run's rule; the host file holds its constants to
    the header).  References: plain-loop restate for a, b, e and f; restate_np for c and d, where plain loops over 130 rows of a
    thousand chains and more take seconds per series.  Series are scaled by (1 + j / 8) where D > 3.  b and d are run twice: a race on the tile that a worker reuses for
    its next chain shows in the bits first."""
    n, G, Np, D, phi, geo, restate = LARGE[case]
    assert (n, G * Np, phi) in R.AR1_LARGE and R.LARGE_SCALED.get((n, G * Np, phi), 0) == (D if D > 3 else 0)
    check_geometry(n, G * Np, D, **geo)
    eng, value = synthetic_engine(demc, n, G, Np, D, phi, 0, scale=D > 3)
    out, rho = eng.summarize(0, n, rho_len=70)
    compare(out, rho, value, label=f"case {case}: n={n} P={G * Np} D={D}", restate=restate)
    if case == "c":  # every pair of [0, L] is kept: the sequence is cut by the end of the half, in a block that holds no pair
        L = n // 2 - 1
        assert L == 64 and (out[:D, 5] == (L + 1) // 2).all(), out[:, 5]
        assert np.isfinite(rho[:D, :L + 1]).all() and np.isnan(rho[:, L + 1:]).all()
    if case in "bd":
        again = eng.summarize(0, n, rho_len=70)
        assert out.tobytes() == again[0].tobytes() and rho.tobytes() == again[1].tobytes()
    eng.close()


def test_global_tile_worker_takes_two_chains(demc):
    """case g: 64 chains of n = 18305 rows, D = 6: the global-tile budget leaves 57 workers, so seven of them stage a second chain in
    the tile they used for the first.  Built as test_long_series is (nothing stepped, theta written by set_history_rows, acceptance
    and lp constant).  Reference: restate_np."""
    n, P, D = 18305, 64, 6
    assert (n, P, 0.5) in R.AR1_LARGE and R.LARGE_SCALED[(n, P, 0.5)] == D
    check_geometry(n, P, D, mode="global", JT=1, tiles=[1] * 8, workers=57, chains_per_worker_max=2)
    eng = demc.HipEngine(n_groups=1, Np=P, D=D, n_rows=n, seed=1)
    base = [R.ar1(n, P, 0.5, s) for s in R.SEEDS]
    eng.set_history_rows(0, np.stack([R.scaled(base[j % 3], j) for j in range(D)], axis=2))
    value = eng.export_chains(0, n)
    out, rho = eng.summarize(0, n, rho_len=8)
    compare(out, rho, value, label=f"case g: n={n} P={P} D={D}", restate=R.restate_np)
    assert np.isfinite(out[:D]).all() and np.isnan(out[D:, 2:5]).all()
    eng.close()


@pytest.mark.parametrize("D,kw", [(63, {}), (63, dict(partner_kind=1, n_initial=3)), (70, {})], ids=["D63", "D63-padded", "D70"])
def test_more_than_64_series(demc, D, kw):
    """case h: D + 2 = 65 and 72 series: the second workgroup of k_sum_final (and nine series tiles); with partners from the history
    the cells of D = 63 are 64 doubles apart.  Reference: plain-loop restate."""
    n, G, Np = 16, 2, 4
    assert (n, G * Np, 0.5) in R.AR1_LARGE and R.LARGE_SCALED[(n, G * Np, 0.5)] >= D
    g = check_geometry(n, G * Np, D, mode="lds64", JT=8, workers=8, chains_per_worker_max=1, lag_blocks=1)
    assert len(g["tiles"]) == 9 and D + 2 > 64
    eng, value = synthetic_engine(demc, n, G, Np, D, 0.5, 0, scale=True, **kw)
    r0 = kw.get("n_initial", 0)
    out, rho = eng.summarize(r0, r0 + n, rho_len=10)
    compare(out, rho, value, label=f"case h: D={D} {kw}")
    assert np.isfinite(out[:D]).all()
    eng.close()


@pytest.mark.parametrize("max_lag", [63, 64, 65, 127, 128])
def test_lag_cap_at_a_block_edge(slow_mixing, max_lag):
    """L = 63: the cap ends block 0 with its last pair; L = 64: block 1 holds one lag and no pair; L = 65: exactly one pair.  127 /
    128 are the same edge one block on: this input's sequence ends by itself in block 1 (34 pairs), so the cap only bounds the
    lags that block reports, and at 128 a third block is launched for series that have all ended.  Reference: plain-loop restate."""
    eng, value = slow_mixing
    L = max_lag
    out, rho = eng.summarize(0, 1000, max_lag=max_lag, rho_len=200)
    refs = compare(out, rho, value, max_lag=max_lag, label=f"max_lag={max_lag}")
    if max_lag <= 65:  # the cap cuts the sequence
        assert out[0, 5] == (L + 1) // 2 == refs[0]["pairs"] == {63: 32, 64: 32, 65: 33}[max_lag]
        assert np.isfinite(rho[0, :L + 1]).all()
    assert np.isnan(rho[:, L + 1:]).all()


def test_lp_that_never_becomes_finite(demc):
    """Group 0 starts with sigma = -1 in all four particles and alpha = 0: every proposal of the group is -1 + gamma * 0 + b with
    |b| <= 1e-3, out of bounds, so its lp stays -inf and nothing is accepted for the whole run.  The lp series then has mean -inf
    and NaN for std / rhat / ess / mcse, no pair, rho_0 = 1; the other series stay finite.  Reference: plain-loop restate."""
    G, Np, n = 3, 4, 40
    prob = make_problem("gaussian", np.random.default_rng(7), N=50)
    eng = demc.HipEngine(n_groups=G, Np=Np, D=2, n_rows=n, schedule=2, seed=31, alpha=0.0, burnin=0)
    setup_engine(eng, prob)
    th = np.stack([np.random.default_rng(31).normal(0.3, 0.2, G * Np), np.random.default_rng(32).uniform(1.0, 1.5, G * Np)], 1)
    th[:Np, 1] = -1.0
    eng.set_state(th)
    eng.step(1, n)
    value = eng.export_chains(0, n)
    assert (value[:, 3, :Np] == -np.inf).all() and (value[:, 2, :Np] == 0.0).all() and (value[:, 1, :Np] == -1.0).all()
    assert np.isfinite(value[:, 3, Np:]).all() and value[:, 2, Np:].any()
    out, rho = eng.summarize(0, n, rho_len=30)
    compare(out, rho, value, label="lp = -inf in four chains")
    assert out[3, 0] == -np.inf and np.isnan(out[3, 1:5]).all() and out[3, 5] == 0.0
    assert rho[3, 0] == 1.0 and np.isnan(rho[3, 1:]).all()
    assert np.isfinite(out[:3]).all() and np.isfinite(rho[:3, :20]).all()
    eng.close()


# ---- invariants -------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_history_stays(stepped):
    eng, _ = stepped
    before = eng.get_history(0, 129)
    a = eng.summarize(0, 129, rho_len=70)
    b = eng.summarize(0, 129, rho_len=70)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    after = eng.get_history(0, 129)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_summarize_between_steps_changes_nothing(demc):
    states = []
    for split in (False, True):
        eng = gaussian_engine(demc, 3, 8, 40, 21)
        if split:
            eng.step(1, 20)
            eng.summarize(0, 20, rho_len=8)
            eng.step(21, 20)
        else:
            eng.step(1, 40)
        states.append(list(eng.get_state()) + list(eng.get_history(0, 40)))
        eng.close()
    for x, y in zip(*states):
        assert x.tobytes() == y.tobytes()


def test_error_cases(demc):
    E = demc._ffi.EINVAL
    eng = gaussian_engine(demc, 2, 4, 10, 1)
    eng.step(1, 10)
    for rows in ((-1, 5), (0, 11), (5, 5), (6, 5)):
        with pytest.raises(demc.DemcError) as e:
            eng.summarize(*rows)
        assert e.value.code == E, rows
    eng.close()
    eng = gaussian_engine(demc, 2, 4, 10, 1, store_history=0)
    with pytest.raises(demc.DemcError) as e:
        eng.summarize(0, 5)
    assert e.value.code == E and "history" in str(e.value)
    eng.close()
    eng = gaussian_engine(demc, 2, 4, 10, 1, n_groups_total=4)
    with pytest.raises(demc.DemcError) as e:
        eng.summarize(0, 5)
    assert e.value.code == E and "sharded" in str(e.value)
    eng.close()


# ---- the public surface -----------------------------------------------------------------------------------------------------------
def test_summarize_equals_sample_then_summarystats(demc):
    D = demc
    data = np.random.default_rng(50514).normal(0.0, 1.0, 50)

    def run(fn):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("μ", "σ"), data=data, prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)),
                          loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
        return fn(model, de, D.HIPBackend(seed=3), 300)

    summary = run(D.summarize)
    chains = run(D.sample)
    assert len(chains) == 200
    host = chains.summarystats()
    assert summary.names == host.names == ["μ", "σ", "acceptance", "lp"]
    worst = 0.0
    for j in range(4):
        for k in range(5):
            a, b = summary.values[j, k], host.values[j, k]
            assert np.isfinite(a) and np.isfinite(b)
            worst = max(worst, abs(a - b) / abs(b))
        assert summary.values[j, 5] == host.values[j, 5]
    print(f"summarize vs sample + summarystats: max relative error {worst:.3g}")
    assert worst <= RTOL
    d, ref = summary.describe(), chains.describe()
    assert set(d) == set(ref) == {"μ", "σ"}
    for nm in ref:
        assert set(d[nm]) == {"mean", "std", "rhat", "ess", "mcse", "pairs"}
        for col in ("mean", "std", "rhat"):
            assert abs(d[nm][col] - ref[nm][col]) <= RTOL * abs(ref[nm][col]), (nm, col)
