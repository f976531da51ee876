"""demc_rankstats and demc_rank_series (include/demc_rank.h, csrc/demc_rank.{hpp,cpp}; the definition is DESIGN.md 5.11) on the GPU.

demc_rank_series is where the sort is held to the definition BIT FOR BIT: the ranks of a series (kind 0) and of |x - med| (kind 2)
against chains.series_ranks of the same slot-keyed rows read back with get_history; the normal scores (kind 1) at the measured bar of
the inverse normal (tests/test_rank_host.py: four times the largest error against mpmath).  Every case asserts through geometry()
the path it is there for.  demc_rankstats is held to the plain-loop restatement of tests/test_rank_host.py applied to export_chains
of the same rows: rtol 1e-9 on every R-hat and ESS (DESIGN.md 5.5's bar: nothing between z and the numbers is new), `distinct` and
the NaN pattern exactly, and every derived reference series keeps its Geyer pairs test_summary_host.MARGIN from zero -- a failure
there asks for another seed, not for a skip.  A handle needs Np >= 3, so one chain (P = 1) is checked on the host only; a pool of
2^31 values cannot be built here, its refusal is checked in tests/rankplan_host.cpp.  Each test prints the maxima it saw."""
import math

import numpy as np
import pytest

import test_quantile_host as Q
import test_rank_host as H
import test_summary_host as R
from test_gpu_summary import gaussian_engine, synthetic_engine

pytestmark = pytest.mark.gpu
RTOL = 1e-9
TILE = H.RANK_TILE


def overwrite(eng, row0, by_id):
    """theta of rows [row0, row0 + n) := by_id[n][id][D], written slot-keyed (row i, slot s holds id idh[i][s])"""
    n = by_id.shape[0]
    idh = eng.get_history(row0, row0 + n)[3]
    eng.set_history_rows(row0, np.take_along_axis(by_id, idh[:, :, None], axis=1))


def slot_series(eng, row0, row1):
    """[D+2] series of [n][P] values, slot-keyed as demc_rank_series answers"""
    th, acc, lp, _ = eng.get_history(row0, row1)
    return [th[:, :, j] for j in range(th.shape[2])] + [acc.astype(np.float64), lp]


def check_series(demc, eng, row0, row1, series, label):
    """kinds 0 and 2 bit for bit, kind 1 at the measured bar, for the given series of the window; returns the worst score error"""
    C = demc.chains
    xs = slot_series(eng, row0, row1)
    worst = 0.0
    for j in series:
        x = xs[j]
        N = x.size
        want = C.series_ranks(x)[0]
        got = eng.rank_series(row0, row1, j, 0)
        assert got.shape == x.shape and np.array_equal(got, want), (label, j, "ranks", np.argwhere(got != want)[:5].tolist())
        med = C.series_quantiles(x, (0.5,))[0]
        with np.errstate(all="ignore"):
            zeta = np.abs(x - med)
        got2 = eng.rank_series(row0, row1, j, 2)
        assert np.array_equal(got2, C.series_ranks(zeta)[0]), (label, j, "ranks of zeta")
        z, zh = eng.rank_series(row0, row1, j, 1), C.normal_scores(want, N)
        err = np.abs(z - zh) / np.where(zh == 0.0, 1.0, np.abs(zh))
        worst = max(worst, float(err.max()))
        assert (err <= H.PPND_BAR).all(), (label, j, "scores", float(err.max()))
    print(f"{label}: ranks and ranks of zeta exact for series {list(series)}; worst relative score error {worst:.3g} (bar {H.PPND_BAR:.3g})")
    return worst


def keys_to_values(keys):
    k = np.asarray(keys, dtype=np.uint64)
    return (k ^ np.where(k >> np.uint64(63) != 0, np.uint64(Q.SIGN), np.uint64(Q.ALL))).view(np.float64)


def patterns(n, P, rng):
    """[n][P][7]: all equal | two values | keys that differ in the top digit only | in the bottom digit only | mixed signs with both
    zeros | heavy ties | a plain Normal"""
    N = n * P
    top = keys_to_values((rng.integers(1, 0xFF, N).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0123456789ABCD))
    assert np.isfinite(top).all() and (N < 256 or ((top < 0).any() and (top > 0).any()))
    bottom = keys_to_values(np.uint64(Q.key(1.0)) | rng.integers(0, 256, N).astype(np.uint64))
    mixed = rng.normal(size=N)
    mixed[rng.random(N) < 0.1] = 0.0
    mixed[rng.random(N) < 0.1] = -0.0
    assert N < 256 or ((np.signbit(mixed) & (mixed == 0)).any() and (~np.signbit(mixed) & (mixed == 0)).any())
    cols = [np.full(N, 2.5), (rng.random(N) < 0.3) * 1.0, top, bottom, mixed, np.round(rng.normal(size=N) * 4.0) / 4.0, rng.normal(size=N)]
    return np.stack(cols, axis=1).reshape(n, P, len(cols))


# ---- demc_rank_series: the sort, bit for bit -------------------------------------------------------------------------------------------
EDGES = {  # case: (n, G, Np, the tiles and the pairs of the last tile it is there for)
    "below one tile": (64, 1, 4, 1, 256),
    "one tile less one": (89, 1, 23, 1, TILE - 1),
    "one full tile": (256, 2, 4, 1, TILE),
    "one tile and one": (683, 1, 3, 2, 1),
    "n = 1": (1, 2, 4, 1, 8),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_rank_series_at_the_tile_edges(demc, case):
    n, G, Np, tiles, last = EDGES[case]
    P = G * Np
    g = H.geometry(n, P, 1)
    assert (g["tiles"], g["last_tile"], g["batch"]) == (tiles, last, 1), g
    eng, _ = synthetic_engine(demc, n, G, Np, 7, 0.5, 0)
    overwrite(eng, 0, patterns(n, P, np.random.default_rng(17)))
    check_series(demc, eng, 0, n, range(9), case)
    xs = slot_series(eng, 0, n)
    assert len(set(xs[0].reshape(-1))) == 1 and len(set(xs[1].reshape(-1))) <= 2  # all equal; two values
    assert (eng.rank_series(0, n, 0, 0) == (n * P + 1) / 2).all()  # all equal: every rank (N + 1) / 2, every pass skipped
    for j in ((2, 3) if n * P >= 256 else ()):  # one digit differs: seven of the eight passes are skipped
        k = demc.chains.series_keys(xs[j]).reshape(-1)
        diff = int(np.bitwise_or.reduce(k) & np.bitwise_or.reduce(~k))
        assert diff and (diff & ~(0xFF << (56 if j == 2 else 0))) == 0, (j, hex(diff))
    eng.close()


def test_rank_series_tie_run_across_tile_boundaries(demc):
    """four tiles; one run of equal keys covers sorted positions 1500 .. 4499, across the boundaries at 2048 and 4096; the patterns of
    the small cases once more at this size (a skipped pass with several tiles); then a window that does not start at row zero"""
    n, G, Np = 1024, 2, 4
    P, N = G * Np, 1024 * 8
    g = H.geometry(n, P, 1)
    assert g["tiles"] == 4 and g["last_tile"] == TILE and N >= 3 * TILE
    eng, _ = synthetic_engine(demc, n, G, Np, 8, 0.5, 0)
    rng = np.random.default_rng(23)
    by_id = np.concatenate([patterns(n, P, rng), np.zeros((n, P, 1))], axis=2)
    x = rng.normal(size=N)
    order = np.argsort(x, kind="stable")
    x[order[1500:4500]] = x[order[1500]]
    by_id[:, :, 7] = x.reshape(n, P)
    overwrite(eng, 0, by_id)
    xs = slot_series(eng, 0, n)
    r = demc.chains.series_ranks(xs[7])[0]
    assert (r == 1500 + (3000 + 1) / 2).sum() == 3000  # the run: L = 1500, E = 3000
    check_series(demc, eng, 0, n, range(10), "four tiles, a tie run across two boundaries")
    assert H.geometry(412, P, 1)["tiles"] == 2 and H.geometry(412, P, 1)["last_tile"] == 412 * 8 - TILE
    check_series(demc, eng, 100, 512, (4, 7, 8, 9), "rows 100 .. 512")
    eng.close()


def test_rank_series_minus_infinity_in_four_whole_chains(demc):
    n, G, Np = 40, 2, 4
    eng, _ = synthetic_engine(demc, n, G, Np, 2, 0.5, 0)
    by_id = np.stack([R.ar1(n, 8, 0.5, 0), R.ar1(n, 8, 0.5, 1)], axis=2)
    by_id[:, 0:4, 0] = -np.inf  # half the pool: the median is -inf and zeta holds NaNs, ranked beyond +inf
    by_id[:, 0:3, 1] = -np.inf  # less than half: the median is finite and zeta = +inf ties at the top
    overwrite(eng, 0, by_id)
    check_series(demc, eng, 0, n, (0, 1), "-inf in whole chains")
    xs = slot_series(eng, 0, n)
    assert demc.chains.series_quantiles(xs[0], (0.5,))[0] == -np.inf and np.isfinite(demc.chains.series_quantiles(xs[1], (0.5,))[0])
    eng.close()


def test_rank_series_padded_history(demc):
    """D = 9 with partners from the history: cells are 16 doubles apart, and the kept rows start behind the initial ones"""
    eng, _ = synthetic_engine(demc, 200, 2, 4, 9, 0.5, 1, n_initial=3, partner_kind=1)
    assert Q.hist_ld(9, True) == 16
    by_id = np.concatenate([patterns(200, 8, np.random.default_rng(29)), np.random.default_rng(30).standard_cauchy(size=(200, 8, 2))], axis=2)
    overwrite(eng, 3, by_id)
    check_series(demc, eng, 3, 203, range(11), "padded cells, rows 3 .. 203")
    eng.close()


# ---- demc_rankstats against the plain-loop restatement ----------------------------------------------------------------------------------
def compare_table(out, value, label, refs=None, max_lag=0):
    """out[D+2][8] against the restatement of value[n][D+2][P] (refs: restatements already at hand, by series)"""
    worst = 0.0
    for j in range(value.shape[1]):
        ref = (refs or {}).get(j) or H.restate(value[:, j, :], max_lag)
        worst = max(worst, H.compare(out[j], ref, RTOL, f"{label} series {j}"))
        if ref["pmin"] is not None:
            assert ref["pmin"] >= R.MARGIN, f"{label}: a derived series of series {j} has a pair {ref['pmin']:.3g} from zero -- choose another seed"
    print(f"{label}: max relative error {worst:.3g}")
    return worst


SYNTH = [(64, 1, 4, 0.0), (65, 1, 4, 0.9), (129, 1, 3, -0.5), (200, 2, 4, 0.5)]


@pytest.mark.parametrize("n,G,Np,phi", SYNTH)
def test_rankstats_heavy_tails(demc, n, G, Np, phi):
    """the AR(1) cases as they are, through exp (monotone: the bulk columns are those of the untransformed input) and through a
    Cauchy quantile (heavy tails)"""
    P = G * Np
    assert (n, P, phi) in H.CASES and H.geometry(n, P, 5)["batches"] == 1
    eng, _ = synthetic_engine(demc, n, G, Np, 3, phi, 0)
    x = R.ar1(n, P, phi, 0)
    overwrite(eng, 0, np.stack([x, H.transformed(x, "exp"), H.transformed(x, "cauchy")], axis=2))
    value = eng.export_chains(0, n)
    assert np.array_equal(value[:, 1, :], H.transformed(x, "exp"))
    out = eng.rankstats(0, n)
    refs = {j: H.case_reference(n, P, phi, how) for j, how in enumerate(("raw", "exp", "cauchy"))}
    compare_table(out, value, f"AR(1) n={n} m={P} phi={phi}", refs)
    for j in (1, 2):  # ranks do not see a monotone map
        for c in (1, 3, 7):
            assert abs(out[j, c] - out[0, c]) <= 1e-12 * abs(out[0, c]), (j, c, out[j, c], out[0, c])
    assert out[0, 7] == n * P and out[3, 7] == 2.0 and np.isnan(out[3, 2])  # acceptance: two values, constant tail indicators
    capped = eng.rankstats(0, n, max_lag=5)
    compare_table(capped[:3], value[:, :3, :], f"AR(1) n={n} max_lag=5", {j: H.case_reference(n, P, phi, how, 5) for j, how in enumerate(("raw", "exp", "cauchy"))}, 5)
    eng.close()


@pytest.fixture(scope="module")
def stepped(demc):
    eng = gaussian_engine(demc, 2, 4, 129, 11)
    eng.step(1, 129)
    value = eng.export_chains(0, 129)
    value.setflags(write=False)
    yield eng, value
    eng.close()


def test_rankstats_sampler_made_history(stepped):
    eng, value = stepped
    compare_table(eng.rankstats(0, 129), value, "sampler-made n=129 P=8")
    compare_table(eng.rankstats(40, 129), value[40:129], "sampler-made rows 40 .. 129")


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8])
def test_rankstats_short_windows(stepped, n):
    """DESIGN.md 5.5's NaN pattern in each column: R-hat needs h >= 2, ESS h >= 4"""
    eng, value = stepped
    out = eng.rankstats(0, n)
    compare_table(out, value[:n], f"n={n}")
    h = n // 2
    for j in range(4):  # (what is finite beyond these is the restatement's to say: a short series may be constant in a chain)
        assert h >= 2 or np.isnan(out[j, [0, 3, 4]]).all(), (n, j, out[j])
        assert h >= 4 or np.isnan(out[j, [1, 2, 5, 6]]).all(), (n, j, out[j])
        assert out[j, 7] >= 1


def test_rankstats_second_batch(demc):
    """D + 2 = 17 series: one batch holds sixteen, so a second one runs, with one series"""
    n, G, Np, D = 64, 1, 4, 15
    g = H.geometry(n, G * Np, D + 2)
    assert (g["batch"], g["batches"], g["last_batch"]) == (16, 2, 1)
    eng, value = synthetic_engine(demc, n, G, Np, D, 0.0, 0, scale=True)
    compare_table(eng.rankstats(0, n), value, "17 series, two batches")
    eng.close()


def test_rankstats_padded_history(demc):
    eng, value = synthetic_engine(demc, 200, 2, 4, 9, 0.5, 1, n_initial=3, partner_kind=1)
    out = eng.rankstats(3, 203)
    refs = {}
    for j in range(9):  # parameter j is the AR(1) input of seed (1 + j) % 3: three restatements serve nine series
        refs[j] = refs.get(j - 3) or H.restate(value[:, j, :])
    compare_table(out, value, "history partners D=9", refs)
    eng.close()


# ---- NaN rules ------------------------------------------------------------------------------------------------------------------------
def test_one_nan_spoils_its_own_series_only(demc):
    n, P = 64, 4
    eng, _ = synthetic_engine(demc, n, 1, 4, 3, 0.0, 0)
    x = R.ar1(n, P, 0.0, 0)
    overwrite(eng, 0, np.stack([x, H.transformed(x, "exp"), H.transformed(x, "cauchy")], axis=2))
    clean = eng.rankstats(0, n)
    bad = np.stack([x, H.transformed(x, "exp"), H.transformed(x, "cauchy")], axis=2)
    bad[17, 2, 1] = np.nan
    overwrite(eng, 0, bad)
    out = eng.rankstats(0, n)
    assert np.isnan(out[1]).all() and np.isfinite(clean[1]).all()
    assert out[[0, 2, 3, 4]].tobytes() == clean[[0, 2, 3, 4]].tobytes()
    eng.close()


def test_lp_that_never_becomes_finite(demc):
    """the recipe of the summary tests with two groups: group 0 never leaves the outside of the bounds, so lp is -inf in four of
    the eight chains: the median of lp is -inf, zeta holds NaNs, rhat_folded and rhat are NaN; bulk and tail are still reported"""
    from conftest import make_problem, setup_engine
    G, Np, n = 2, 4, 40
    prob = make_problem("gaussian", np.random.default_rng(7), N=50)
    eng = demc.HipEngine(n_groups=G, Np=Np, D=2, n_rows=n, schedule=2, seed=31, alpha=0.0, burnin=0)
    setup_engine(eng, prob)
    th = np.stack([np.random.default_rng(31).normal(0.3, 0.2, G * Np), np.random.default_rng(32).uniform(1.0, 1.5, G * Np)], 1)
    th[:Np, 1] = -1.0
    eng.set_state(th)
    eng.step(1, n)
    value = eng.export_chains(0, n)
    assert (value[:, 3, :Np] == -np.inf).all() and np.isfinite(value[:, 3, Np:]).all()
    out = eng.rankstats(0, n)
    compare_table(out, value, "lp = -inf in four chains")
    assert np.isnan(out[3, 0]) and np.isnan(out[3, 4]) and np.isfinite(out[3, 1]) and np.isfinite(out[3, 3]) and out[3, 7] > 1
    eng.close()


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_history_stays(stepped):
    eng, _ = stepped
    before = eng.get_history(0, 129)
    a, b = eng.rankstats(0, 129), eng.rankstats(0, 129)
    assert a.tobytes() == b.tobytes()
    for kind in (0, 1, 2):
        assert eng.rank_series(0, 129, 3, kind).tobytes() == eng.rank_series(0, 129, 3, kind).tobytes()
    for x, y in zip(before, eng.get_history(0, 129)):
        assert np.array_equal(x, y)
    out = np.full((5, 8), -7.0)  # only (D + 2) x 8 doubles are written
    import ctypes as C
    assert eng.L.demc_rankstats(eng.h, 0, 129, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert out[:4].tobytes() == a.tobytes() and (out[4] == -7.0).all()


def test_rankstats_between_steps_changes_nothing(demc):
    states = []
    for split in (False, True):
        eng = gaussian_engine(demc, 3, 8, 40, 21)
        if split:
            eng.step(1, 20)
            eng.rankstats(0, 20)
            eng.rank_series(0, 20, 1, 2)
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
        for call in (lambda: eng.rankstats(*rows), lambda: eng.rank_series(*rows, 0, 0)):
            with pytest.raises(demc.DemcError) as e:
                call()
            assert e.value.code == E and "bad rows" in str(e.value), rows
    for series, kind, word in ((-1, 0, "series"), (4, 0, "series"), (0, -1, "kind"), (0, 3, "kind")):
        with pytest.raises(demc.DemcError) as e:
            eng.rank_series(0, 5, series, kind)
        assert e.value.code == E and word in str(e.value), (series, kind)
    with pytest.raises(demc.DemcError) as e:
        eng.rankstats(0, 5, max_lag=-1)
    assert e.value.code == E and "max_lag" in str(e.value)
    assert eng.L.demc_rankstats(eng.h, 0, 5, 0, None) == E and b"out is NULL" in eng.L.demc_last_error(eng.h)
    assert eng.L.demc_rank_series(eng.h, 0, 5, 0, 0, None) == E
    assert eng.rankstats(0, 5).shape == (4, 8)  # the handle is still good
    eng.close()
    eng = gaussian_engine(demc, 2, 4, 10, 1, store_history=0)
    with pytest.raises(demc.DemcError) as e:
        eng.rankstats(0, 5)
    assert e.value.code == E and "history" in str(e.value)
    eng.close()
    eng = gaussian_engine(demc, 2, 4, 10, 1, n_groups_total=4)
    for call in (lambda: eng.rankstats(0, 5), lambda: eng.rank_series(0, 5, 0, 0)):
        with pytest.raises(demc.DemcError) as e:
            call()
        assert e.value.code == E and "sharded" in str(e.value)
    eng.close()


# ---- the public surface ---------------------------------------------------------------------------------------------------------------
def test_summarize_rank_equals_sample_then_rankstats(demc):
    D = demc
    data = np.random.default_rng(50514).normal(0.0, 1.0, 50)

    def run(fn, **kw):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("μ", "σ"), data=data, prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)),
                          loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
        return fn(model, de, D.HIPBackend(seed=3), 300, **kw)

    summary = run(D.summarize, rank=True)
    plain = run(D.summarize)
    chains = run(D.sample)
    host = chains.rankstats()
    assert isinstance(summary.rank, D.RankStats) and summary.rank.names == host.names == ["μ", "σ", "acceptance", "lp"]
    assert plain.rank is None and plain.values.tobytes() == summary.values.tobytes()
    worst = 0.0
    for j in range(4):
        for k in range(7):
            a, b = summary.rank.values[j, k], host.values[j, k]
            assert math.isnan(a) == math.isnan(b), (j, k, a, b)
            if not math.isnan(b):
                worst = max(worst, abs(a - b) / abs(b))
        assert summary.rank.values[j, 7] == host.values[j, 7]
    print(f"summarize(rank=True) vs sample + rankstats: max relative error {worst:.3g}")
    assert worst <= RTOL and np.isfinite(summary.rank.values[:2, :3]).all()
