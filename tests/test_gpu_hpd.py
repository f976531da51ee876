"""demc_hpd (include/demc_hpd.h, csrc/demc_hpdplan.hpp, the kernels in csrc/demc_rank.cpp; the definition is DESIGN.md 5.12) on the GPU.

Every comparison is BIT FOR BIT against chains.series_hpd of the same slot-keyed rows read back with get_history: the definition is
integer positions, one subtraction and a first-minimum rule, so there is no tolerance to choose.  Every case asserts through
test_hpd_host.geometry() (and sort_passes()) the path it is there for.  A handle needs Np >= 3, so one chain is checked on the host
only; a pool of 2^31 values cannot be built here, its refusal is checked in tests/hpdplan_host.cpp."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import test_hpd_host as HP
import test_quantile_host as Q
from test_gpu_rank import keys_to_values, overwrite, patterns, slot_series
from test_gpu_summary import gaussian_engine, synthetic_engine

pytestmark = pytest.mark.gpu
ALPHAS = (1e-9, 0.05, 0.5, 0.999)  # m = 1, a typical m, overlapping halves, m = N or a position or two below it
WG, MAX_BLOCKS = HP.HPD_WG, HP.HPD_MAX_BLOCKS


def check_table(demc, eng, row0, row1, alphas, label):
    """the whole table of the window against series_hpd, bit for bit (the NaN pattern included) -> (table, the series)"""
    xs = slot_series(eng, row0, row1)
    out = eng.hpd(row0, row1, alphas)
    assert out.shape == (len(xs), len(alphas), 4), (label, out.shape)
    for j, x in enumerate(xs):
        want = demc.chains.series_hpd(x, alphas)
        assert Q.same_bits(out[j], want), (label, j, out[j].tolist(), want.tolist())
    print(f"{label}: {len(xs)} series x {len(alphas)} alphas bit for bit")
    return out, xs


# ---- 1. tile and size edges -------------------------------------------------------------------------------------------------------------
EDGES = {  # the sizes of test_gpu_rank.EDGES: (n, G, Np, tiles, pairs of the last tile)
    "N = 8": (1, 2, 4, 1, 8),
    "N = 256": (64, 1, 4, 1, 256),
    "N = 2047": (89, 1, 23, 1, 2047),
    "N = 2048": (256, 2, 4, 1, 2048),
    "N = 2049": (683, 1, 3, 2, 1),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_hpd_at_the_tile_edges(demc, case):
    n, G, Np, tiles, last = EDGES[case]
    P = G * Np
    N = n * P
    alphas = ALPHAS + (1.0 - 1e-9,)  # ... and m = N exactly, at every size
    g = HP.geometry(n, P, 9, alphas)
    assert (g["tiles"], g["last_tile"], g["batch"], g["batches"]) == (tiles, last, 9, 1), g
    assert g["m"][0] == 1 and 2 * g["m"][2] >= N and N - 2 <= g["m"][3] <= N and g["m"][4] == N and max(g["trips"]) == 1, g
    assert N == 8 or 1 < g["m"][1] < g["m"][2], g
    eng, _ = synthetic_engine(demc, n, G, Np, 7, 0.5, 0)
    overwrite(eng, 0, patterns(n, P, np.random.default_rng(17)))
    out, xs = check_table(demc, eng, 0, n, alphas, case)
    assert len(set(xs[0].reshape(-1))) == 1 and len(set(xs[1].reshape(-1))) <= 2  # all equal; two values
    assert (out[0, :, 2] == 0.0).all() and (out[0, :, :2] == 2.5).all()  # all equal: every width ties at zero, the first candidate wins
    assert (out[:, :, 3] == np.array(g["m"], dtype=np.float64)).all()
    assert (out[:, 0, 2] == 0.0).all() and (out[:, 4, 2] == 0.0).all()  # m = 1: one candidate; m = N: every width zero
    for j in range(9):  # m = 1: the whole range
        assert out[j, 0, 0] == xs[j].min() and out[j, 0, 1] == xs[j].max()
    eng.close()


# ---- 2. which of the two buffers holds the sorted pool ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G,Np", [(64, 1, 4), (683, 1, 3)])
def test_hpd_reads_the_buffer_the_passes_left_the_pool_in(demc, n, G, Np):
    """columns whose sort runs zero, one, one, two and eight passes: the sorted pool is in buffer 0, 1, 1, 0, 0"""
    P = G * Np
    N = n * P
    rng = np.random.default_rng(41)
    pat = patterns(n, P, rng)
    both = keys_to_values((rng.integers(1, 0xFF, N).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0123456789AB00) | rng.integers(0, 256, N).astype(np.uint64))
    assert np.isfinite(both).all()
    by_id = np.stack([pat[:, :, 0], pat[:, :, 2], pat[:, :, 3], both.reshape(n, P), pat[:, :, 6]], axis=2)
    eng, _ = synthetic_engine(demc, n, G, Np, 5, 0.5, 0)
    overwrite(eng, 0, by_id)
    out, xs = check_table(demc, eng, 0, n, ALPHAS, f"buffer parity N={N}")
    assert [HP.sort_passes(x) for x in xs[:5]] == [(0, 0), (1, 1), (1, 1), (2, 0), (8, 0)], [HP.sort_passes(x) for x in xs[:5]]
    for j, digit in ((1, 7), (2, 0)):  # one digit differs, as test_rank_series_at_the_tile_edges checks it: by the diff word
        k = demc.chains.series_keys(xs[j]).reshape(-1)
        diff = int(np.bitwise_or.reduce(k) & np.bitwise_or.reduce(~k))
        assert diff and (diff & ~(0xFF << (8 * digit))) == 0, (j, hex(diff))
    k = demc.chains.series_keys(xs[3]).reshape(-1)
    diff = int(np.bitwise_or.reduce(k) & np.bitwise_or.reduce(~k))
    assert (diff >> 56) & 0xFF and diff & 0xFF and (diff & ~((0xFF << 56) | 0xFF)) == 0, hex(diff)
    for j in range(5):  # an answer read from the other buffer would not be sorted: the ends would not be the pool's extremes at m = 1
        assert out[j, 0, 0] == xs[j].min() and out[j, 0, 1] == xs[j].max() and out[j, 0, 2] == 0.0
    eng.close()


# ---- 3. where the minimum sits -----------------------------------------------------------------------------------------------------------
def test_hpd_finds_the_minimum_wherever_it_sits(demc):
    """a shuffled ramp: every width ties at N - m and the first candidate wins; then the value at sorted position N - m + i* is lowered
    by 0.5, so that candidate i* alone is narrower: i* = 0, the last lane of a wave, both sides of the workgroup edge, a candidate of
    the second grid stride, and m - 1.  N is the smallest pool of eight chains in which a thread takes more than one candidate"""
    n, G, Np, alpha = 2051, 2, 4, 0.999
    P = G * Np
    N = n * P
    alphas = (alpha, 0.5)
    g = HP.geometry(n, P, 3, alphas)
    m = g["m"][0]
    assert g["wgs"] == [MAX_BLOCKS, 33] and g["trips"] == [2, 1] and HP.geometry(n - 1, P, 3, alphas)["trips"] == [1, 1], g
    stride = MAX_BLOCKS * WG
    assert stride < m < N and g["tiles"] == 9
    eng, _ = synthetic_engine(demc, n, G, Np, 1, 0.5, 0)
    ramp = np.random.default_rng(3).permutation(N).astype(np.float64)
    overwrite(eng, 0, ramp.reshape(n, P, 1))
    out, _ = check_table(demc, eng, 0, n, alphas, "ramp")
    assert out[0, 0].tolist() == [0.0, float(N - m), 0.0, float(m)] and out[0, 1, 2] == 0.0
    for i_star in (0, 63, 64, WG - 1, WG, stride - 1, stride, stride + 5, m - 1):
        x = ramp.copy()
        x[ramp == float(N - m + i_star)] -= 0.5
        overwrite(eng, 0, x.reshape(n, P, 1))
        out, _ = check_table(demc, eng, 0, n, alphas, f"i* = {i_star}")
        assert out[0, 0].tolist() == [float(i_star), N - m + i_star - 0.5, float(i_star), float(m)], (i_star, out[0, 0].tolist())
    eng.close()


# ---- 4. widths that tie only after rounding ------------------------------------------------------------------------------------------------
def test_hpd_ties_of_rounded_widths_go_to_the_smallest_position(demc):
    """the lower half of the pool in [0, 1), the upper half at 1e16 + {0, 2, 4}: the true widths 1e16 + 2 k - u are all distinct, the
    doubles they round to take three values.  The first of the smallest rounded widths wins, not the smallest true width"""
    n, G, Np = 256, 2, 4
    P = G * Np
    N = n * P
    rng = np.random.default_rng(11)
    low = rng.random(N // 2)
    high = 1e16 + 2.0 * rng.integers(0, 3, N // 2)
    assert len(set(low)) == N // 2
    x = rng.permutation(np.concatenate([low, high]))
    eng, _ = synthetic_engine(demc, n, G, Np, 1, 0.5, 0)
    overwrite(eng, 0, x.reshape(n, P, 1))
    out, xs = check_table(demc, eng, 0, n, (0.5, 0.25), "rounded widths")
    y = np.sort(xs[0].reshape(-1))
    m = N // 2
    assert out[0, 0, 3] == m
    exact = [Fraction(float(y[m + i])) - Fraction(float(y[i])) for i in range(m)]
    rounded = y[m:] - y[:m]
    first = int(out[0, 0, 2])
    assert len(set(exact)) == m and len(set(rounded.tolist())) == 3
    assert rounded[first] == rounded.min() and (rounded[:first] > rounded[first]).all() and (rounded == rounded.min()).sum() > 1
    assert exact.index(min(exact)) != first  # the case is a real one: exact arithmetic would have chosen another candidate
    eng.close()


# ---- 5. infinities and NaN ---------------------------------------------------------------------------------------------------------------
def test_hpd_lp_minus_infinity_in_half_the_pool(demc):
    """the recipe of test_gpu_rank: group 0 never leaves the outside of the bounds, lp is -inf in four of the eight chains.  alpha =
    0.75: a candidate spans N / 4 + 1 values, the first lies wholly among the -inf: [-inf, -inf].  alpha = 0.25: every candidate has
    one end at -inf, widths of +inf tie and the first wins"""
    from conftest import make_problem, setup_engine
    G, Np, n = 2, 4, 40
    prob = make_problem("gaussian", np.random.default_rng(7), N=50)
    eng = demc.HipEngine(n_groups=G, Np=Np, D=2, n_rows=n, schedule=2, seed=31, alpha=0.0, burnin=0)
    setup_engine(eng, prob)
    th = np.stack([np.random.default_rng(31).normal(0.3, 0.2, G * Np), np.random.default_rng(32).uniform(1.0, 1.5, G * Np)], 1)
    th[:Np, 1] = -1.0
    eng.set_state(th)
    eng.step(1, n)
    out, xs = check_table(demc, eng, 0, n, (0.75, 0.25), "lp = -inf in four chains")
    N = n * G * Np
    assert (xs[3] == -np.inf).sum() == N // 2 and HP.geometry(n, G * Np, 4, (0.75, 0.25))["m"] == [3 * N // 4, N // 4]
    assert out[3, 0].tolist() == [-np.inf, -np.inf, 0.0, 3 * N // 4]
    assert out[3, 1, 0] == -np.inf and np.isfinite(out[3, 1, 1]) and out[3, 1, 2] == 0.0
    eng.close()


def test_hpd_infinite_widths_never_win_and_one_nan_spoils_its_own_series_only(demc):
    n, G, Np = 64, 1, 4
    P = G * Np
    rng = np.random.default_rng(19)
    eng, _ = synthetic_engine(demc, n, G, Np, 3, 0.5, 0)
    clean = rng.normal(size=(n, P, 3))
    clean[3:8, 1, 0] = -np.inf  # a few: the candidates that start there have widths of +inf
    clean[9, 2, 2] = np.inf
    overwrite(eng, 0, clean)
    before, _ = check_table(demc, eng, 0, n, ALPHAS, "a few infinities")
    assert np.isfinite(before[0, 1:3]).all() and before[0, 1, 2] >= 5 and np.isfinite(before[2, 1:3]).all()
    assert before[0, 0, 0] == -np.inf and before[2, 0, 1] == np.inf  # m = 1: the whole range is all there is
    bad = clean.copy()
    bad[17, 2, 1] = np.nan
    overwrite(eng, 0, bad)
    out, _ = check_table(demc, eng, 0, n, ALPHAS, "one NaN")
    assert np.isnan(out[1, :, :3]).all() and (out[1, :, 3] == before[1, :, 3]).all() and np.isfinite(before[1]).all()
    assert out[[0, 2, 3, 4]].tobytes() == before[[0, 2, 3, 4]].tobytes()
    eng.close()


# ---- 6. history and batching -----------------------------------------------------------------------------------------------------------
def test_hpd_padded_history(demc):
    """D = 9 with partners from the history: cells are 16 doubles apart, and the kept rows start behind the initial ones"""
    eng, _ = synthetic_engine(demc, 200, 2, 4, 9, 0.5, 1, n_initial=3, partner_kind=1)
    assert Q.hist_ld(9, True) == 16
    by_id = np.concatenate([patterns(200, 8, np.random.default_rng(29)), np.random.default_rng(30).standard_cauchy(size=(200, 8, 2))], axis=2)
    overwrite(eng, 3, by_id)
    check_table(demc, eng, 3, 203, ALPHAS, "padded cells, rows 3 .. 203")
    eng.close()


def test_hpd_window_that_does_not_start_at_row_zero(demc):
    n, G, Np = 1024, 2, 4
    eng, _ = synthetic_engine(demc, n, G, Np, 7, 0.5, 0)
    overwrite(eng, 0, patterns(n, G * Np, np.random.default_rng(23)))
    g = HP.geometry(412, G * Np, 9, ALPHAS)
    assert g["tiles"] == 2 and g["last_tile"] == 412 * 8 - 2048
    a, _ = check_table(demc, eng, 100, 512, ALPHAS, "rows 100 .. 512")
    b, _ = check_table(demc, eng, 0, n, ALPHAS, "rows 0 .. 1024")
    assert a.tobytes() != b.tobytes()
    eng.close()


@pytest.fixture(scope="module")
def stepped(demc):
    eng = gaussian_engine(demc, 2, 4, 129, 11)
    eng.step(1, 129)
    yield eng
    eng.close()


def test_hpd_sampler_made_history(demc, stepped):
    out, xs = check_table(demc, stepped, 0, 129, ALPHAS, "sampler-made n=129 P=8")
    check_table(demc, stepped, 40, 129, (0.05,), "sampler-made rows 40 .. 129")
    assert np.isfinite(out).all() and (out[:2, 1, 0] < out[:2, 1, 1]).all()
    assert set(out[2, :, 0].tolist()) | set(out[2, :, 1].tolist()) <= {0.0, 1.0}  # acceptance: the ends are pool values


def test_hpd_second_batch(demc):
    """D + 2 = 17 series: one batch holds sixteen, so a second one runs, with one series"""
    n, G, Np, D = 64, 1, 4, 15
    g = HP.geometry(n, G * Np, D + 2, ALPHAS)
    assert (g["batch"], g["batches"], g["last_batch"]) == (16, 2, 1)
    eng, _ = synthetic_engine(demc, n, G, Np, D, 0.0, 0, scale=True)
    out, _ = check_table(demc, eng, 0, n, ALPHAS, "17 series, two batches")
    assert np.isfinite(out[16]).all() and out[16, 1, 0] < out[16, 1, 1]  # lp: the series of the second batch
    eng.close()


# ---- 7. behaviour around the call -------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_history_stays(demc, stepped):
    eng = stepped
    before = eng.get_history(0, 129)
    rank_before = eng.rankstats(0, 129)
    a, b = eng.hpd(0, 129, ALPHAS), eng.hpd(0, 129, ALPHAS)
    assert a.tobytes() == b.tobytes()
    assert eng.hpd(0, 129, (0.5,)).tobytes() == a[:, 2:3].tobytes()  # an alpha's answer does not depend on its neighbours
    for x, y in zip(before, eng.get_history(0, 129)):
        assert np.array_equal(x, y)
    assert eng.rankstats(0, 129).tobytes() == rank_before.tobytes()
    assert eng.rank_series(0, 129, 1, 0).tobytes() == demc.chains.series_ranks(slot_series(eng, 0, 129)[1])[0].tobytes()
    out = np.full((5, 2, 4), -7.0)  # only (D + 2) x n_alphas x 4 doubles are written
    al = np.array([0.05, 0.5])
    assert eng.L.demc_hpd(eng.h, 0, 129, al.ctypes.data_as(C.POINTER(C.c_double)), 2, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert out[:4].tobytes() == a[:, 1:3].tobytes() and (out[4] == -7.0).all()
    assert eng.hpd(0, 129).shape == (4, 1, 4) and eng.hpd(0, 129).tobytes() == a[:, 1:2].tobytes()  # the default: alpha = 0.05


def test_hpd_between_steps_changes_nothing(demc):
    states = []
    for split in (False, True):
        eng = gaussian_engine(demc, 3, 8, 40, 21)
        if split:
            eng.step(1, 20)
            eng.hpd(0, 20, ALPHAS)
            eng.step(21, 20)
        else:
            eng.step(1, 40)
        states.append(list(eng.get_state()) + list(eng.get_history(0, 40)))
        eng.close()
    for x, y in zip(*states):
        assert x.tobytes() == y.tobytes()


# ---- 8. error cases -----------------------------------------------------------------------------------------------------------------------
def test_error_cases(demc):
    E, U = demc._ffi.EINVAL, demc._ffi.EUNSUPPORTED
    assert (E, U) == (1, 5)
    dp = C.POINTER(C.c_double)
    eng = gaussian_engine(demc, 2, 4, 10, 1)
    eng.step(1, 10)
    out, al = np.zeros((4, 17, 4)), np.full(17, 0.5)

    def raw(row0, row1, alphas, k, o):
        code = eng.L.demc_hpd(eng.h, row0, row1, None if alphas is None else alphas.ctypes.data_as(dp), k, None if o is None else o.ctypes.data_as(dp))
        return code, eng.L.demc_last_error(eng.h).decode()

    for rows in ((-1, 5), (0, 11), (5, 5), (6, 5)):
        with pytest.raises(demc.DemcError) as e:
            eng.hpd(*rows)
        assert e.value.code == E and "bad rows: demc_hpd needs at least one row of the history" in str(e.value), rows
        assert raw(*rows, None, 0, None) == (E, "bad rows: demc_hpd needs at least one row of the history")  # the rows rank before the arguments
    assert raw(0, 5, al, 1, None) == (E, "demc_hpd: out is NULL")
    assert raw(0, 5, None, 1, None) == (E, "demc_hpd: out is NULL")
    assert raw(0, 5, None, 1, out) == (E, "demc_hpd: alphas is NULL")
    for k in (0, -1, 17):
        assert raw(0, 5, al, k, out) == (E, "demc_hpd: n_alphas must be between 1 and 16")
    with pytest.raises(demc.DemcError) as e:
        eng.hpd(0, 5, (0.5,) * 17)
    assert e.value.code == E and "n_alphas must be between 1 and 16" in str(e.value)
    for bad in (0.0, 1.0, -0.05, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(demc.DemcError) as e:
            eng.hpd(0, 5, (0.5, bad))
        assert e.value.code == E and "demc_hpd: every alpha must be finite and strictly inside (0, 1)" in str(e.value), bad
    assert (out == 0.0).all()  # a refused call writes nothing
    assert raw(0, 5, al, 16, out)[0] == 0 and eng.hpd(0, 5).shape == (4, 1, 4)  # sixteen are taken; the handle is still good
    eng.close()
    eng = gaussian_engine(demc, 2, 4, 10, 1, store_history=0)
    for rows in ((0, 5), (-1, 50)):  # no history ranks first
        with pytest.raises(demc.DemcError) as e:
            eng.hpd(*rows)
        assert e.value.code == E and "demc_hpd: history is not stored on this handle" in str(e.value)
    eng.close()
    eng = gaussian_engine(demc, 2, 4, 10, 1, n_groups_total=4)
    with pytest.raises(demc.DemcError) as e:
        eng.hpd(0, 5)
    assert e.value.code == E and "sharded handle: gather demc_get_history from every rank and take the intervals of the pool on the host" in str(e.value)
    with pytest.raises(demc.DemcError) as e:  # the call's own arguments rank before the sharded handle
        eng.hpd(0, 5, (2.0,))
    assert e.value.code == E and "strictly inside (0, 1)" in str(e.value)
    eng.close()


# ---- 9. the public surface ----------------------------------------------------------------------------------------------------------------
def test_summarize_hpd_equals_sample_then_hpd(demc):
    D = demc
    data = np.random.default_rng(50514).normal(0.0, 1.0, 50)

    def run(fn, **kw):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("μ", "σ"), data=data, prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)),
                          loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=100, Np=6)
        return fn(model, de, D.HIPBackend(seed=3), 300, **kw)

    summary = run(D.summarize, hpd=(0.05, 0.5))
    plain = run(D.summarize)
    chains = run(D.sample)
    host = chains.hpd((0.05, 0.5))
    assert isinstance(summary.hpd, D.Hpd) and summary.hpd.names == host.names == ["μ", "σ", "acceptance", "lp"] and summary.hpd.alphas == (0.05, 0.5)
    assert plain.hpd is None and plain.values.tobytes() == summary.values.tobytes()
    assert Q.same_bits(summary.hpd.values, host.values), (summary.hpd.values.tolist(), host.values.tolist())
    one = run(D.summarize, hpd=0.05)
    assert Q.same_bits(one.hpd.values, host.values[:, :1]) and set(one.hpd.describe()) == {"μ", "σ"}
    lo, hi = one.hpd["μ"]["lower"], one.hpd["μ"]["upper"]
    assert lo < summary["μ"]["mean"] < hi and np.isfinite(summary.hpd.values).all()
