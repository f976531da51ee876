"""demc_pointwise_loglik and demc_waic at every kernel instance and at the edges of the plan, beside
tests/test_gpu_pointwise.py, whose helpers and bars it uses.  The references of sections 1 and 2 are produced by no device kernel:
tests/pointwise_cases.py's closed forms on the raw data (held to 40 digits on the host) and the oracle's per-trial densities.

1. every <family, X> instance of DEMC_PW_INSTANCES, in k_pw_matrix (the terms) and in k_pw_accumulate (demc_waic against
   waic_from_loglik of the REFERENCE's terms);
2. observation indices past the first tile of 256, the LBA's kept permutation across the tile boundary;
3. the plan's edges, each geometry asserted through test_pwplan_host.geometry before the case runs;
4. the conditioning cases of pointwise_cases.py at the tolerance derived there (test_pointwise_cases_host proves on the CPU that the
   walk without its shift misses that tolerance by more than a factor of 100 on the concentrated cases);
5. -Inf, NaN and wide-range patterns across chunks, the LBA's own -Inf and its floor.

demc_last_kernels names the kernels of the last UPDATE only, not those of these two calls, so the instance a case selects is stated
in a comment (pw_instance_x of csrc/demc_pointwise.cpp, dp_direct of prep_mvn) and not asserted."""
import math

import mpmath
import numpy as np
import pytest

import pointwise_cases as PC
import test_gpu_pointwise as TP
import test_pwplan_host as PL
from conftest import make_problem

pytestmark = pytest.mark.gpu
BAR, LBA_BAR = TP.BAR, TP.LBA_BAR


def _geometry(name, N, S, want):
    g = PL.geometry(N, S)
    for k, v in want.items():
        assert g[k] == v, f"{name}: {k} is {g[k]}, the case was chosen for {v} -- the constants of csrc/demc_pwplan.hpp moved"
    return g


def _reference(orc, prob, theta):
    from demc_amd import families as F
    return TP.oracle_terms(orc, prob, theta) if prob["fam"] in (F.FAM_LBA, F.FAM_LNR) else PC.closed_terms(prob, theta)


def _term_bars(prob, ref):
    """per term: 1e-9 max(1, |ref|); LBA 1e-5 max(1, |sum_j l_j|) of the draw"""
    from demc_amd import families as F
    fin = np.isfinite(ref)
    if prob["fam"] == F.FAM_LBA:
        return LBA_BAR * np.maximum(1.0, np.abs(np.where(fin, ref, 0.0).sum(axis=1)))[:, None] * np.ones_like(ref)
    return BAR * np.maximum(1.0, np.abs(ref))


def check_terms_independently(orc, prob, eng, label, rows=(3, 70)):
    """k_pw_matrix against a reference no device kernel produced -> worst error in units of the bar"""
    worst = 0.0
    for n in rows:
        theta = prob["init"](n)
        got = eng.pointwise_loglik(theta)
        ref = _reference(orc, prob, theta)
        assert got.shape == ref.shape == (n, prob["dims"][0])
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], ref[~fin]), label  # (-Inf exactly where the reference has it)
        err = np.abs(got - ref)[fin] / _term_bars(prob, ref)[fin]
        worst = max(worst, float(err.max()) if err.size else 0.0)
    print(f"{label}: worst term error {worst:.3g} of its bar")
    assert worst <= 1.0, (label, worst)
    return worst


def check_waic_independently(demc, orc, prob, eng, n, label):
    """k_pw_accumulate / k_pw_final against waic_from_loglik of the REFERENCE's terms of the exported rows: lppd_i and mean_i at
    1e-9 max(1, |ref|); p_waic_i at 1e-9 var_i plus, for the LBA, what the term bar allows, 2 sd_i max_s bar_s (d var = 2 / (S - 1)
    sum_s (l_s - mean) e_s <= 2 sd max|e| sqrt(S / (S - 1)) by Cauchy-Schwarz)"""
    from demc_amd import families as F
    theta = TP.draws_of(eng.export_chains(0, n), prob["D"])
    ll = _reference(orc, prob, theta)
    assert np.isfinite(ll).all(), label
    S = ll.shape[0]
    ref = demc.waic_from_loglik(ll).pointwise
    sd = ll.std(axis=0, ddof=1)
    assert (sd >= 1e-3 * np.abs(ll).max(axis=0)).all() and (ref[:, 1] > 0).all(), label  # the conditioning the 1e-9 bars were derived for
    _, pt = eng.waic(0, n, pointwise=True)
    assert np.isfinite(pt).all(), label
    tol_pw = BAR * ref[:, 1]
    if prob["fam"] == F.FAM_LBA:
        tol_pw = tol_pw + 2.0 * sd * math.sqrt(S / (S - 1.0)) * _term_bars(prob, ll).max()
    e_lppd = (np.abs(pt[:, 0] - ref[:, 0]) / (BAR * np.maximum(1.0, np.abs(ref[:, 0])))).max()
    e_mean = (np.abs(pt[:, 2] - ref[:, 2]) / (BAR * np.maximum(1.0, np.abs(ref[:, 2])))).max()
    e_pw = (np.abs(pt[:, 1] - ref[:, 1]) / tol_pw).max()
    print(f"{label}: S={S} in units of the bars: lppd {e_lppd:.3g} p_waic {e_pw:.3g} mean {e_mean:.3g}")
    assert e_lppd <= 1.0 and e_mean <= 1.0 and e_pw <= 1.0, (label, e_lppd, e_pw, e_mean)
    assert np.array_equal(pt[:, 3], pt[:, 0] - pt[:, 1]), label
    return e_lppd, e_pw, e_mean


# ---- 1. every instance, both kernels ------------------------------------------------------------------------------------------------
# pw_instance_x: LBA n_acc = 2 -> <LBA, 2>, 3 -> <LBA, 3>, anything else -> <LBA, 0>, the body with a run-time n_acc; LNR -> <LNR, 0> at
# every n_acc (its loop is always a run-time one); MvNormal -> <family, dp> with dp = dp_direct of prep_mvn: 8 for d <= 8, 16 for
# d <= 16, 32 for d <= 32, else 64
@pytest.mark.parametrize("family,na", [("lba", 1), ("lba", 2), ("lba", 4), ("lba", 8), ("lnr", 1), ("lnr", 8)])
def test_race_instances_against_the_oracle(demc, orc, family, na):
    """lba 1, 4, 8 -> <LBA, 0>; lba 2 -> <LBA, 2>; lnr 1, 8 -> <LNR, 0> at the two ends of its accumulator loop"""
    prob = make_problem(family, np.random.default_rng(6000 + 10 * na), N=65, na=na)
    eng, _ = TP.engine(demc, prob, 10, 13)
    check_terms_independently(orc, prob, eng, f"{family} n_acc={na}")
    check_waic_independently(demc, orc, prob, eng, 10, f"{family} n_acc={na} waic")
    eng.close()


@pytest.mark.parametrize("d", [1, 9, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("family", ["mvn_iso", "mvn_full"])
def test_mvn_instances_against_the_closed_form(demc, orc, family, d):
    """DIRECT mode.  d = 1 -> rows of 8; 9, 16 -> 16 (one padded, one full); 17, 32 -> 32; 33, 64 -> 64 (the largest register
    footprint, one padded, one full)"""
    dp = 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64
    assert dp == {1: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}[d]
    prob = make_problem(family, np.random.default_rng(6500 + d), N=65, d=d)
    eng, _ = TP.engine(demc, prob, 10, 13, loglike_mode=2)
    check_terms_independently(orc, prob, eng, f"{family} d={d} (rows of {dp})")
    check_waic_independently(demc, orc, prob, eng, 10, f"{family} d={d} (rows of {dp}) waic")
    eng.close()


# ---- 2. past the first tile ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [255, 256, 257, 513])
@pytest.mark.parametrize("family", ["gaussian", "binomial", "lba"])
def test_past_the_first_tile_independently(demc, orc, family, N):
    prob = make_problem(family, np.random.default_rng(7000 + N), N=N)
    _geometry(f"{family} N={N}", N, 130, dict(tiles=-(-N // 256)))
    if family == "lba":  # the trials arrive unsorted, and the library's order moves trials across the tile boundary
        ch, rt = prob["data"][:N], prob["data"][N:]
        order = np.lexsort((rt, ch))
        assert not np.array_equal(order, np.arange(N)), "the trials are already in the library's order"
        if N > 256:
            assert (order[:256] >= 256).any() and (order[256:] < 256).any(), "no trial crosses the boundary between the tiles"
    eng, _ = TP.engine(demc, prob, 10, 13)
    check_terms_independently(orc, prob, eng, f"{family} N={N}", rows=(3,))
    check_waic_independently(demc, orc, prob, eng, 10, f"{family} N={N} waic")
    eng.close()


# ---- 3. the plan's edges (the reference is waic_from_loglik of the device's terms: the reductions alone) ---------------------------
def test_1024_chunks_of_64_and_1013_chunks_of_65(demc):
    """3a: 16 groups of 16 particles, 256 rows: S = 65 536 = 1 024 chunks (the cap) of exactly kPwMinChunk = 64 draws, 256 blocks of
    k_pw_prepare, and a handle with more than one group.  3b: 257 rows of the same handle: 1 013 chunks of 65, the last of 12."""
    N, G, Np = 65, 16, 16
    _geometry("3a", N, 256 * G * Np, dict(tiles=1, chunks=PL.PW_MAX_CHUNKS, chunk_len=PL.PW_MIN_CHUNK, last_chunk=64))
    _geometry("3b", N, 257 * G * Np, dict(tiles=1, chunks=1013, chunk_len=65, last_chunk=12))
    assert PL.PW_MAX_CHUNKS == 1024 and PL.PW_MIN_CHUNK == 64 and 256 * G * Np // 256 == 256
    prob = make_problem("gaussian", np.random.default_rng(8001), N=N)
    eng, _ = TP.engine(demc, prob, 257, Np, n_groups=G)
    assert eng.P == G * Np
    TP.check_waic(demc, eng, prob, 0, 256, "3a: 1024 chunks of 64")
    TP.check_waic(demc, eng, prob, 0, 257, "3b: 1013 chunks of 65, the last of 12")
    eng.close()


def _totals_of(pt):
    """the eight totals of a pointwise table by the definition, sums in np.longdouble"""
    p = pt.astype(np.longdouble)
    N = p.shape[0]
    elpd = p[:, 3].sum()
    se = np.sqrt(N * (((p[:, 3] - elpd / N) ** 2).sum() / np.longdouble(N - 1))) if N > 1 else np.nan
    return np.array([elpd, se, p[:, 1].sum(), p[:, 0].sum(), -2 * elpd, -2 * p[:, 2].sum(), (pt[:, 1] > 0.4).sum(),
                     (~(np.isfinite(pt[:, 0]) & np.isfinite(pt[:, 1]))).sum()], dtype=np.float64)


def test_more_tiles_than_workgroups_aimed_at(demc):
    """3c: N = 262 145 = 1 025 tiles, one valid lane in the last; fill = 2 048 / 1 025 = 1, so one chunk however many draws"""
    N, n, P = 262145, 3, 13
    g = _geometry("3c", N, n * P, dict(tiles=1025, chunks=1, chunk_len=39))
    assert N - 256 * (g["tiles"] - 1) == 1 and PL.PW_TARGET_WG // g["tiles"] == 1
    assert PL.geometry(N, 1 << 20)["chunks"] == 1  # (however many draws)
    rng = np.random.default_rng(8003)
    prob = make_problem("gaussian", rng, N=N)
    x = np.asarray(prob["data"])
    rows = np.array([x.mean(), x.std()]) + 0.1 * rng.normal(0, 1, (n, P, 2))
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    theta = TP.draws_of(eng.export_chains(0, n), 2)
    ll = eng.pointwise_loglik(theta)  # 39 x 262 145 doubles: 82 MB
    assert ll.shape == (n * P, N)
    # the terms against the closed form on the last tile and on 1 000 sampled columns
    cols = np.unique(np.concatenate([np.arange(N - 257, N), rng.integers(0, N, 1000), [0, 255, 256]]))
    want = PC.closed_terms(prob, theta, cols=cols)
    e_t = (np.abs(ll[:, cols] - want) / (BAR * np.maximum(1.0, np.abs(want)))).max()
    assert e_t <= 1.0, e_t
    tot, pt = eng.waic(0, n, pointwise=True)
    worst = np.zeros(3)
    ref_pt = np.empty((N, 4))
    for i0 in range(0, N, 32768):  # the reference in blocks of observations
        ref_pt[i0:i0 + 32768] = demc.waic_from_loglik(ll[:, i0:i0 + 32768]).pointwise
    r = ref_pt
    assert np.isfinite(pt).all() and np.isfinite(r).all()
    worst[0] = (np.abs(pt[:, 0] - r[:, 0]) / np.maximum(1.0, np.abs(r[:, 0]))).max()
    worst[1] = (np.abs(pt[:, 1] - r[:, 1]) / r[:, 1]).max()
    worst[2] = (np.abs(pt[:, 2] - r[:, 2]) / np.maximum(1.0, np.abs(r[:, 2]))).max()
    sd = ll.std(axis=0, ddof=1)
    assert (sd >= 1e-3 * np.abs(ll).max(axis=0)).all()
    want_tot = _totals_of(r)
    sums = [np.abs(r[:, 3]).sum(), want_tot[1], np.abs(r[:, 1]).sum(), np.abs(r[:, 0]).sum(), 2 * np.abs(r[:, 3]).sum(), 2 * np.abs(r[:, 2]).sum()]
    t_err = [abs(tot[j] - want_tot[j]) / sums[j] for j in range(6)]
    print(f"3c: terms {e_t:.3g} of the bar; lppd {worst[0]:.3g} p_waic {worst[1]:.3g} mean {worst[2]:.3g}; totals {max(t_err):.3g}")
    assert (worst <= BAR).all() and max(t_err) <= BAR, (worst, t_err)
    assert tot[6] == want_tot[6] and tot[7] == want_tot[7] == 0
    eng.close()


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 2049])
def test_totals_at_the_laps_of_k_pw_totals(demc, N):
    """3d: one workgroup of 1 024 threads: N = 1 (se_elpd is 0 / 0) and 2, one lap less one, exactly one lap, a second lap of one
    row, a third of one row.  One central and one far observation: n_high is neither 0 nor N (N = 1: it is 1)."""
    rng = np.random.default_rng(8100 + N)
    prob = make_problem("gaussian", rng, N=N)
    x = np.asarray(prob["data"]).copy()
    x[0] = 4.0
    if N > 1:
        x[-1] = 0.3
    prob["data"] = x
    n, P = 10, 13
    rows = np.stack([0.3 + 0.3 * rng.normal(0, 1, (n, P)), 1.2 + 0.05 * rng.normal(0, 1, (n, P))], axis=2)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows)
    tot, pt = TP.check_waic(demc, eng, prob, 0, n, f"3d: N={N}")
    if N == 1:
        assert math.isnan(tot[1]) and tot[6] == 1
    else:
        assert math.isfinite(tot[1]) and 0 < tot[6] < N and pt[0, 1] > 0.4 > pt[-1, 1]
    assert tot[7] == 0
    eng.close()


def test_two_groups_with_different_draws_on_a_late_window(demc):
    """3e: the draws of a window are the cells of ALL groups, P = G Np a row: group 0 sits at mu = -1, group 1 at mu = +2"""
    rng = np.random.default_rng(8200)
    N, G, Np, n = 65, 2, 8, 12
    prob = make_problem("gaussian", rng, N=N)
    rows = np.empty((n, G * Np, 2))
    rows[:, :Np, 0] = -1.0 + 0.1 * rng.normal(0, 1, (n, Np))
    rows[:, Np:, 0] = 2.0 + 0.1 * rng.normal(0, 1, (n, Np))
    rows[:, :, 1] = 1.2 + 0.05 * rng.normal(0, 1, (n, G * Np))
    eng, rows = TP.engine(demc, prob, n, Np, rows=rows, n_groups=G)
    r0, r1 = 3, 11
    tot, pt = TP.check_waic(demc, eng, prob, r0, r1, "3e: two groups, rows 3..11")
    pooled = PC.closed_terms(prob, rows[r0:r1].reshape(-1, 2))       # every cell of the window, as written
    assert pooled.shape[0] == (r1 - r0) * G * Np
    TP.check_waic(demc, eng, prob, r0, r1, "3e against the rows written", ll=pooled)
    one = demc.waic_from_loglik(PC.closed_terms(prob, rows[r0:r1, :Np].reshape(-1, 2)))  # group 0 alone: visibly another answer
    assert abs(one.elpd_waic - tot[0]) > 1e-3 * abs(tot[0]) and abs(one.p_waic - tot[2]) > 0.5 * tot[2]
    eng.close()


# ---- 4. conditioning --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", list(PC.COND_SHAPES))
def test_conditioning_cases_at_the_derived_tolerance(demc, S):
    """|l| >> sd: what the shifted one-pass sums and the pairwise merge exist for.  The truth is waic_from_loglik of the device's own
    terms; |p_waic_i - truth| <= tol_i (pointwise_cases.tolerance) for every observation of every case."""
    shape = PC.COND_SHAPES[S]
    cases = [c for c in PC.conditioning_cases() if c["S"] == S]
    assert len(cases) == len(PC.COND_KINDS)
    g = _geometry(f"conditioning S={S}", len(PC.X_COND), S, {k: shape[k] for k in ("chunks", "chunk_len", "last_chunk")})
    eng = None
    for case in cases:
        prob = PC.cond_problem(case)
        rows = case["theta"].reshape(shape["rows"], shape["n_groups"] * shape["Np"], 2)
        if eng is None:
            eng, _ = TP.engine(demc, prob, shape["rows"], shape["Np"], rows=rows, n_groups=shape["n_groups"])
        else:
            eng.set_history_rows(0, rows)
        theta = TP.draws_of(eng.export_chains(0, shape["rows"]), 2)
        assert np.array_equal(theta, case["theta"]), "the exported draws are not in the order the window is walked"
        ll = eng.pointwise_loglik(theta)
        assert np.isfinite(ll).all()
        want = PC.closed_terms(prob, theta)
        assert (np.abs(ll - want) <= BAR * np.maximum(1.0, np.abs(want))).all(), case["name"]
        ref = demc.waic_from_loglik(ll).pointwise
        tol, var = PC.tolerance(ll, g["chunk_len"])
        if case["concentrated"]:
            assert (tol <= 1e-7 * var).all() and (np.abs(ll).max(axis=0) >= 1e5 * np.sqrt(var)).all(), case["name"]
        _, pt = eng.waic(0, shape["rows"], pointwise=True)
        assert np.isfinite(pt).all(), case["name"]
        r_pw = (np.abs(pt[:, 1] - ref[:, 1]) / tol).max()
        e_lppd = (np.abs(pt[:, 0] - ref[:, 0]) / np.maximum(1.0, np.abs(ref[:, 0]))).max()
        e_mean = (np.abs(pt[:, 2] - ref[:, 2]) / np.maximum(1.0, np.abs(ref[:, 2]))).max()
        print(f"{case['name']}: p_waic worst error / tol {r_pw:.3g} (tol / var <= {np.max(tol / var):.3g}); lppd {e_lppd:.3g} mean {e_mean:.3g}")
        assert r_pw <= 1.0, (case["name"], r_pw)
        assert e_lppd <= BAR and e_mean <= BAR, (case["name"], e_lppd, e_mean)
    eng.close()


# ---- 5. non-finite and range patterns across chunks -----------------------------------------------------------------------------------
S3, L3 = 130, 44  # three_chunks_ragged: 10 rows of 13 particles, chunks [0, 44), [44, 88), [88, 130)


def _three_chunks(N):
    _geometry("three_chunks_ragged", N, S3, dict(tiles=1, chunks=3, chunk_len=L3, last_chunk=42))


LATE = {  # the draws (index into the pooled window) whose tau lies above the fastest decision time
    "the whole middle chunk": np.arange(L3, 2 * L3),                         # E_c = 0, M_c = -Inf among finite chunks
    "the first draw of chunks 1 and 2": np.array([L3, 2 * L3]),               # l0 = -Inf in two chunks
    "all but one draw of the last chunk": np.delete(np.arange(S3), 100),      # one finite term in all: lppd = l - log S
}


@pytest.mark.parametrize("which", list(LATE))
def test_lnr_minus_infinity_across_chunks(demc, which):
    N, n, P = 65, 10, 13
    _three_chunks(N)
    prob = make_problem("lnr", np.random.default_rng(88), N=N, na=2)
    rt = np.asarray(prob["data"][N:])
    late = int(np.argmin(rt))
    tau = (rt[late] + np.sort(rt)[1]) / 2  # above the fastest decision time only
    rows = np.stack([prob["init"](P) for _ in range(n)]).reshape(S3, 3)
    rows[LATE[which], 2] = tau
    prob["hi"] = [np.inf] * 3  # (the matrix call would refuse tau above the bound)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows.reshape(n, P, 3))
    ll = eng.pointwise_loglik(TP.draws_of(eng.export_chains(0, n), 3))
    want = np.zeros(S3, dtype=bool)
    want[LATE[which]] = True
    assert np.array_equal(np.isneginf(ll[:, late]), want) and np.isfinite(np.delete(ll, late, axis=1)).all()
    tot, pt = TP.check_waic(demc, eng, prob, 0, n, f"tau late in {which}", ll=ll, guard=False)
    _, ref = PC.ref_waic(ll[:, late:late + 1])
    assert math.isfinite(pt[late, 0]) and abs(pt[late, 0] - ref[0, 0]) <= BAR * max(1.0, abs(ref[0, 0]))
    assert np.isnan(pt[late, 1:]).all() and np.isfinite(np.delete(pt, late, axis=0)).all()
    assert tot[7] == 1 and math.isfinite(tot[3]) and math.isnan(tot[0]) and math.isnan(tot[2]) and math.isnan(tot[5])
    eng.close()


@pytest.mark.parametrize("s", [100, L3], ids=["in the last, ragged chunk", "the first draw of chunk 1"])
def test_nan_cell_across_chunks(demc, s):
    N, n, P = 65, 10, 13
    _three_chunks(N)
    prob = make_problem("lnr", np.random.default_rng(89), N=N, na=2)
    rows = np.stack([prob["init"](P) for _ in range(n)]).reshape(S3, 3)
    rows[s, 0] = np.nan
    eng, _ = TP.engine(demc, prob, n, P, rows=rows.reshape(n, P, 3))
    tot, pt = TP.check_waic(demc, eng, prob, 0, n, f"a NaN cell at draw {s}", guard=False)
    assert np.isnan(pt).all() and tot[7] == N and np.isnan(tot[:6]).all() and tot[6] == 0
    eng.close()


def test_lba_minus_infinity_of_its_own(demc, orc):
    """a draw whose tau is not below the fastest decision time: lba_trial returns 0 for that trial, its log is -Inf, every other trial
    of the draw stays finite"""
    N, n, P, na = 65, 10, 13, 3
    _three_chunks(N)
    prob = make_problem("lba", np.random.default_rng(90), N=N, na=na)
    rt = np.asarray(prob["data"][N:])
    late = int(np.argmin(rt))
    tau = (rt[late] + np.sort(rt)[1]) / 2
    rows = np.stack([prob["init"](P) for _ in range(n)]).reshape(S3, na + 3)
    hit = np.array([5, L3, 129])  # inside chunk 0, the first draw of chunk 1, the last draw of all
    rows[hit, na + 2] = tau
    prob["hi"] = [np.inf] * (na + 3)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows.reshape(n, P, na + 3))
    theta = TP.draws_of(eng.export_chains(0, n), na + 3)
    ll = eng.pointwise_loglik(theta)
    ref = TP.oracle_terms(orc, prob, theta)
    want = np.zeros((S3, N), dtype=bool)
    want[hit, late] = True
    assert np.array_equal(np.isneginf(ref), want), "the case is not the one constructed"
    assert np.array_equal(np.isneginf(ll), want) and np.isfinite(ll[~want]).all()
    with np.errstate(invalid="ignore"):
        assert (np.abs(ll - ref)[~want] <= _term_bars(prob, ref)[~want]).all()
    tot, pt = TP.check_waic(demc, eng, prob, 0, n, "LBA: tau late in 3 of 130 draws", ll=ll, guard=False)
    assert math.isfinite(pt[late, 0]) and np.isnan(pt[late, 1:]).all() and np.isfinite(np.delete(pt, late, axis=0)).all() and tot[7] == 1
    eng.close()


def _lba_density(nu, A, k, tau, choice, rt):
    """the LBA's defective density (Brown and Heathcote 2008, s = 1, normalised by 1 - P(all drifts <= 0)) WITHOUT its floor, 40 digits"""
    with mpmath.workdps(40):
        m = mpmath.mpf
        Phi, phi = mpmath.ncdf, mpmath.npdf
        A, b, t = m(A), m(A) + m(k), m(rt) - m(tau)
        den, pneg = m(1), m(1)
        for a, v in enumerate(nu):
            v = m(v)
            n1, n2 = (b - A - t * v) / t, (b - t * v) / t
            if a + 1 == choice:
                den *= (-v * Phi(n1) + phi(n1) + v * Phi(n2) - phi(n2)) / A
            else:
                den *= -((b - A - t * v) / A) * Phi(n1) + ((b - t * v) / A) * Phi(n2) - (t / A) * phi(n1) + (t / A) * phi(n2)
            pneg *= Phi(-v)
        return den / (1 - pneg)


def test_lba_floor(demc, orc):
    """fast accumulators and the slowest trials of the data: the density of a tail trial is far below 1e-10 (constructed: evaluated
    at 40 digits without the floor), the oracle answers log(1e-10) and the device's term is exactly that"""
    N, na = 65, 3
    prob = make_problem("lba", np.random.default_rng(91), N=N, na=na)
    ch, rt = np.asarray(prob["data"][:N]), np.asarray(prob["data"][N:])
    theta = np.array([[6.0, 6.0, 6.0, 0.8, 0.2, 0.05], [1.0, 1.5, 2.0, 0.8, 0.2, 0.05]])
    dens = np.array([float(_lba_density(theta[0, :na], 0.8, 0.2, 0.05, int(ch[i]), rt[i])) for i in range(N)])
    tail = int(np.argmax(rt))
    assert 0.0 < dens[tail] < 1e-12 and rt[tail] > 1.4, (dens[tail], rt[tail])
    floored = dens < 1e-12
    usual = np.array([float(_lba_density(theta[1, :na], 0.8, 0.2, 0.05, int(ch[i]), rt[i])) for i in range(N)])
    assert floored.sum() >= 5 and (usual > 1e-8).all()  # (the second row: the same trials away from the floor)
    ref = TP.oracle_terms(orc, prob, theta)
    assert (ref[0, floored] == math.log(1e-10)).all()
    assert (np.abs(ref[1] - np.log(usual)) <= 1e-9).all()  # the oracle is the density written above
    eng, _ = TP.engine(demc, prob, 1, 4)
    got = eng.pointwise_loglik(theta)
    print("LBA floor: device", got[0, tail].hex(), "log(1e-10)", math.log(1e-10).hex(), "floored trials", int(floored.sum()))
    assert (got[0, floored] == math.log(1e-10)).all(), (got[0, floored] - math.log(1e-10))
    assert (np.abs(got - ref) <= _term_bars(prob, ref)).all()
    eng.close()


WIDE = {"the first draw of a chunk": L3, "the last draw of a chunk": 2 * L3 - 1, "alone in the last chunk": 100}


@pytest.mark.parametrize("where", list(WIDE))
def test_gaussian_terms_that_span_more_than_2000(demc, where):
    """one observation x = 0; draws (sigma = 1, mu about 1): l about -1.4; (sigma = 1e-3, mu = 0.07): l = -2444; (sigma = 1e-3, |mu| <=
    2e-3): l from 4 to 6; the maximum (sigma = 1e-3, mu = 0: l = 5.99) once.  exp(l - M) and E exp(M - l) underflow between the
    groups: both branches of the online log-sum-exp and the merge of chunks whose maxima are 2 450 apart.  "alone in the last chunk":
    every other draw of that chunk is at -2444."""
    N, n, P = 1, 10, 13
    _three_chunks(N)
    rng = np.random.default_rng(92)
    from demc_amd import families as F
    prob = dict(fam=F.FAM_GAUSSIAN, data=np.array([0.0]), dims=[1], hyper=None, D=2, pk=[1, 2], pa=[0, 0], pb=[10, 1], pref=[0, 0],
                lo=[-np.inf, 0], hi=[np.inf, np.inf])
    kind = rng.integers(0, 3, S3)
    mu = np.where(kind == 0, rng.normal(1.0, 0.3, S3), np.where(kind == 1, 0.07, rng.uniform(0.5e-3, 2e-3, S3)))
    sg = np.where(kind == 0, 1.0, 1e-3)
    at = WIDE[where]
    if where == "alone in the last chunk":
        mu[2 * L3:], sg[2 * L3:] = 0.07, 1e-3
        kind[2 * L3:] = 1
    mu[at], sg[at] = 0.0, 1e-3
    rows = np.stack([mu, sg], axis=1)
    eng, _ = TP.engine(demc, prob, n, P, rows=rows.reshape(n, P, 2))
    ll = eng.pointwise_loglik(TP.draws_of(eng.export_chains(0, n), 2))
    assert int(np.argmax(ll[:, 0])) == at and ll.max() - ll.min() > 2000 and (ll[:, 0] < ll[at, 0]).sum() == S3 - 1
    assert (kind == 0).any() and (kind == 1).any()
    tot_ref, ref = PC.ref_waic(ll)
    tot, pt = eng.waic(0, n, pointwise=True)
    e = np.abs(pt[0] - ref[0]) / np.array([max(1.0, abs(ref[0, 0])), ref[0, 1], max(1.0, abs(ref[0, 2])), max(1.0, abs(ref[0, 0])) + ref[0, 1]])
    print(f"maximum at {where}: lppd {pt[0, 0]!r} ref {ref[0, 0]!r}; errors lppd {e[0]:.3g} p_waic {e[1]:.3g} mean {e[2]:.3g}")
    assert (e <= BAR).all(), e
    assert abs(tot[3] - tot_ref[3]) <= BAR * max(1.0, abs(tot_ref[3])) and math.isnan(tot[1]) and tot[7] == 0
    eng.close()
