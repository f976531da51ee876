"""demc_bridge on the host: the numpy twins of chains.py held to an mpmath restatement at 40 digits, the edge rules
exactly, the Philox restatement against the known answers, the plan program of csrc/demc_bridgeplan.hpp (tests/bridgeplan_host.cpp) run
under the sanitizers, the closed forms on the twins alone, and the header against the library and both bindings.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bridge_cases as BC
from conftest import setup_engine

ROOT, CSRC, BAR = BC.ROOT, BC.CSRC, BC.BAR
INF = math.inf


def _bars(got, ref):
    return BC.err_in_bars(np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64))


# ---- the twins against 40 digits ------------------------------------------------------------------------------------------------------
BOUNDS = [(-INF, INF), (0.0, INF), (-2.5, INF), (-INF, 6.0), (0.0, 1.0), (-3.0, 0.25)]


def test_transform_and_logjac_against_mpmath(demc):
    worst = 0.0
    for lo, hi in BOUNDS:
        if lo > -INF and hi < INF:
            u = np.array([1e-300, 1e-17, 1e-9, 0.01, 0.3, 0.5, 0.9, 1 - 1e-9, 1 - 2.0 ** -52])
            th = lo + (hi - lo) * u if lo != 0.0 or hi != 1.0 else u
        elif lo > -INF:
            th = lo + np.array([1e-300, 1e-12, 0.3, 1.0, 7.5, 1e6, 1e300])
        elif hi < INF:
            th = hi - np.array([1e-300, 1e-12, 0.3, 1.0, 7.5, 1e6, 1e300])
        else:
            th = np.array([-1e300, -3.5, 0.0, 2.0 ** -1074, 1e300])
        th = th[(th > lo) & (th < hi)]
        xi, lj = demc.bridge_transform(th[:, None], [lo], [hi])
        ref = np.array([BC.mp_transform(t, lo, hi) for t in th])
        # xi of a theta next to a bound carries the rounding of theta - lo: the bar is taken on what was computed from the same difference
        w = max(_bars(xi[:, 0], ref[:, 0]), _bars(lj, ref[:, 1]))
        worst = max(worst, w)
        assert w <= 1.0, (lo, hi, w)
        back, lj2 = demc.chains.bridge_inverse(xi, [lo], [hi])
        assert np.array_equal(lj2, lj)
        inside = np.abs(xi[:, 0]) < 30
        assert (np.abs(back[inside, 0] - th[inside]) <= BAR * np.maximum(1.0, np.abs(th[inside]))).all(), (lo, hi)
    # |xi| large on the two-sided transform: logJ at a given xi, no overflow, against log((hi - lo) s (1 - s))
    for lo, hi in ((0.0, 1.0), (-3.0, 0.25)):
        xi = np.array([-745.0, -700.0, -40.0, -1e-9, 0.0, 1e-9, 36.0, 40.0, 709.0, 745.0])
        th, lj = demc.chains.bridge_inverse(xi[:, None], [lo], [hi])
        assert np.isfinite(lj).all() and (th >= lo).all() and (th <= hi).all()
        w = _bars(lj, [BC.mp_logjac_both(x, lo, hi) for x in xi])
        worst = max(worst, w)
        assert w <= 1.0, (lo, hi, w)
    print(f"transform and logJ: worst {worst:.3g} bars")


def test_a_draw_on_or_outside_a_bound_is_not_finite(demc):
    nan = float("nan")
    xi, lj = demc.bridge_transform(np.array([[0.0, 0.5, 1.0], [-1.0, 1.0, 7.0], [0.5, 0.0, 6.0], [nan, 0.5, 1.0]]), [0.0, 0.0, -INF], [INF, 1.0, 6.0])
    assert np.array_equal(np.isfinite(xi), [[False, True, True], [False, False, False], [True, False, False], [False, True, True]])
    assert xi[0, 0] == -INF and math.isnan(xi[1, 0]) and xi[1, 1] == INF and math.isnan(xi[1, 2]) and xi[2, 1] == -INF and xi[2, 2] == -INF


def test_fit_and_logg_against_mpmath(demc):
    import mpmath
    rng = np.random.default_rng(410)
    worst = 0.0
    for D, n in ((1, 5), (2, 3), (3, 40), (8, 30)):
        A = rng.normal(0, 1, (D, D))
        x = rng.normal(0, 1, (n, D)) @ A.T + 1e3 * rng.normal(0, 1, D)  # a mean far from 0: the corrected two-pass form is needed
        m, L = demc.bridge_fit(x)
        with mpmath.workdps(BC.DIGITS):
            X = mpmath.matrix(x.tolist())
            mu = [mpmath.fsum(X[i, k] for i in range(n)) / n for k in range(D)]
            V = mpmath.matrix(D, D)
            for a in range(D):
                for b in range(D):
                    V[a, b] = mpmath.fsum((X[i, a] - mu[a]) * (X[i, b] - mu[b]) for i in range(n)) / (n - 1)
            Lr = mpmath.cholesky(V)
            m_ref = np.array([float(v) for v in mu])
            L_ref = np.array([[float(Lr[a, b]) for b in range(D)] for a in range(D)])
        cond = np.linalg.cond(L_ref)
        wm, wl = _bars(m, m_ref), _bars(L, L_ref)
        pts = rng.normal(0, 1, (6, D)) @ L.T * np.array([0.1, 1, 1, 3, 10, 30])[:, None] + m
        wg = _bars(demc.chains.bridge_logg(pts, m, L), [BC.mp_logg(p, m, L) for p in pts])
        print(f"D={D} n={n} cond(L)={cond:.3g}: m {wm:.3g} L {wl:.3g} log g {wg:.3g} bars")
        worst = max(worst, wm, wl, wg)
    assert worst <= 1.0
    with pytest.raises(ValueError, match="pivot 1 of 2 is not positive"):
        demc.chains.bridge_cholesky(np.ones((2, 2)))
    with pytest.raises(ValueError, match="pivot 0"):
        demc.bridge_fit(np.array([[1.0, 2.0], [1.0, 3.0], [1.0, 5.0]]))


def _logs(rng, n1, n2, spread):
    l1 = rng.normal(-300.0, 1.0, n1)
    l2 = l1.mean() - np.abs(rng.normal(0.0, spread, n2))
    return l1, l2


def test_iteration_against_mpmath(demc):
    rng = np.random.default_rng(411)
    for n1, n2, spread in ((40, 40, 1.0), (30, 7, 3.0), (7, 60, 0.3), (50, 50, 600.0)):
        l1, l2 = _logs(rng, n1, n2, spread)
        if spread > 100:  # more than 1500 log units between the extremes of the two vectors
            l1[0], l2[0], l2[1] = l1.max() - 800.0, l1.max() - 1600.0, l1.max() + 20.0
            assert max(l1.max(), l2.max()) - min(l1.min(), l2.min()) > 1500
        with np.errstate(all="raise"):  # no overflow, no invalid operation on the way
            got = demc.bridge_from_logs(l1, l2)
        ref = BC.mp_bridge(l1, l2)
        w = [_bars([got.logml], [ref[0]]), _bars([got.re2_prop], [ref[1]]), _bars([got.re2_post_iid], [ref[2]])]
        print(f"N1={n1} N2={n2} spread {spread}: logml {got.logml:.6f}, {int(got.n_iter)} iterations (mpmath {ref[3]}); bars {w}")
        # (the last case overlaps so poorly that the fixed point is approached at a rate near 1: both stop at 1000 iterations, on the same value)
        assert bool(got.converged) == (ref[3] < 1000) and (got.converged or spread > 100) and all(math.isfinite(v) for v in got.out[[0, 1, 2, 8, 11]]) and max(w) <= 1.0 and abs(got.n_iter - ref[3]) <= 1
        assert got.l_star == l1.max() and (got.rel_change <= 1e-10) == bool(got.converged) and got.n1 == n1 and got.n2 == n2


def test_edge_rules_exactly(demc):
    rng = np.random.default_rng(412)
    l1, l2 = _logs(rng, 30, 30, 1.0)
    base = demc.bridge_from_logs(l1, l2)
    # a proposal draw with lp = -Inf contributes 0 and is counted: the same as a draw whose term is 0, with N2 unchanged
    z = l2.copy()
    z[[3, 17]] = -INF
    got = demc.bridge_from_logs(l1, z)
    ref = BC.mp_bridge(l1, z)
    assert got.n_zero_prop == 2 and got.n_nonfinite == 0 and got.n2 == 30 and got.converged and got.logml < base.logml
    assert _bars([got.logml, got.re2_prop, got.re2_post_iid], ref[:3]) <= 1.0
    lp2 = np.zeros(30)
    lp2[5] = -INF
    assert demc.bridge_from_logs(l1, l2, lp2=lp2).n_zero_prop == 1
    # a -Inf among l1 is a posterior draw of density 0 relative to g: allowed, its term is 1 / (s2 r)
    y = l1.copy()
    y[4] = -INF
    got = demc.bridge_from_logs(y, l2)
    assert got.n_nonfinite == 0 and math.isfinite(got.logml) and _bars([got.logml], [BC.mp_bridge(y, l2)[0]]) <= 1.0
    # NaN or +Inf anywhere: logml NaN, counted, no iteration
    for vec, bad in ((0, math.nan), (0, INF), (1, math.nan), (1, INF)):
        a, b = l1.copy(), l2.copy()
        (a if vec == 0 else b)[7] = bad
        (a if vec == 0 else b)[9] = bad
        got = demc.bridge_from_logs(a, b)
        assert got.n_nonfinite == 2 and math.isnan(got.logml) and math.isnan(got.re2_prop) and math.isnan(got.re2_post_iid) and got.n_iter == 0 and not got.converged
        assert got.l_star == (np.nanmax(a) if bad != INF or vec == 1 else INF)
    none = demc.bridge_from_logs(np.full(5, -INF), l2)
    assert math.isnan(none.logml) and none.l_star == -INF and none.n_iter == 0 and not none.converged and none.n_nonfinite == 0 and math.isnan(none.rel_change)
    # an iterate that is not a positive finite number stops the iteration: counted, not converged, NaN outputs, n_nonfinite 0, and no
    # exception.  Proposal draws 2000 or 760 log units below l*: every e^(-x2) is +Inf, every term of the numerator is 0, r_1 = 0
    for drop in (2000.0, 760.0):
        trace = []
        got = demc.bridge_from_logs(l1, np.full(30, l1.max() - drop), n_fit=17, trace=trace)
        assert got.n_iter == 1 and not got.converged and got.n_nonfinite == 0 and got.n_zero_prop == 0 and got.l_star == l1.max() and got.n_fit == 17
        assert all(math.isnan(v) for v in (got.logml, got.re2_prop, got.re2_post_iid, got.rel_change)) and math.isnan(got.se())
        assert len(trace) == 1 and trace[0][0] == 0.0 and math.isnan(trace[0][1])
        assert "NOT converged" in repr(got)
    # ... and a mean of f1 whose square underflows divides as the device's FP64 does (0 / 0 = NaN), it does not raise either
    tiny = demc.bridge_from_logs(np.array([0.0, -1.0]), np.array([-700.0, -700.0]))
    assert math.isfinite(tiny.logml) and math.isnan(tiny.re2_prop) and math.isfinite(tiny.re2_post_iid) and tiny.n_iter == 1000 and not tiny.converged
    # the record of a converged call carries its trace: the last entry is (r, rel_change)
    trace = []
    again = demc.bridge_from_logs(l1, l2, trace=trace)
    assert again.out.tobytes() == base.out.tobytes() and len(trace) == base.n_iter and trace[-1][1] == base.rel_change and math.log(trace[-1][0]) + base.l_star == base.logml
    one = demc.bridge_from_logs(l1, l2[:1])
    assert math.isnan(one.re2_prop) and math.isfinite(one.logml) and math.isnan(one.se())
    assert base.se(1.0) == math.sqrt(base.re2_prop + base.re2_post_iid) and base.se(4.0) == math.sqrt(base.re2_prop + 4.0 * base.re2_post_iid)


def test_compare_bridge(demc):
    rng = np.random.default_rng(413)
    a = demc.bridge_from_logs(*_logs(rng, 30, 30, 1.0))
    b = demc.bridge_from_logs(*_logs(rng, 30, 30, 1.0))
    b.rho = 3.0
    c = demc.compare_bridge(a, b)
    assert c["log_bf"] == a.logml - b.logml and c["se"] == math.sqrt(a.se(1.0) ** 2 + b.se(3.0) ** 2)
    assert abs(c["prob_a"] - 1 / (1 + math.exp(-c["log_bf"]))) < 1e-15 and c["prob_a"] + c["prob_b"] == 1.0
    d = demc.compare_bridge(a, b, prior_odds=math.exp(-c["log_bf"]))
    assert abs(d["prob_a"] - 0.5) < 1e-12
    far = demc.Bridge([-2000.0] + [0.0] * 11)
    assert demc.compare_bridge(a, far)["prob_a"] == 1.0 and demc.compare_bridge(far, a)["prob_a"] == 0.0
    assert demc.chains.BRIDGE_OUT[0] == "logml" and len(demc.chains.BRIDGE_OUT) == demc._ffi.BRIDGE_NOUT == 12


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_philox_restatement_matches_the_known_answers(demc):
    """Random123's kat_vectors for philox4x32-10, the ones tests/test_oracle_kat.py holds the oracle to"""
    P = demc.chains.philox4x32_10
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert [int(w) for w in P([np.uint64(c) for c in ctr], key)] == want
    # ... and the addressing of csrc/demc_philox.hpp, as tests/weighted_pick_cases.py restates it
    import weighted_pick_cases as W
    seed, n, D = 0x1234567887654321, 70, 5
    z = demc.chains.bridge_normals(n, D, seed)
    ent, blk = np.meshgrid(np.arange(n), np.arange(3), indexing="ij")
    r = W.philox_blocks(seed, demc.chains.BRIDGE_STREAM, 0, 0, ent, blk)
    u1, u2 = W.u53_array(r[..., 0], r[..., 1]), W.u53_array(r[..., 2], r[..., 3])
    rad = np.sqrt(-2.0 * np.log(1.0 - u1))
    want = np.stack([rad * np.cos(2 * math.pi * u2), rad * np.sin(2 * math.pi * u2)], -1).reshape(n, 6)[:, :D]
    assert np.array_equal(z, want) and z.shape == (n, D)
    assert np.array_equal(demc.chains.bridge_normals(n, 4, seed), z[:, :4])  # odd D: the last sine is unused, nothing else moves
    assert not np.array_equal(demc.chains.bridge_normals(n, D, seed + 1), z)
    big = demc.chains.bridge_normals(20000, 2, 5)
    assert abs(big.mean()) < 0.03 and abs(big.std() - 1) < 0.03 and abs(np.corrcoef(big.T)[0, 1]) < 0.03


def test_draws_follow_the_definition(demc):
    rng = np.random.default_rng(414)
    D = 3
    m, L = rng.normal(0, 1, D), np.tril(rng.normal(0, 1, (D, D))) + 2 * np.eye(D)
    lo, hi = [-INF, 0.0, -1.0], [INF, INF, 2.0]
    th, lj, lg = demc.bridge_draws(m, L, 50, 9, lo, hi)
    z = demc.chains.bridge_normals(50, D, 9)
    xi = m + z @ L.T
    assert _bars(demc.bridge_transform(th, lo, hi)[0], xi) <= 1.0 and (th[:, 1] > 0).all() and (th[:, 2] > -1).all() and (th[:, 2] < 2).all()
    assert _bars(lg, demc.chains.bridge_logg(xi, m, L)) <= 1.0 and _bars(lg, [BC.mp_logg(x, m, L) for x in xi]) <= 1.0
    assert _bars(lj, demc.bridge_transform(th, lo, hi)[1]) <= 1.0


# ---- the plan program -------------------------------------------------------------------------------------------------------------------
def test_plan_program_under_the_sanitizers():
    run = subprocess.run([BC.program()], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr[-4000:]
    assert re.search(r"^\d+ checks, 0 failures$", run.stdout.strip())


def test_plan_header_is_host_only():
    deps = subprocess.run(["g++", "-std=c++17", "-MM", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "bridgeplan_host.cpp")],
                          capture_output=True, text=True)
    assert deps.returncode == 0, deps.stderr
    assert "demc_bridgeplan.hpp" in deps.stdout and "hip" not in deps.stdout.lower().replace("demc_hip", "") and "rocm" not in deps.stdout.lower()
    text = open(os.path.join(CSRC, "demc_bridgeplan.hpp")).read()
    assert "#include <hip" not in text and '#include "demc_philox.hpp"' not in text
    run_cpp = open(os.path.join(CSRC, "demc_bridge.cpp")).read()
    assert "kBridgeStream" in run_cpp and "atomicAdd(&p.word" in run_cpp and "double*" not in re.findall(r"atomic\w+\(([^,]*),", run_cpp)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "demc_bridge.cpp" in makefile and "$(OBJ).bridge.o" in makefile


def test_transform_of_the_header_is_the_twins(demc):
    reqs, th_all = [], []
    for lo, hi in BOUNDS:
        for t in (-4.0, -0.3, 1e-9, 0.1, 0.2, 0.9, 3.0, 5.9):
            if lo < t < hi:
                reqs.append(f"T {t!r} {lo!r} {hi!r}")
                th_all.append((t, lo, hi))
    run = subprocess.run([BC.program(), "--dump"], input="\n".join(reqs) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stderr
    rows = [[float(v) for v in line.split()] for line in run.stdout.splitlines()]
    assert len(rows) == len(reqs)
    for (t, lo, hi), (xi, lj, back) in zip(th_all, rows):
        x, j = demc.bridge_transform(np.array([[t]]), [lo], [hi])
        assert _bars([xi, lj], [x[0, 0], j[0]]) <= 1e-3 and abs(back - t) <= 1e-12 * max(1.0, abs(t))  # the same operations: a few ulps of libm


def test_geometry_restated_is_the_planners(demc):
    """bridge_cases.geometry, which every GPU case asserts its path through, against plan_bridge (and plan_cov for the fit) itself"""
    grid = [(R, P, D, n) for R in (2, 3, 7, 130) for P in (3, 13, 16, 512) for D in (1, 2) for n in (0, 1, 63, 64, 65, 1024, 1025, 2049, 262144, 262145, 1 << 22)]
    shapes = BC.GPU_SHAPES + grid
    for shape, plan in zip(shapes, BC.plan_geometry(shapes)):
        g = BC.geometry(*shape)
        assert {k: g[k] for k in BC.GEOMETRY_KEYS} == plan, (shape, g, plan)
    g = BC.geometry(BC.WIN_R, BC.WIN_P, 2, 2049)
    assert (g["W1"], g["W2"], g["logs_blocks"], g["N2"] - (g["logs_blocks"] - 1) * BC.BRIDGE_WG, g["cov_chunks"], g["solve_blocks"]) == (2, 3, 9, 1, 3, 17)
    g = BC.geometry(2, BC.CAP_P, 2, BC.CAP_N2)
    assert (g["W2"], g["W1"], g["chunks2"]) == (256, 1, 513) and BC.geometry(2, BC.CAP_P, 2, BC.CAP_N2 - 1)["W2"] == 256 and BC.geometry(2, BC.CAP_P, 2, BC.CAP_N2 - 1025)["W2"] == 255
    assert -(-BC.CAP_N2 // (256 * BC.BRIDGE_WG)) == 5 and -(-(BC.CAP_N2 - 1) // (256 * BC.BRIDGE_WG)) == 4  # a thread's fifth element
    run = subprocess.run([BC.program(), "--dump"], input="G 2 3 3 0\nG 4 3 65 0\n", capture_output=True, text=True, timeout=120)
    assert run.stdout.splitlines() == [f"refused={demc._ffi.EINVAL} message=demc_bridge: the fit half holds N_fit = 3 draws, the covariance of the proposal needs more than D = 3; pass a wider window",
                                       f"refused={demc._ffi.EINVAL} message=demc_bridge: D = 65 is above the cap of 64 (DEMC_BRIDGE_MAX_D: the covariance of the proposal)"], run.stdout


# ---- the split windows of the iteration, on the twins alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.WINDOWS))
def test_split_windows_meet_their_conditions(demc, orc, name):
    """each window of the device's iteration tests meets the condition it exists for, on the twins with the oracle's log posterior"""
    w = BC.WINDOWS[name]
    prob, rows = BC.split_window(name)
    o = orc.Oracle(n_groups=1, Np=4, D=prob["D"], n_rows=1)
    setup_engine(o, prob)
    trace = []
    b, l1, l2 = BC.twin_bridge(demc, rows, prob["lo"], prob["hi"], o.logpost, n_prop=w["n_prop"], seed=BC.WINDOW_DRAW_SEED, trace=trace)
    o.close()
    print(f"{name}: {b!r}, n_iter {int(b.n_iter)}, the last changes {[f'{t[1]:.3g}' for t in trace[-3:]]}")
    BC.window_condition(name, b, trace)
    assert np.isfinite(l1).all() and np.isfinite(l2).all() and b.n_nonfinite == 0 and b.n_zero_prop == 0
    if w["kind"] == "limit":
        # the sequence is stable, not oscillating: 40 digits and FP64 stop on the same value, so the device's logml is held to the bar too
        ref = BC.mp_bridge(l1, l2)
        bars = [_bars([b.logml], [ref[0]]), _bars([b.re2_prop], [ref[1]]), _bars([b.re2_post_iid], [ref[2]])]
        print(f"{name}: against 40 digits {bars} bars, mpmath ran {ref[3]} iterations")
        assert ref[3] == 1000 and max(bars) <= 1.0
    if w["kind"] == "stops":
        assert all(math.isnan(v) for v in (b.logml, b.re2_prop, b.re2_post_iid, b.rel_change)) and math.isfinite(b.l_star)
        assert (b.n_fit, b.n1, b.n2) == ((w["R"] // 2) * w["P"], (w["R"] - w["R"] // 2) * w["P"], w["n_prop"])


# ---- closed forms, on the twins alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["binomial", "mvn_full"])
def test_closed_forms_on_the_twins(demc, orc, family):
    prob, exact, rows, (th_hat, log_post_hat) = BC.closed_problem(family)
    o = orc.Oracle(n_groups=1, Np=4, D=prob["D"], n_rows=1)
    setup_engine(o, prob)
    logpost = lambda th: np.concatenate([o.logpost(np.ascontiguousarray(th[i:i + 4096])) for i in range(0, len(th), 4096)])  # noqa: E731
    # the closed form is lp(theta_hat) - log posterior density(theta_hat) on the oracle's log posterior: the constants are checked
    identity = float(logpost(np.asarray(th_hat, dtype=np.float64)[None, :])[0]) - log_post_hat
    print(f"{family}: closed form {exact:.12f}, lp - log posterior at theta_hat {identity:.12f}")
    assert abs(identity - exact) <= BAR * max(1.0, abs(exact))
    b, l1, l2 = BC.twin_bridge(demc, rows, prob["lo"], prob["hi"], logpost, seed=5)
    o.close()
    print(f"{family}: twin logml {b.logml:.6f}, difference {b.logml - exact:.2e} = {abs(b.logml - exact) / b.se(1.0):.2f} se (se {b.se(1.0):.2e}), {int(b.n_iter)} iterations")
    assert b.converged and b.n_nonfinite == 0 and b.n1 == 1024 and b.n2 == 1024 and b.n_fit == 1024
    assert abs(b.logml - exact) <= 5 * b.se(1.0)


# ---- the header, the library and both bindings ------------------------------------------------------------------------------------------
def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demc_bridge.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return text, protos


def test_header_library_and_python_binding_agree(demc):
    import ctypes as C
    text, protos = _prototypes()
    assert sorted(protos) == sorted(demc._ffi.BRIDGE_EXPORTS) == ["demc_bridge"]
    for other in (demc._ffi.EXPORTS, demc._ffi.SUMMARY_EXPORTS, demc._ffi.QUANTILE_EXPORTS, demc._ffi.COV_EXPORTS, demc._ffi.PW_EXPORTS, demc._ffi.LOO_EXPORTS):
        assert not set(protos) & set(other), "declared in another header as well"
    for h in ("demc.h", "demc_summary.h", "demc_quantile.h", "demc_cov.h", "demc_pointwise.h", "demc_loo.h"):
        assert "demc_bridge" not in open(os.path.join(ROOT, "include", h)).read(), h
    lib = demc._ffi.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double*": C.POINTER(C.c_double), "demc_handle*": C.c_void_p}
    ret, args = protos["demc_bridge"]
    fn = lib.demc_bridge
    assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args] and len(args) == 9
    for name, value in (("NOUT", 12), ("MAX_D", 64), ("MAX_DRAWS", 4194304), ("MAX_ITER", 1000)):
        assert re.search(rf"#define DEMC_BRIDGE_{name} {value}\b", text) and getattr(demc._ffi, f"BRIDGE_{name}") == value
    assert '#include "demc.h"' in text
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "demc_bridge.h")])
    assert callable(getattr(demc._ffi.HipEngine, "bridge")) and callable(getattr(demc._ffi.HipEngine, "bridge_served"))


def test_julia_ccall_matches_the_prototype(demc):
    import test_julia_shim as J
    _, protos = _prototypes()
    main_jl = open(os.path.join(ROOT, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPBridge.jl")' in main_jl and "demc_bridge" not in main_jl
    jl = open(os.path.join(ROOT, "julia", "DEMCHIPBridge.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= {"demc_bridge"}
    main = J.c_prototypes()
    for m in calls:
        end = J.balanced(jl, m.end() - 1)
        jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
        if m.group(1) in protos:
            cret, ctypes_ = protos[m.group(1)]
            assert jtypes == [J.julia_type(c) for c in ctypes_], (jtypes, ctypes_)
            assert re.match(r"::([A-Za-z0-9{}]+)", jl[end:]).group(1) == J.julia_type(cret)
        else:
            assert m.group(1) in main and jtypes == [J.julia_type(c) for c in main[m.group(1)][1]], (m.group(1), jtypes)
    names = re.search(r"const BRIDGE_OUT = \(([^)]*)\)", jl).group(1)
    assert tuple(n.strip().lstrip(":") for n in names.split(",")) == demc.chains.BRIDGE_OUT


def test_bridge_kernels_use_no_scratch(tmp_path, demc):
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_bridge_" in k[0]]
    assert len(ks) == 11, [k[0] for k in ks]
    for name, regs, agpr, wg, scratch in ks:
        assert scratch == 0 and regs <= 128 and wg in (64, 256), (name, regs, wg, scratch)


def test_summarize_refuses_before_the_run(demc):
    """an engine without bridge, and what bridge_served refuses, end the run before its first step"""
    class NoBridge:
        def __init__(self, **cfg):
            pass

        def close(self):
            pass

    rng = np.random.default_rng(1)
    sp = lambda: [rng.uniform(0.1, 0.9)]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, names=("θ",), data=dict(N=[10.0], k=[4.0]), prior_loglike=demc.Priors(θ=demc.Beta(1, 1)), loglike=demc.BinomialLikelihood())
    de = demc.DE(sample_prior=sp, bounds=((0.0, 1.0),), burnin=10, Np=4)
    with pytest.raises(demc.DemcError, match="needs an engine with bridge"):
        demc.summarize(model, de, demc.HIPBackend(seed=1), 20, bridge=True, engine_factory=NoBridge)
    with pytest.raises(ValueError, match="bridge= takes True or dict"):
        demc.summarize(model, de, demc.HIPBackend(seed=1), 20, bridge=dict(draws=5), engine_factory=NoBridge)
