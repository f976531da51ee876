"""tests/pointwise_cases.py on the CPU: the numpy closed forms against the 40-digit terms, chains.waic_from_loglik against the
40-digit definition (with its -Inf and NaN rules), and the three conditions on the conditioning cases -- the restated arithmetic of
k_pw_accumulate / k_pw_final is within 0.25 tol on every case, the same arithmetic without its shift is beyond 100 tol on at least
three, and tol <= 1e-7 var on the concentrated ones: a device test at tol proves that the shift is there.  No GPU."""
import math

import numpy as np
import pytest

import pointwise_cases as PC
from conftest import make_problem


@pytest.mark.parametrize("family,kw", [("gaussian", dict(N=40)), ("binomial", dict(N=40)), ("mvn_iso", dict(N=5, d=9)), ("mvn_iso", dict(N=3, d=64)),
                                       ("mvn_full", dict(N=5, d=17)), ("mvn_full", dict(N=3, d=64))])
def test_closed_forms_against_40_digits(family, kw):
    rng = np.random.default_rng(11)
    prob = make_problem(family, rng, **kw)
    theta = prob["init"](4)
    ref, got = PC.ref_terms(prob, theta), PC.closed_terms(prob, theta)
    assert ref.shape == got.shape == (4, kw["N"]) and np.isfinite(ref).all()
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{family} {kw}: worst {err.max():.3g}")
    assert err.max() <= 1e-13
    sub = PC.closed_terms(prob, theta, cols=[kw["N"] - 1, 0])
    assert np.array_equal(sub, got[:, [kw["N"] - 1, 0]])


def test_closed_form_at_the_conditioning_data():
    """x = 50 under mu = 1e-6 z: the column every conditioning case leans on"""
    case = PC.conditioning_cases()[0]
    prob = PC.cond_problem(case)
    th = case["theta"][:40]
    ref, got = PC.ref_terms(prob, th), PC.closed_terms(prob, th)
    assert (np.abs(got - ref) <= 1e-13 * np.maximum(1.0, np.abs(ref))).all()
    assert abs(ref[0, 0] + 1250.9) < 0.1


def _same(a, b, rel):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), (a, b)
    with np.errstate(invalid="ignore"):
        assert (np.abs(a - b)[fin] <= rel * np.maximum(1.0, np.abs(b[fin]))).all(), (a, b)


def test_waic_from_loglik_against_the_definition_in_40_digits(demc):
    rng = np.random.default_rng(5)
    inf, nan = np.inf, np.nan
    plain = rng.normal(-1.4, 0.3, (130, 5))
    some_inf = plain.copy()
    some_inf[7, 1] = some_inf[129, 3] = -inf
    all_inf = plain.copy()
    all_inf[:, 2] = -inf
    a_nan = plain.copy()
    a_nan[44, 0] = nan
    a_nan[3, 4] = -inf
    wide = plain.copy()
    wide[:, 0] = rng.uniform(-2500, -1, 130)  # terms more than 745 apart: exp(l - M) underflows for most of them
    for name, ll in [("plain", plain), ("-Inf in some draws", some_inf), ("-Inf in every draw", all_inf), ("a NaN", a_nan), ("wide", wide),
                     ("S=1", plain[:1]), ("S=2", plain[:2]), ("N=1", plain[:, :1]), ("N=2", plain[:, :2]), ("S=1 N=1", plain[:1, :1])]:
        w = demc.waic_from_loglik(ll)
        tot, pt = PC.ref_waic(ll)
        _same(w.pointwise, pt, 1e-14)
        assert w.totals[6] == tot[6] and w.totals[7] == tot[7], name
        scale = [np.abs(pt[:, 3]).sum(), None, np.abs(pt[:, 1]).sum(), np.abs(pt[:, 0]).sum(), 2 * np.abs(pt[:, 3]).sum(), 2 * np.abs(pt[:, 2]).sum()]
        for j in (0, 2, 3, 4, 5):
            if math.isfinite(tot[j]):
                assert abs(w.totals[j] - tot[j]) <= 1e-14 * max(1.0, scale[j]), (name, j, w.totals[j], tot[j])
            else:
                assert (math.isnan(tot[j]) and math.isnan(w.totals[j])) or w.totals[j] == tot[j], (name, j, w.totals[j], tot[j])
        if math.isfinite(tot[1]):
            assert abs(w.totals[1] - tot[1]) <= 1e-12 * tot[1], (name, w.totals[1], tot[1])
        else:
            assert math.isnan(w.totals[1]) and math.isnan(tot[1]), (name, w.totals[1], tot[1])
    # the rules by name
    tot, pt = PC.ref_waic(some_inf)
    assert math.isfinite(pt[1, 0]) and np.isnan(pt[1, 1:]).all() and tot[7] == 2 and math.isnan(tot[0]) and math.isfinite(tot[3])
    tot, pt = PC.ref_waic(all_inf)
    assert pt[2, 0] == -inf and np.isnan(pt[2, 1:]).all() and tot[3] == -inf and tot[7] == 1
    tot, pt = PC.ref_waic(a_nan)
    assert np.isnan(pt[0]).all() and math.isfinite(pt[4, 0]) and tot[7] == 2 and math.isnan(tot[3])
    assert math.isnan(PC.ref_waic(plain[:, :1])[0][1]) and np.isnan(PC.ref_waic(plain[:1])[1][:, 1]).all()


def test_kernel_walk_on_easy_columns_is_the_definition(demc):
    """the restatement itself: at every chunk length, with the patterns of 5.8, against waic_from_loglik"""
    rng = np.random.default_rng(6)
    ll = rng.normal(-1.4, 0.3, (130, 6))
    ll[50, 1] = -np.inf          # inside the middle chunk of three
    ll[44:88, 2] = -np.inf       # the whole middle chunk: E_c = 0, M_c = -Inf
    ll[88, 3] = np.nan           # the first term of the last chunk
    ll[:, 4] = -np.inf
    ll[:, 5] = rng.uniform(-2500, -1, 130)
    ref = demc.waic_from_loglik(ll).pointwise
    for L in (44, 64, 65, 130, 1):
        lppd, pw, mean = PC.kernel_walk(ll, L)
        _same(lppd, ref[:, 0], 1e-13)
        _same(mean, ref[:, 2], 1e-13)
        fin = np.isfinite(ref[:, 1])
        assert np.array_equal(np.isnan(pw), np.isnan(ref[:, 1])) and (np.abs(pw - ref[:, 1])[fin] <= 1e-12 * ref[fin, 1]).all()
    assert np.allclose(PC.unshifted(ll[:, 0]), ref[0, 1], rtol=1e-10)


def test_conditioning_cases_separate_the_shifted_walk_from_the_unshifted_one():
    cases = PC.conditioning_cases()
    assert len(cases) == len(PC.COND_SHAPES) * len(PC.COND_KINDS) and len({c["name"] for c in cases}) == len(cases)
    beyond, beyond_textbook, delta_binds = [], [], []
    for case in cases:
        prob = PC.cond_problem(case)
        ll = PC.closed_terms(prob, case["theta"])
        S, L = case["S"], case["chunk_len"]
        assert ll.shape == (S, len(case["x"])) and np.isfinite(ll).all()
        L_ = ll.astype(np.longdouble)
        truth = (((L_ - L_.sum(axis=0) / S) ** 2).sum(axis=0) / np.longdouble(S - 1)).astype(np.float64)
        tol, var = PC.tolerance(ll, L)
        assert np.allclose(var, truth, rtol=1e-12) and (tol > 0).all()
        _, pw, _ = PC.kernel_walk(ll, L)
        _, pw_lost, _ = PC.kernel_walk(ll, L, shift=False)
        r_shift = (np.abs(pw - truth) / tol).max()
        r_lost = (np.abs(pw_lost - truth) / tol).max()
        r_text = (np.abs(PC.unshifted(ll) - truth) / tol).max()
        print(f"{case['name']}: shifted {r_shift:.3g} tol, shift lost {r_lost:.3g} tol, textbook {r_text:.3g} tol, tol / var {np.max(tol / var):.3g}")
        assert r_shift <= 0.25, (case["name"], r_shift)  # (a miss here means the bound is wrong: correct the derivation, not the factor)
        if case["concentrated"]:
            assert (tol <= 1e-7 * var).all(), (case["name"], tol / var)
            assert (np.abs(ll).max(axis=0) >= 1e5 * np.sqrt(var)).all()  # |l| >> sd: what check_waic's guard refuses
        if r_lost > 100:
            beyond.append(case["name"])
        if r_text > 100:
            beyond_textbook.append(case["name"])
        if case["kind"] == "far_apart":
            # the column of x = 50: the D term is the largest of the three
            col = ll[:, 0].astype(np.longdouble)
            n_c = np.minimum(L, S - L * np.arange(-(-S // L)))
            starts = L * np.arange(len(n_c))
            mean_c = np.array([col[s:s + n].sum() / n for s, n in zip(starts, n_c)])
            l0 = col[starts]
            v = ((col - col.sum() / S) ** 2).sum() / (S - 1)
            msh = (n_c * (mean_c - l0) ** 2).sum() / (S - 1)
            D = np.abs(mean_c - col.sum() / S).max()
            t1, t2, t3 = L * (v + msh), 2 * D * (np.abs(col).max() + L * np.sqrt(v + msh)), len(n_c) * v
            assert abs(float(4 * PC.U * (t1 + t2 + t3)) - tol[0]) <= 1e-12 * tol[0]  # (the formula, written a second time)
            if t2 > t1 and t2 > t3:
                delta_binds.append(case["name"])
    print("shift lost beyond 100 tol:", beyond)
    print("textbook beyond 100 tol:", beyond_textbook)
    assert len(beyond) >= 3 and len(beyond_textbook) >= 3
    for S in PC.COND_SHAPES:  # every concentrated case, at every size: a device without the shift fails there
        assert f"concentrated_S{S}" in beyond and f"concentrated_S{S}" in beyond_textbook
    assert delta_binds, "no case in which the chunk means are what binds"
