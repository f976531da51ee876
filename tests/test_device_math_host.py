"""What tests/test_gpu_device_math.py rests on, checked without a GPU: the probe compiles for gfx950 with the library's flags, the
80-bit references agree with 40-digit arithmetic, the generated arguments contain the ties, clamps and specials they are meant to
(by count, so that a later edit cannot drop them silently), and the request / result files round-trip through a numpy stand-in
for the probe."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import device_math_cases as C


def test_probe_compiles_for_gfx950_with_the_library_flags(tmp_path):
    cmd = C.probe_build_command(str(tmp_path / "device_math_probe"))
    mk = open(os.path.join(C.CSRC, "Makefile")).read()
    for flag in ("-O3", "-std=c++17", "-ffp-contract=off"):
        assert flag in mk and flag in cmd, flag
    assert "--offload-arch=$(ARCH)" in mk and "--offload-arch=gfx950" in cmd and '-DDEMC_ARCH_STR="gfx950"' in cmd
    assert "-shared" not in cmd and "-fPIC" not in cmd
    if shutil.which(cmd[0]) is None:
        pytest.skip("needs hipcc")
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    assert os.path.getsize(cmd[-1]) > 0


def test_longdouble_references_agree_with_40_digits():
    """2000 points per helper: exp, softplus and 1/x in np.longdouble against mpmath to 1e-18 relative"""
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.default_rng(5)
    a = rng.uniform(-700.0, 0.0, 2000)
    x = np.concatenate([rng.uniform(-40, 40, 1500), rng.uniform(-700, 700, 500)])
    v = np.exp(rng.uniform(np.log(1e-300), np.log(1e300), 2000))
    mpf = mpmath.mpf
    for name, pts, got, want in (
            ("exp", a, C.exp_ref(a), [mpmath.exp(mpf(float(t))) for t in a]),
            ("softplus", x, C.softplus_ref(x), [max(mpf(float(t)), 0) + mpmath.log1p(mpmath.exp(-abs(mpf(float(t))))) for t in x]),
            ("1/x", v, C.recip_ref(v), [1 / mpf(float(t)) for t in v])):
        # an 80-bit number as the exact sum of two doubles
        hi = got.astype(np.float64)
        lo = (got - hi.astype(C.ld)).astype(np.float64)
        rel = np.array([float(abs((mpf(float(h)) + mpf(float(l)) - w) / w)) for h, l, w in zip(hi, lo, want)])
        print("%s: 80-bit against 40 digits, largest relative difference %.3g at %r" % (name, rel.max(), pts[rel.argmax()]))
        assert rel.max() < 1e-18, name
    w0, w1 = rng.integers(0, 2 ** 32, (2, 500)).astype(np.float64)
    rx, ry, rad = C.box_muller_ref_ld(w0, w1)
    exact = lambda g: mpf(float(np.float64(g))) + mpf(float(g - C.ld(np.float64(g))))  # an 80-bit number as two doubles
    for (mx, my, mr), gx, gy in zip(C.box_muller_ref(w0, w1), rx, ry):
        assert abs(exact(gx) - mx) < 1e-18 * mr and abs(exact(gy) - my) < 1e-18 * mr


def test_generated_arguments_contain_the_ties_clamps_and_specials():
    cases = C.all_cases()
    count = lambda name: {k: s.stop - s.start for k, s in cases[name][3].items()}
    has = lambda x, vals: all(((x == v) | (np.isnan(x) & np.isnan(v))).any() for v in vals)

    _, x, _, w = cases["exp_nonpos"]
    assert count("exp_nonpos") == dict(random=200000, ties=3 * (2 * 1011 - 1), specials=7, nan=1)
    t = x[w["ties"]][1::3].astype(C.ld) / np.log(C.ld(2))  # the centres: n +- 1/2 to the rounding of a
    assert np.abs(np.abs(t - np.rint(t)) - 0.5).max() < 1e-12 and t.min() < -1010 and t.max() > -0.51
    assert has(x, [0.0, -5e-324, -700.0, -700.0000001, -1e300, -np.inf, np.nan]) and np.signbit(x[x == 0.0]).any()
    assert x[w["random"]].min() >= -700.0 and x[w["random"]].max() <= 0.0

    for form in ("softplus_fast", "softplus_tab"):
        _, x, _, w = cases[form]
        kspc = C.softplus_header()["kSpC"]
        nk = int(np.floor(40 * kspc))
        assert count(form) == dict(table_test=392005, k_ties=2 * 3 * nk, j_ties=2 * 3 * 128, specials=6, below_clamp=4, inf=1, nan=1)
        k = x[w["k_ties"]][1:3 * nk:3].astype(C.ld) * C.ld(kspc)
        assert np.abs(np.abs(k - np.rint(k)) - 0.5).max() < 1e-10 and k.min() < -(nk - 1) and k.max() > -0.51
        j = 128 * np.exp(x[w["j_ties"]][1:3 * 128:3].astype(C.ld))
        assert np.abs(j - (np.arange(128) + 0.5)).max() < 1e-12
        assert has(x, [0.0, 700.0, -700.0, 745.0, -745.0, 1e300, -1e300, np.inf, -np.inf, np.nan])
        # the point set of tests/test_tables.py, seed and all
        rng = np.random.default_rng(3)
        assert np.array_equal(x[:300000], rng.uniform(-40, 40, 300000)) and x[w["table_test"]][-1] == -690.0

    _, x, _, w = cases["recip_pos"]
    assert count("recip_pos") == dict(random=200000, pow2=1993, one=3, decision_times=22001, denormal=3)
    assert x[w["random"]].min() >= 1e-300 and x[w["random"]].max() <= 1e300 and x[w["random"]].min() < 1e-290 and x[w["random"]].max() > 1e290
    p = x[w["pow2"]]
    assert p.min() >= 1e-300 and p.min() / 2 < 1e-300 and p.max() <= 1e300 and p.max() * 2 > 1e300 and (np.frexp(p)[0] == 0.5).all()
    assert list(x[w["one"]]) == [1 - 2.0 ** -53, 1.0, 1 + 2.0 ** -52]
    assert x[w["decision_times"]].min() == 1e-3 and x[w["decision_times"]].max() == 60.0
    assert (x[w["denormal"]] < 2.2250738585072014e-308).all()

    _, x, _, w = cases["phi_table"]
    ints = C.header_ints("demc_phi_table.hpp")
    assert ints["kPhiPerUnit"] == C.PHI_S and 8.5 * ints["kPhiPerUnit"] == C.PHI_HALF and ints["kPhiIntervals"] == 2 * C.PHI_HALF + 1
    assert count("phi_table") == dict(grid=400001, ties=3 * 544, ends=6, beyond=6, nan=1)
    t = x[w["ties"]][1::3] + C.PHI_HALF
    assert np.array_equal(t, np.arange(544) + 0.5)
    assert has(x, [-C.PHI_HALF, C.PHI_HALF, 30 * C.PHI_S, -30 * C.PHI_S, 1e300, -1e300, np.inf, -np.inf, np.nan])
    assert np.array_equal(x[w["grid"]], np.linspace(-8.5, 8.5, 400001) * C.PHI_S)

    _, x, _, w = cases["log_phi_neg"]
    ints = C.header_ints("demc_logphi_table.hpp")
    assert ints["kLogPhiRows"] == 377 and ints["kLogPhiPerUnit"] == 8
    assert count("log_phi_neg") == dict(table_test=8001, ties=3 * 376, clamps=4, below=5, far=2000, far_special=3, nan=1)
    assert np.array_equal(8 * x[w["ties"]][1::3] + 68.0, np.arange(376) + 0.5)
    assert x[w["far"]].min() == np.nextafter(38.5, np.inf) and x[w["far"]].max() == 1e3
    assert has(x, [-8.5, 38.5, np.nextafter(-8.5, -np.inf), -1e300, -np.inf, 1e150, 1e300, np.inf, np.nan])

    total = 0
    for name, na in C.LBA_NA.items():
        _, x, y, w = cases[name]
        c = count(name)
        total += c["random"]
        assert c["tail"] == 3 * 2 * 2 * len(C.LBA_TAIL_DRIFTS) * na and c["dead"] == 5
        assert set(y[0]) == set(range(1, na + 1)) and (y[1 + na:5] == 0).all()
        tl = w["tail"]
        t, A, k = x[tl] - y[7, tl], y[5, tl], y[6, tl]
        assert {round(v, 9) for v in t} == {1e-3, 5.0, 60.0} and set(A) == {1e-3, 5.0}
        n1, n2 = k / t - y[1:1 + na, tl], (A + k) / t - y[1:1 + na, tl]
        assert (y[1:1 + na, tl] < 0).any() and (n1 > 8.5).any() and (n2 < -8.5).any()
        d = w["dead"]
        assert np.isnan(x[d]).sum() == 1 and (~(x[d] - y[7, d] > 1e-300)).all()
        r = w["random"]  # drawn like conftest.make_problem("lba")
        assert 0.45 <= x[r].min() and x[r].max() <= 1.6 and 0.5 <= y[1:1 + na, r].min() and y[1:1 + na, r].max() <= 4.0
        assert 0.5 <= y[5, r].min() and y[5, r].max() <= 1.1 and 0.05 <= y[6, r].min() and y[6, r].max() <= 0.4 and y[7, r].max() <= 0.405
    assert total == 20000

    _, x, y, _ = cases["prior_term"]
    assert [int((y[0] == k).sum()) for k in C.PRIOR_KINDS] == [C.PRIOR_PER_KIND] * 8 and C.PRIOR_PER_KIND == 200
    par = {(int(k), a, b) for k, a, b in y.T}
    assert {(4, 0.5, 0.5), (4, 1.0, 1.0), (6, 0.5, 1.0), (6, 1.0, 2.0)} <= par and len(par) == sum(len(v) for v in C.PRIOR_PARAMS.values())
    for k, a, b in par:
        xs = x[(y[0] == k) & (y[1] == a) & (y[2] == b)]
        lo, hi = C.prior_support(k, a, b)
        ends = [v for v in (lo, hi) if np.isfinite(v)] or [0.0]
        for e in ends:
            assert has(xs, [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]), (k, a, b, e)
        assert has(xs, [1e-300, 1e300, -1e300])
        assert ((xs > lo) & (xs < hi)).sum() >= 25

    _, x, y, w = cases["box_muller"]
    assert count("box_muller") == dict(random=100000, specials=25)
    assert {(int(a), int(b)) for a, b in zip(x[w["specials"]], y[0][w["specials"]])} == {(a, b) for a in C.BM_WORDS for b in C.BM_WORDS}
    assert x.max() < 2 ** 32 and y.max() < 2 ** 32 and (x == np.floor(x)).all()


def test_request_and_result_files_round_trip_through_the_stand_in(tmp_path):
    cases = C.all_cases()
    req, res = str(tmp_path / "request.bin"), str(tmp_path / "result.bin")
    sent = [(fn, x, y) for fn, x, y, _ in cases.values()]
    C.write_request(req, sent)
    back = C.read_request(req)
    assert len(back) == len(sent)
    for (fn, x, y), (fn2, x2, y2) in zip(sent, back):
        assert fn == fn2 and np.array_equal(x.view(np.uint64), x2.view(np.uint64))  # (bits: the NaN and -0.0 survive)
        assert y2.shape == (C.YCOLS[fn], x.size) and (y is None or np.array_equal(np.asarray(y, np.float64).view(np.uint64), y2.view(np.uint64)))
    outs = C.standin(back)
    C.write_result(res, outs)
    got = C.read_result(res)
    assert [(fn, o.shape) for fn, o in got] == [(fn, (2, x.size)) for fn, x, _ in sent]
    for (_, a), (_, b) in zip(outs, got):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    with open(res, "ab") as f:
        f.write(b"\0" * 8)
    with pytest.raises(AssertionError):
        C.read_result(res)
    # the stand-in (libm forms, float64) and the references describe the same functions
    out = {name: o for name, (_, o) in zip(cases, got)}
    _, x, _, w = cases["exp_nonpos"]
    assert C.rel_err(out["exp_nonpos"][0][w["random"]], C.exp_ref(x[w["random"]])).max() < 1e-15
    _, x, _, w = cases["softplus_tab"]
    assert C.rel_err(out["softplus_tab"][0][w["table_test"]], C.softplus_ref(x[w["table_test"]])).max() < 1e-15
    _, x, _, w = cases["phi_table"]
    i = np.arange(w["grid"].start, w["grid"].stop, 1000)
    P, f = C.phi_ref(x[i] / C.PHI_S)
    assert C.mp_abs_err(out["phi_table"][1][i], P).max() < 1e-15 and C.mp_abs_err(C.PHI_S * out["phi_table"][0][i], f).max() < 1e-15
    _, x, _, w = cases["log_phi_neg"]
    i = np.arange(w["table_test"].start, w["table_test"].stop, 20)
    g = C.log_phi_neg_ref(x[i])
    assert (C.mp_abs_err(out["log_phi_neg"][0][i], g) / np.maximum(1.0, np.abs([float(v) for v in g]))).max() < 3e-15  # (scipy's log_ndtr)
    for name, na in C.LBA_NA.items():
        _, x, y, w = cases[name]
        i = np.concatenate([np.arange(300), np.arange(w["dead"].start, w["dead"].stop)])
        err, base, kpart, ref = C.lba_check(out[name][0][i], x[i], y[:, i], na)
        assert (err[-5:] == 0).all() and (err[:300] <= 1e-11 * np.abs(ref[:300])).all() and (base[:300] > 0).all() and (kpart[:300] > 0).all()
