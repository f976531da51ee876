"""The hand-written FP64 helpers of csrc/demc_device.hpp and csrc/demc_kernels.hpp, run as DEVICE code on chosen arguments and
compared point by point with 40-digit (mpmath) and 80-bit (np.longdouble) references: exp_nonpos, softplus_fast, softplus_tab,
recip_pos, phiS_Phi_table, log_Phi_neg_table with its out-of-line log_Phi_neg_far, lba_trial<2 / 3 / 0>, prior_term and box_muller.

tests/device_math_probe.hip includes the kernels' own headers and is compiled with the FLAGS line of csrc/Makefile (read from the
Makefile, less -shared -fPIC), so the helpers are the code the kernels run: FMA where they say fma, the hardware reciprocal, the
magic-number roundings, the exponent-field adds and the device library's log / log1p / sincospi.  The module builds the probe and
runs it ONCE, in a child process, on every case (tests/device_math_cases.py holds the arguments and the references); each test only
reads the answers.  A failed build, a non-zero exit or a timeout fails every test from the kept message and nothing is started on
the GPU again.  Every test prints the largest error it saw and where."""
import subprocess

import numpy as np
import pytest

import device_math_cases as C

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("device_math")
    exe, req, res = (str(d / n) for n in ("device_math_probe", "request.bin", "result.bin"))
    cases = C.all_cases()
    state = dict(cases=cases, out={}, error=None)
    try:
        b = subprocess.run(C.probe_build_command(exe), capture_output=True, text=True, timeout=600)
        if b.returncode != 0:
            state["error"] = "the probe did not build:\n" + b.stderr[-4000:]
            return state
        C.write_request(req, [(fn, x, y) for fn, x, y, _ in cases.values()])
        r = subprocess.run([exe, req, res], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            state["error"] = "the probe ended with status %d:\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            return state
        outs = C.read_result(res)
        if [(fn, o.shape[1]) for fn, o in outs] != [(fn, x.size) for fn, x, _, _ in cases.values()]:
            state["error"] = "the result file does not answer the request case by case"
            return state
        state["out"] = {name: o for name, (_, o) in zip(cases, outs)}
    except subprocess.TimeoutExpired as e:
        state["error"] = "timed out: %r" % (e.cmd,)
    return state


def answers(probe, name):
    """(x, y, where, out[2, n]) of one case; fails from the kept message when the one run of the probe failed"""
    if probe["error"]:
        pytest.fail(probe["error"])
    _, x, y, where = probe["cases"][name]
    return x, y, where, probe["out"][name]


def bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def idx(where, *names):
    return np.concatenate([np.arange(where[n].start, where[n].stop) for n in names])


def report(what, err, at):
    i = int(np.nanargmax(err))
    print("%s: largest %.4g at %r" % (what, err[i], at[i]))
    return float(err[i])


def test_exp_nonpos(probe):
    """relative error below 2.5e-16 (the header's bound) against 80-bit exp on 2e5 random a in [-700, 0], every rounding tie
    a = (n +- 1/2) ln 2 of n = 0 .. -1010 with both neighbours, 0, -0.0, -5e-324, -700, -700.0000001, -1e300 and -Inf; every
    a <= -700 returns the bits of a = -700, +-0 returns exactly 1, and a NaN is read as -700 (fmax).
    Measured on an MI355X: largest relative error 1.35e-16 (a = -244.41)."""
    x, _, w, out = answers(probe, "exp_nonpos")
    got = out[0]
    held = idx(w, "random", "ties", "specials")
    rel = C.rel_err(got[held], C.exp_ref(x[held]))
    report("exp_nonpos, relative", rel, x[held])
    assert rel.max() < 2.5e-16
    at_clamp = got[x == -700.0]
    assert at_clamp.size >= 1 and (x <= -700.0).sum() >= 7  # (the tie (-1010 - 1/2) ln 2 lies below the clamp too)
    assert (bits(got[x <= -700.0]) == bits(at_clamp[0])).all()
    assert (x == 0.0).sum() == 2 and (bits(got[x == 0.0]) == bits(1.0)).all()
    print("exp_nonpos(NaN) = %r" % got[w["nan"]][0])
    assert bits(got[w["nan"]])[0] == bits(at_clamp[0])  # exp(-700) = 9.8596765437597708e-305


@pytest.mark.parametrize("form", ["softplus_fast", "softplus_tab"])
def test_softplus(probe, form):
    """relative error below 6e-16 (tests/test_tables.py's bar and DESIGN 5.2's for the table form; the two serve the same likelihood)
    against 80-bit arithmetic on the point set of test_softplus_table_of_the_row_streaming_kernel, every tie of k
    (a = (k + 1/2) / kSpC, a in [-40, 0)) and of j (128 exp(a) = j + 1/2) with both neighbours and both signs, +-0, +-700, 745,
    1e300.  The argument of exp is clamped at -700 by design, so from -745 down (-745, -1e300, -Inf) the value is pinned to
    [0, 1e-300] instead; +Inf gives +Inf; a NaN is read as -700 by the two fmax and returns softplus(-700) = 9.8596765437597708e-305.
    Measured on an MI355X: largest relative error 4.54e-16 for softplus_fast (x = -7.609; the header said ~2e-16 and
    DESIGN 5.2 2.5e-16 before this was measured) and 4.44e-16 for softplus_tab (x = -36.69)."""
    x, _, w, out = answers(probe, form)
    got = out[0]
    held = idx(w, "table_test", "k_ties", "j_ties", "specials")
    rel = C.rel_err(got[held], C.softplus_ref(x[held]))
    report(form + ", relative", rel, x[held])
    assert rel.max() < 6e-16
    below = got[w["below_clamp"]]
    assert ((below >= 0.0) & (below <= 1e-300)).all(), below
    assert got[w["inf"]][0] == np.inf
    print("%s(NaN) = %r" % (form, got[w["nan"]][0]))
    assert bits(got[w["nan"]])[0] == bits(got[x == -700.0][0])


RECIP_DENORMAL = ["nan", "nan", "4.494232837155791e+307"]  # of 5e-324, 1e-310 and 2.225073858507201e-308, as the MI355X returns them


def test_recip_pos(probe):
    """within 2 ulp -- relative 4.5e-16, the header's "to the last bit or two" -- of the 80-bit quotient on 2e5 x log-uniform in
    [1e-300, 1e300], every power of two in that range, 1 and its neighbours, and the decision times t in [1e-3, 60] lba_trial
    passes.  A denormal x is pinned, not held to a bar (lba_trial guards it with t > 1e-300).
    Measured on an MI355X: largest relative error 1.11e-16 (1 ulp, at x = 1 - 2^-53); 5e-324 and 1e-310 give NaN."""
    x, _, w, out = answers(probe, "recip_pos")
    got = out[0]
    held = idx(w, "random", "pow2", "one", "decision_times")
    rel = C.rel_err(got[held], C.recip_ref(x[held]))
    report("recip_pos, relative", rel, x[held])
    assert rel.max() <= 4.5e-16
    assert (got[w["pow2"]] == 1.0 / x[w["pow2"]]).all()  # (a power of two has an exact reciprocal)
    den = got[w["denormal"]]
    print("recip_pos of the denormals %r = %r" % (list(x[w["denormal"]]), list(den)))
    assert [repr(float(v)) for v in den] == RECIP_DENORMAL


@pytest.mark.parametrize("half", [0, 1])
def test_phi_table(probe, half):
    """(the points in two halves, z < 0 and z >= 0, to keep each case short)  |Ph - Phi| <= 2.5e-16 and |S phS - phi| <= 3e-16 (the bars of tests/test_tables.py) against 40 digits, on a 38 000-point
    subsample of the 400 001-point grid of test_phi_table_of_the_lba_kernels, every row tie zs = i + 1/2 - 8.5 S with both neighbours
    (whichever row the device takes there, the value is held to the bar), |z| = 8.5 with its neighbours; beyond the clamp (+-30,
    +-1e300, +-Inf) the bits of |z| = 8.5; a NaN returns the bits of z = -8.5.
    Measured on an MI355X: largest |Ph - Phi| 1.10e-16 (z = 6.72), largest |S phS - phi| 9.8e-17 (z = -0.703)."""
    x, _, w, out = answers(probe, "phi_table")
    phS, Ph = out
    g = w["grid"]
    sub = np.unique(np.round(np.linspace(g.start, g.stop - 1, 38000)).astype(np.int64))
    held = np.concatenate([sub, idx(w, "ties", "ends")])
    assert held.size <= 40000
    held = held[(x[held] >= 0) == bool(half)]
    z = x[held] / C.PHI_S  # (exact: S is a power of two)
    P, f = C.phi_ref(np.clip(z, -8.5, 8.5))
    eP, ef = C.mp_abs_err(Ph[held], P), C.mp_abs_err(C.PHI_S * phS[held], f)
    report("phiS_Phi_table, |Ph - Phi|", eP, z)
    report("phiS_Phi_table, |S phS - phi|", ef, z)
    assert eP.max() <= 2.5e-16 and ef.max() <= 3e-16
    assert np.isfinite(out[:, :w["nan"].start]).all()
    lo, hi = int(np.flatnonzero(x == -C.PHI_HALF)[0]), int(np.flatnonzero(x == C.PHI_HALF)[0])
    for o in out:
        for i in idx(w, "beyond"):
            assert bits(o[i]) == bits(o[lo if x[i] < 0 else hi]), x[i]
        assert bits(o[w["nan"]])[0] == bits(o[lo])


def test_log_phi_neg_table(probe):
    """error relative to max(1, |g|) at most 3e-16 against g = log Phi(-z) at 40 digits on the points of
    test_log_phi_table_of_the_lnr_kernel, every row tie with both neighbours, both clamps, and z < -8.5 down to -Inf.  The far
    branch (log_Phi_neg_far, which no other test executes): 2000 points of (38.5, 1e3] and z = 1e150 to relative 1e-11 (the header's
    claim), finite until z^2 overflows, -Inf at 1e300 and +Inf, never NaN.  At the seam the table at 38.5 and the far form at the next
    double differ by no more than the two bars together.  A NaN reads row 0: the bits of z = -8.5.
    Measured on an MI355X: table 2.04e-16 (z = 5.19), far branch 2.9e-14 relative (at the seam, 38.5 + 1 ulp)."""
    x, _, w, out = answers(probe, "log_phi_neg")
    got = out[0]
    held = idx(w, "table_test", "ties", "clamps", "below")
    g = C.log_phi_neg_ref(x[held])
    e = C.mp_abs_err(got[held], g) / np.maximum(1.0, np.abs([float(v) for v in g]))
    report("log_Phi_neg_table, relative to max(1, |g|)", e, x[held])
    assert e.max() <= 3e-16
    far = np.concatenate([idx(w, "far"), idx(w, "far_special")[:1]])
    assert x[far].min() > 38.5 and x[far].max() == 1e150 and np.isfinite(got[far]).all()
    gf = C.log_phi_neg_ref(x[far])
    ef = C.mp_abs_err(got[far], gf) / np.abs([C.to_float(v) for v in gf])
    report("log_Phi_neg_far, relative", ef, x[far])
    assert ef.max() <= 1e-11
    assert (got[w["far_special"]][1:] == -np.inf).all()  # z = 1e300 (z^2 overflows) and +Inf
    assert not np.isnan(got[:w["nan"].start]).any()
    a, b = int(np.flatnonzero(x == 38.5)[0]), w["far"].start
    assert x[b] == np.nextafter(38.5, np.inf)
    ga, gb = (float(v) for v in C.log_phi_neg_ref([x[a], x[b]]))
    print("seam: table(38.5) = %r, far(next) = %r" % (got[a], got[b]))
    assert abs(got[a] - got[b]) <= 3e-16 * abs(ga) + 1e-11 * abs(gb) + abs(ga - gb)
    assert bits(got[w["nan"]])[0] == bits(got[x == -8.5][0])


LBA_K = dict(lba2=1, lba3=1, lba_rt4=1)  # the largest observed error over the bound at K = 1, rounded up to a power of two


@pytest.mark.parametrize("part", [0, 1, 2])
@pytest.mark.parametrize("name", ["lba2", "lba3", "lba_rt4"])
def test_lba_trial(probe, name, part):
    """(every instance's rows in three parts, rows part, part + 3, ..., to keep each case short)  lba_trial<2>, <3> and <0> (four accumulators), one trial per lane, with the per-proposal values formed as lba_range_sum forms
    them, against the formulas of tests/golden/make_golden.py at 40 digits: 2e4 rows drawn like make_problem("lba") between the three
    instances, and tail rows (t in {1e-3, 5, 60}, A in {1e-3, 5}, negative drifts, arguments beyond +-8.5); the factor is exactly 0
    where rt - tau <= 1e-300 or rt is NaN.  The bar follows the conditioning and comes from the reference alone
    (device_math_cases.lba_check): with EPS_P = 2.5e-16 and EPS_PHI = 3e-16, the table's bars,
        E_a = EPS_P (sum |coefficients of Phi|) + 2 EPS_PHI (prefactor) + K 2^-53 M_a,
    M_a the sum of the magnitudes of the factor's terms with n^2 phi for the rounded arguments, and the product may be off by
    |ref| (sum_a E_a / |factor_a| + n_a EPS_P / (1 - p_neg)); compared after the 1e-10 floor.
    Measured on an MI355X: largest error over the bound at K = 1: 0.45 (<2>), 0.48 (<3>), 0.56 (<0>, four accumulators), so
    K = 1; largest absolute error 3.2e-15 on factors of order one."""
    x, y, w, out = answers(probe, name)
    rows = np.arange(part, x.size, 3)
    err, base, kpart, ref = (np.zeros(x.size) for _ in range(4))
    err[rows], base[rows], kpart[rows], ref[rows] = C.lba_check(out[0][rows], x[rows], y[:, rows], C.LBA_NA[name])
    dead = np.intersect1d(idx(w, "dead"), rows)
    assert dead.size >= 1 and (err[dead] == 0.0).all() and (out[0][dead] == 0.0).all()
    live = np.intersect1d(idx(w, "random", "tail"), rows)
    ratio = err[live] / (base[live] + kpart[live])
    i = int(np.argmax(ratio))
    print("%s: largest error / bound(K = 1) = %.4g at row %d (rt %r, y %r): error %.4g, reference %.6g" %
          (name, ratio[i], live[i], x[live[i]], list(y[:, live[i]]), err[live[i]], ref[live[i]]))
    print("%s: largest relative error above the floor %.4g" % (name, (err[live] / np.maximum(np.abs(ref[live]), 1e-10)).max()))
    K = LBA_K[name]
    assert K <= 16
    bad = np.flatnonzero(err[live] > base[live] + K * kpart[live])
    assert bad.size == 0, (name, live[bad[:5]], err[live[bad[:5]]])


def test_prior_term(probe):
    """prior_term for the kinds 1-4 and 6-9, the table entry formed by demc_prep.hpp's prior_entry (c from prior_const, b or 1/b as
    the kernels expect it), 200 points a kind: interior points, both ends of the support with their neighbours, +-1e-300, +-1e300;
    Beta(1/2, 1/2), Beta(1, 1), Gamma of shape 1/2 and 1 among the parameters.  Bar: 16 * 2^-53 times the sum of the magnitudes of the
    reference's terms (the roundings of a sum of at most four terms, a device log within 1 ulp, the host's lgamma within a few).
    Outside the support exactly -Inf.  Pinned as they are: Gamma at x = 0 is -Inf whatever the shape (the device's support test is
    x > 0); Beta at 0 (1) drops the term whose exponent a - 1 (b - 1) is 0 and is +-Inf otherwise; Exponential and half-Cauchy at
    x = 0 follow the closed form.
    Measured on an MI355X: largest error 2.57 x 2^-53 times the sum of magnitudes (Normal(-3, 10) at x = 37.5).
    Before log1p_sq (csrc/demc_kernels.hpp) the Cauchy and half-Cauchy arms returned -Inf at |x| = 1e300 -- z * z overflowed -- where the
    log-density is -1382.7 for Cauchy(0, 1): this test found it."""
    import mpmath
    x, y, _, out = answers(probe, "prior_term")
    got = out[0]
    assert x.size == len(C.PRIOR_KINDS) * C.PRIOR_PER_KIND
    worst, where, n_out, n_pin = 0.0, None, 0, 0
    bad = []
    for i in range(x.size):
        kind, a, b = int(y[0, i]), float(y[1, i]), float(y[2, i])
        val, mag = C.prior_ref(kind, a, b, float(x[i]))
        if val is None:  # Gamma at 0
            n_pin += 1
            ok = got[i] == -np.inf
        elif val == -np.inf or val == np.inf or not np.isfinite(C.to_float(val)):
            n_out += val == -np.inf
            ok = got[i] == C.to_float(val)
        else:
            e = float(abs(mpmath.mpf(float(got[i])) - val)) if np.isfinite(got[i]) else np.inf
            e = e / mag if mag > 0 else (0.0 if e == 0 else np.inf)  # (Uniform(0, 1): the one term is 0, and so is the answer)
            if e > worst:
                worst, where = e, (kind, a, b, float(x[i]), float(got[i]))
            ok = e <= 16 * U
        if not ok:
            bad.append((kind, a, b, float(x[i]), float(got[i]), None if val is None else C.to_float(val)))
    print("prior_term: largest error / sum of magnitudes = %.3g (%.2f x 2^-53) at (kind, a, b, x, got) = %r" % (worst, worst / U, where))
    print("prior_term: %d points outside the support, %d pinned at Gamma's x = 0" % (n_out, n_pin))
    assert n_out >= 90 and n_pin == 4
    assert not bad, bad[:10]


def test_box_muller(probe):
    """both outputs within 8 * 2^-53 * rad (one log, one sqrt, one sincospi and one product, each within 2 ulp) of
    rad (cos, sin)(2 pi u1), rad = sqrt(-2 log(1 - u0)): 1e5 random word pairs and every pair of {0, 1, 0x7FFFFFFF, 0x80000000,
    0xFFFFFFFF} against 80-bit arithmetic, 2e4 of them (the special pairs included) against 40 digits; never NaN or Inf.
    Measured on an MI355X: largest error 2.72 x 2^-53 rad."""
    x, y, w, out = answers(probe, "box_muller")
    assert np.isfinite(out).all()
    rx, ry, rad = C.box_muller_ref_ld(x, y[0])
    e = np.maximum(np.abs(out[0].astype(C.ld) - rx), np.abs(out[1].astype(C.ld) - ry)) / rad
    e = e.astype(np.float64)
    report("box_muller against 80 bits, in 2^-53 rad", e / U, list(zip(x, y[0])))
    assert e.max() <= 8 * U
    sub = np.concatenate([np.arange(20000 - 25), idx(w, "specials")])
    ref = C.box_muller_ref(x[sub], y[0][sub])
    em = np.array([float(max(abs(mpmath_f(out[0][i]) - r[0]), abs(mpmath_f(out[1][i]) - r[1])) / r[2]) for i, r in zip(sub, ref)])
    report("box_muller against 40 digits, in 2^-53 rad", em / U, list(zip(x[sub], y[0][sub])))
    assert em.max() <= 8 * U


def mpmath_f(v):
    import mpmath
    return mpmath.mpf(float(v))
