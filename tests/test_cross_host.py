"""tests/cross_cases.py on the CPU: the cases reach every branch the kernels' control flow has, the drawn integers have no accidental
symmetry that would hide a layout error, the references are right, and the request / result files round trip.  The probe itself
(tests/cross_probe.hip) needs an MI355X: tests/test_gpu_cross.py."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import cross_cases as C


@pytest.fixture(scope="module")
def cases():
    return C.all_cases()


def int_cases(cases):
    return [c for c in cases.values() if not c["real"]]


def test_every_branch_is_covered(cases):
    """the restated control flow (mt_ladder, asm_trips, chunk_tiles) over all cases reaches every branch; a missing one is named"""
    hc = C.header_constants()
    assert hc["instances"] == [(1, 4), (2, 4), (4, 4), (8, 4), (16, 4)], "DEMC_CROSS_INSTANCES moved: " + repr(hc["instances"])
    assert int(re.search(r"kMaxDynLds = (\d+) \* 1024", open(os.path.join(C.CSRC, "demc_constants.hpp")).read()).group(1)) * 1024 == C.MAX_LDS
    seen = set()
    for c in cases.values():
        if c["kind"] == C.KIND_CROSS:
            n_prop = c["n_groups"] * c["n_act"]
            seen.add("k_cross_mfma<%d,4> dpad %d" % (c["KS"], c["dpad"]))
            for n in C.chunk_tiles(c["n_tiles"], c["n_chunks"]):
                seen.add("k_cross_mfma<%d,4> chunk: %s" % (c["KS"], "empty" if n == 0 else "odd" if n & 1 else "even"))
            seen.add("k_cross_mfma<%d,4> last fragment: %d rows" % (c["KS"], (n_prop - 1) % 16 + 1))
            seen.add("k_cross_mfma<%d,4> particle tiles: %d" % (c["KS"], (n_prop + 255) // 256))
            seen.add("k_cross_mfma<%d,4> glist: %s" % (c["KS"], "yes" if c["glist"] else "null"))
            continue
        fn = C.FN_NAME[c["fn"]]
        calls = C.mt_ladder(c["KS"], c["n_act"], hc)
        seen.add("%s KS %d ladder %s" % (fn, c["KS"], C.ladder_name(calls)))
        for n in c["counts"]:
            for mt, _ in calls:
                if C.takes_asm_loop(c["fn"], c["KS"], mt, hc):
                    seen.add("asm loop MT %d after %s: %s" % (mt, "MT 4" if len(calls) > 1 else "nothing",
                                                              "skipped" if n == 0 else "nq %d np %d two %d" % C.asm_trips(n, hc)))
                else:
                    seen.add("%s KS %d builtin loop: %d tiles" % (fn, c["KS"], n))
        seen.add("%s zero tile: %s" % (fn, "n_tiles - xt_lo" if c["xt_lo"] else "appended"))
    want = set()
    for KS, dpad in [(1, 4), (2, 8), (4, 16), (8, 32), (16, 64), (16, 128)]:
        want.add("k_cross_mfma<%d,4> dpad %d" % (KS, dpad))
        want |= {"k_cross_mfma<%d,4> chunk: %s" % (KS, k) for k in ("empty", "odd", "even")}
        want |= {"k_cross_mfma<%d,4> last fragment: %d rows" % (KS, r) for r in (1, 12)}
        want |= {"k_cross_mfma<%d,4> particle tiles: %d" % (KS, n) for n in (1, 2)}
        want |= {"k_cross_mfma<%d,4> glist: %s" % (KS, g) for g in ("yes", "null")}
    for fn in ("cross_stage<lds_cptr>", "cross_stage<glb_cptr>"):
        for KS in (1, 2, 4, 8):
            want |= {"%s KS %d ladder %s" % (fn, KS, k) for k in ("1", "2", "3p", "4", "4+2", "4+3p", "4+4+1")}
            want |= {"%s KS %d builtin loop: %d tiles" % (fn, KS, n) for n in ((0, 1, 2, 3) if KS >= 8 else (0, 1, 2, 3, 4, 5))}
        want |= {"%s KS 16 ladder %s" % (fn, k) for k in ("1", "2", "2+1")}
        want |= {"%s KS 16 builtin loop: %d tiles" % (fn, n) for n in (0, 1, 2, 3)}
    want |= {"cross_ks<2,lds_cptr,true> KS 2 ladder %s" % k for k in ("1", "2", "3p", "4", "4+2", "4+3p", "4+4+1")}
    want |= {"cross_ks<8,lds_cptr,true> KS 8 ladder %s" % k for k in ("1", "2", "3p", "4", "4+2", "4+3p", "4+4+1")}
    for after in ("nothing", "MT 4"):  # (n_act = 32: MT = 2 alone; n_act = 96: behind an MT = 4 pass of the builtin loop)
        want.add("asm loop MT 2 after %s: skipped" % after)
        want |= {"asm loop MT 2 after %s: nq %d np %d two %d" % ((after,) + C.asm_trips(n, hc)) for n in range(1, 14)}
    trips = [C.asm_trips(n, hc) for n in range(1, 14)]  # n = 1 .. 13 is enough only while the trips are of four and two tiles
    for k, (what, vals) in enumerate([("nq", (0, 1, 2, 3)), ("np", (0, 1)), ("two", (0, 1))]):
        assert {t[k] for t in trips} == set(vals), "asm loop: n = 1 .. 13 gives %s in %r" % (what, sorted({t[k] for t in trips}))
    want |= {"cross_stage<lds_cptr> zero tile: appended", "cross_stage<glb_cptr> zero tile: n_tiles - xt_lo"}
    missing = sorted(want - seen)
    assert not missing, "no case reaches: " + "; ".join(missing)
    for c in cases.values():  # every wave's range starts past tile 0, and a launch stays inside the LDS the project asks for
        if c["kind"] == C.KIND_STAGE:
            assert min(c["t_lo"][:c["wg"] // 64]) >= 1 and C.lds_bytes(c) <= C.MAX_LDS


def test_asm_trips_restates_the_loop():
    """n = 4 nq + 2 np + 1 + two with np, two in {0, 1}: the trips consume every tile once"""
    for n in range(1, 200):
        nq, np_, two = C.asm_trips(n)
        assert nq >= 0 and np_ in (0, 1) and two in (0, 1) and 4 * nq + 2 * np_ + 1 + two == n


def test_the_sums_are_exact_in_any_order(cases):
    """integers of [-1023, 1023]: max sum |y x| < 2^53 in every case, so no order of summation rounds"""
    worst = 0.0
    for c in int_cases(cases):
        Yq = C.y_rows(c)
        assert (Yq == np.round(Yq)).all() and np.abs(Yq).max() <= 1023
        worst = max(worst, C.magnitude(c).max())
        assert C.magnitude(c).max() < 2.0 ** 53, c["name"]
    print("largest sum |y x| over the integer cases: 2^%.1f" % np.log2(worst))


def changed_everywhere(c, ref, other):
    return [u for u in C.units(c) if (ref[u[0], u[1]:u[2]] == other[u[0], u[1]:u[2]]).all()]


def test_layout_errors_change_every_reference(cases):
    """no accidental symmetry in the drawn integers: in every case, for every (plane, 16-row fragment) with at least one tile,
    exchanging any two k lanes of A changes the exact reference, so does k-step 1 read as k-step 0, and the fragment's rows are
    pairwise different (exchanging two result rows changes it)"""
    for c in int_cases(cases):
        ref = C.reference_int(c)
        for j1 in range(4):
            for j2 in range(j1 + 1, 4):
                same = changed_everywhere(c, ref, C.reference_int(c, Y=C.swap_k_lanes(c, j1, j2)))
                assert not same, (c["name"], "k lanes", j1, j2, same[:3])
        if c["KS"] >= 2:
            same = changed_everywhere(c, ref, C.reference_int(c, Xo=C.kstep1_from_kstep0(c)))
            assert not same, (c["name"], "k-step 1 from k-step 0", same[:3])
        for i, q0, q1 in C.units(c):
            rows = np.delete(ref[i, q0:q1], c["nan_q"] - q0) if c["nan_q"] is not None and q0 <= c["nan_q"] < q1 else ref[i, q0:q1]
            assert np.unique(rows).size == rows.size, (c["name"], "two equal rows", i, q0)


def exact_dot(c, plane, q):
    r0, r1, c0, c1, _ = C.planes(c)[plane]
    y = [Fraction(float(v)) for v in C.y_rows(c)[q, c0:c1]]
    return sum((yk * Fraction(float(x)) for row in c["Xo"][r0:r1, c0:c1] for yk, x in zip(y, row)), Fraction(0))


def test_references_against_exact_rationals(cases):
    """on a sample of outputs: the int64 reference IS the fractions.Fraction dot product, and the longdouble reference of the
    real-valued companions agrees with it to 1e-18 of sum |y x|"""
    rng = np.random.default_rng(7)
    for name in ("cross_ks1_d4_N17_seventeen", "cross_ks16_d100_N1030_main", "cross_ks8_d32_N33_main", "stage_glb_d16_n130", "asm_n96_b",
                 "stage_lds_d64_n48"):
        c = cases[name]
        ref = C.reference_int(c)
        for _ in range(6):
            i, q = int(rng.integers(ref.shape[0])), int(rng.integers(ref.shape[1]))
            assert Fraction(int(ref[i, q])) == exact_dot(c, i, q), (name, i, q)
    worst = 0.0
    for name in ("real_k_cross_mfma<16,4>_two_pass", "real_k_cross_mfma<1,4>", "real_cross_stage<glb_cptr>_d64", "real_cross_ks<2,lds_cptr,true>"):
        c = cases[name]
        ref, mag = C.reference_ld(c), C.magnitude(c)
        for _ in range(4):
            i, q = int(rng.integers(ref.shape[0])), int(rng.integers(ref.shape[1]))
            if mag[i, q] == 0:
                continue
            ex = exact_dot(c, i, q)
            hi = float(ex)  # the longdouble nearest the rational, in two pieces
            e = abs((C.ld(hi) - ref[i, q]) + C.ld(float(ex - Fraction(hi)))) / C.ld(mag[i, q])
            worst = max(worst, float(e))
            assert e <= 1e-18, (name, i, q, float(e))
    print("longdouble reference against the rationals: largest error %.3g of sum |y x|" % worst)


def test_fragment_order_is_the_formula_of_demc_prep():
    """Xf[tile][kstep][lane] = X[16 tile + (lane & 15)][4 kstep + (lane >> 4)] (tests/prep_host.cpp pins demc_prep.hpp to the same)"""
    X = np.arange(48 * 12, dtype=np.float64).reshape(48, 12)
    Xf = C.fragments(X, 12)
    for t in range(3):
        for ks in range(3):
            for lane in range(64):
                assert Xf[t, ks, lane] == X[16 * t + (lane & 15), 4 * ks + (lane >> 4)]


def test_files_round_trip_and_the_stand_in_meets_the_references(cases, tmp_path):
    """request -> stand-in -> result: the files carry the headers and the operands unchanged, and a correct answer formed from the
    fragment-ordered request passes the checks the device answer is held to"""
    import test_gpu_cross as G
    names = ["cross_ks2_d8_N33_main", "cross_ks16_d100_N17_one", "cross_ks4_d16_isolation", "stage_glb_d8_n100", "stage_lds_d64_n48", "asm_n32_a",
             "real_cross_ks<8,lds_cptr,true>"]
    sub = [cases[n] for n in names]
    req, res = str(tmp_path / "request.bin"), str(tmp_path / "result.bin")
    C.write_request(req, sub)
    back = C.read_request(req)
    assert len(back) == len(sub)
    for c, (h, Y, X) in zip(sub, back):
        hh, Xf = C.header(c)
        assert h == hh and h[1] == c["Y"].size and h[3] == C.n_out(c)
        assert (Y.view(np.uint64) == c["Y"].ravel().view(np.uint64)).all() and (X.view(np.uint64) == Xf.ravel().view(np.uint64)).all()
    C.write_result(res, [(c["kind"], C.stand_in(c)) for c in sub])
    state = dict(cases=dict(zip(names, sub)), out={}, error=None)
    assert G.load_answers(state, res) is None
    for n in names[:-1]:
        G.check_exact(*G.answers(state, n))
    G.test_real_valued_companion(state, names[-1])
    # a stored entry that should have rested, and a wrong sum, are both seen
    bad = state["out"]["stage_lds_d64_n48"].copy()
    bad[cases["stage_lds_d64_n48"]["n_act"]] = 0.0
    with pytest.raises(AssertionError):
        G.check_exact(cases["stage_lds_d64_n48"], bad)
    bad = state["out"]["asm_n32_a"].copy()
    bad[C.out_index(cases["asm_n32_a"])[3, 5]] += 1.0
    with pytest.raises(AssertionError):
        G.check_exact(cases["asm_n32_a"], bad)
    C.write_result(res, [(c["kind"], C.stand_in(c)) for c in sub[:-1]])
    assert G.load_answers(dict(cases=dict(zip(names, sub)), out={}), res) is not None
