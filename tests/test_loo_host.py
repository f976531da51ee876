"""PSIS-LOO on the host: chains.loo_from_loglik held to the definition restated in mpmath at 40 digits
(tests/loo_cases.py), every edge rule checked exactly, the header of demc_loo held to the library and to both bindings, and the plan
program of csrc/demc_looplan.hpp (tests/looplan_host.cpp) run under the sanitizers and held to its Python restatement.  No GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import loo_cases as LC

ROOT = LC.ROOT
CSRC = LC.CSRC
inf, nan = float("inf"), float("nan")


# ---- the definition in mpmath ---------------------------------------------------------------------------------------------------------
def test_numpy_twin_against_the_definition_at_40_digits(demc):
    worst, tails = {}, {}
    for S, seed in ((21, 3), (26, 23), (130, 2), (2000, 2)):  # (seeds at which y = 50 keeps a floored tail long enough to be fitted)
        ll = LC.gaussian_terms(LC.Y_FLOOR, LC.gaussian_draws(np.random.default_rng(seed), S))
        got = demc.loo_from_loglik(ll).pointwise
        ref = LC.ref_table(ll)
        w = LC.check_table(got, ref, f"S={S}")
        tails[S] = got[:, 4].astype(int).tolist()
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst error in units of 1e-9 max(1, |ref|):", worst, "n_tail:", tails)
    assert all(v <= 1.0 for v in worst.values()), worst
    # the floor was active and a floored tail was still fitted (y = 50 beside ordinary points)
    assert 4 < tails[2000][4] < LC.tail_len(2000) and tails[2000][:4] == [135] * 4
    assert 4 < tails[130][4] < 26 and tails[26][4] == 5


def test_totals(demc):
    rng = np.random.default_rng(4)
    ll = LC.gaussian_terms(LC.Y_FLOOR, LC.gaussian_draws(rng, 130))
    r = demc.loo_from_loglik(ll)
    p = r.pointwise
    assert r.elpd_loo == pytest.approx(p[:, 0].sum(), rel=1e-14) and r.p_loo == pytest.approx(p[:, 1].sum(), rel=1e-14)
    assert r.lppd == pytest.approx(p[:, 3].sum(), rel=1e-14) and r.looic == -2 * r.elpd_loo
    assert r.se_elpd == pytest.approx(math.sqrt(5 * p[:, 0].var(ddof=1)), rel=1e-12)
    assert r.n_k_high == (p[:, 2] > 0.7).sum() and r.n_k_bad == (p[:, 2] > 1).sum() and r.n_nonfinite == 0
    assert demc.chains.LOO_TOTALS == ("elpd_loo", "se_elpd", "p_loo", "lppd", "looic", "n_k_high", "n_k_bad", "n_nonfinite")
    assert "khat > 0.7" in repr(r) or r.n_k_high == 0
    c = demc.compare_loo(r, r)
    assert c == dict(elpd_diff=0.0, se_diff=0.0)
    other = demc.loo_from_loglik(ll - 0.25)
    c = demc.compare_loo(r, other)
    assert c["elpd_diff"] == pytest.approx(1.25, rel=1e-9) and c["se_diff"] < 1e-6
    with pytest.raises(ValueError):
        demc.compare_loo(demc.chains.Loo(r.totals), r)


# ---- the edge rules, each exactly -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 20])
def test_short_windows_form_no_tail(demc, S):
    rng = np.random.default_rng(S)
    ll = LC.gaussian_terms(LC.Y_FLOOR[:4], LC.gaussian_draws(rng, S))
    p = demc.loo_from_loglik(ll).pointwise
    assert (p[:, 4] == 0).all() and np.isnan(p[:, 5]).all() and np.isposinf(p[:, 2]).all()
    ref = LC.ref_table(ll)
    assert all(v <= 1.0 for v in LC.check_table(p, ref, f"S={S}").values())
    if S == 1:  # one draw: the weight is 1, elpd_loo is the term itself
        assert np.array_equal(p[:, 0], ll[0]) and np.array_equal(p[:, 3], ll[0]) and (p[:, 1] == 0).all()


def test_S_21_is_the_first_window_with_a_tail(demc):
    assert LC.tail_len(20) == 4 and LC.tail_len(21) == 5
    l = -np.arange(1.0, 22.0)[:, None]  # 21 distinct terms: -1 ... -21
    p = demc.loo_from_loglik(l).pointwise
    assert p[0, 4] == 5 and p[0, 5] == -16.0 and math.isfinite(p[0, 2])  # the five smallest, cut at the sixth smallest
    assert all(v <= 1.0 for v in LC.check_table(p, LC.ref_table(l), "S=21").values())


def test_constant_column(demc):
    for S in (21, 130, 5000):
        p = demc.loo_from_loglik(np.full((S, 1), -1.25)).pointwise
        assert p[0].tolist()[:5] == [-1.25, 0.0, inf, -1.25, 0.0] and p[0, 5] == -1.25


def test_ties_at_the_cutoff_stay_outside(demc):
    S = 130
    M = LC.tail_len(S)
    l = -np.linspace(1.0, 2.0, S)
    ls = np.sort(l)
    l = np.where((l == ls[M - 1]) | (l == ls[M - 2]), ls[M], l)  # the M-th and (M-1)-th smallest now tie with the cutoff
    p = demc.loo_from_loglik(l[:, None]).pointwise
    assert p[0, 4] == M - 2 and p[0, 5] == ls[M]
    ref = LC.ref_table(l[:, None])
    assert ref[0, 4] == M - 2 and all(v <= 1.0 for v in LC.check_table(p, ref, "ties").values())
    # the M + 1 smallest terms tied: the cutoff is the minimum itself, x_cut = 0 and nothing lies above it
    l2 = np.where(l <= ls[M], ls[0], l)
    p2 = demc.loo_from_loglik(l2[:, None]).pointwise
    assert p2[0, 4] == 0 and p2[0, 2] == inf and p2[0, 5] == ls[0]
    assert all(v <= 1.0 for v in LC.check_table(p2, LC.ref_table(l2[:, None]), "ties at the minimum").values())


def test_floor_shrinks_the_tail(demc):
    rng = np.random.default_rng(2)
    th = LC.gaussian_draws(rng, 2000)
    ll = LC.gaussian_terms([50.0], th)
    p = demc.loo_from_loglik(ll).pointwise
    x = ll.min() - np.sort(ll[:, 0])
    assert p[0, 4] == (x > LC.LOG_MIN).sum() < 135 and x[135] < LC.LOG_MIN  # the floor, not the cutoff, bounds the tail
    assert LC.LOG_MIN == math.log(2.2250738585072014e-308) == demc.chains.LOO_LOG_MIN


def test_khat_zero_is_the_exponential_limit(demc):
    C = demc.chains
    n, sigma, exc = 40, 0.3, 0.01
    x0 = C.psis_smooth(0.0, sigma, n, exc)
    p = (np.arange(1, n + 1) - 0.5) / n
    want = np.minimum(np.log(-sigma * np.log1p(-p) + exc), 0.0)
    assert np.array_equal(x0, want) and np.isfinite(x0).all()
    near = C.psis_smooth(1e-9, sigma, n, exc)
    assert np.abs(near - x0).max() < 1e-7


def test_non_finite_draws(demc):
    rng = np.random.default_rng(12)
    ll = LC.gaussian_terms(LC.Y_FLOOR[:3], LC.gaussian_draws(rng, 130))
    lppd = demc.waic_from_loglik(ll).pointwise[:, 0]
    a = ll.copy()
    a[7, 1] = -inf
    r = demc.loo_from_loglik(a)
    p = r.pointwise
    assert p[1, 0] == -inf and p[1, 1] == inf and p[1, 2] == inf and math.isfinite(p[1, 3]) and p[1, 4] == 0 and p[1, 5] == -inf
    assert np.isfinite(p[[0, 2]]).all() and r.n_nonfinite == 1 and r.elpd_loo == -inf and r.n_k_high >= 1 and r.n_k_bad >= 1
    assert np.array_equal(p[[0, 2], 3], lppd[[0, 2]])
    a[:, 1] = -inf  # every draw: lppd is -Inf too and p_loo = -Inf - -Inf
    p = demc.loo_from_loglik(a).pointwise
    assert p[1, 0] == -inf and p[1, 3] == -inf and math.isnan(p[1, 1])
    for bad in (nan, inf):  # +Inf is treated as NaN
        b = ll.copy()
        b[9, 2] = bad
        r = demc.loo_from_loglik(b)
        assert np.isnan(r.pointwise[2]).all() and np.isfinite(r.pointwise[:2]).all() and r.n_nonfinite == 1 and math.isnan(r.elpd_loo)
        assert r.n_k_high == (r.pointwise[:2, 2] > 0.7).sum()
    ref = LC.ref_table(np.where(np.arange(130)[:, None] == 7, np.array([0.0, -inf, 0.0])[None, :] + ll, ll))
    assert ref[1, 0] == -inf and ref[1, 5] == -inf and ref[1, 4] == 0


def test_one_observation(demc):
    rng = np.random.default_rng(13)
    ll = LC.gaussian_terms([1.3], LC.gaussian_draws(rng, 130))
    r = demc.loo_from_loglik(ll)
    assert math.isnan(r.se_elpd) and r.elpd_loo == r.pointwise[0, 0] and r.pointwise.shape == (1, 6)
    with pytest.raises(ValueError):
        demc.loo_from_loglik(np.empty((0, 3)))


# ---- summarize(..., loo=True) without a device ----------------------------------------------------------------------------------------
def _tiny_model(demc):
    sp = lambda: [0.1, 1.0]  # noqa: E731
    model = demc.DEModel(sample_prior=sp, prior_loglike=demc.Priors(μ=demc.Normal(0, 10), σ=demc.TruncatedCauchy(0, 1)),
                         loglike=demc.GaussianLikelihood(), data=np.arange(5.0), names=("μ", "σ"))
    return model, demc.DE(sample_prior=sp, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=2, Np=4)


def test_summarize_refuses_an_engine_without_loo(demc):
    class Bare:
        def __init__(self, **cfg):
            self.closed = False

        def close(self):
            self.closed = True

    made = []

    def factory(**cfg):
        made.append(Bare(**cfg))
        return made[-1]

    model, de = _tiny_model(demc)
    with pytest.raises(demc.DemcError) as e:
        demc.summarize(model, de, 4, loo=True, engine_factory=factory)
    assert e.value.code == demc._ffi.EUNSUPPORTED and "demc_loo" in str(e.value)
    assert len(made) == 1 and made[0].closed


def test_summarize_asks_before_the_run_what_loo_is_certain_to_refuse(demc):
    log = []

    class Refusing:
        def __init__(self, **cfg):
            pass

        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return lambda *a, **k: log.append(name)

        def loo_served(self):
            log.append("loo_served")
            raise demc.DemcError(demc._ffi.EUNSUPPORTED, "demc_loo: the MvNormal families answer per observation only with loglike_mode = direct")

    model, de = _tiny_model(demc)
    with pytest.raises(demc.DemcError) as e:
        demc.summarize(model, de, 4, loo=True, engine_factory=Refusing)
    assert e.value.code == demc._ffi.EUNSUPPORTED and "demc_loo" in str(e.value)
    assert "set_model" in log and log.index("set_model") < log.index("loo_served") and "step" not in log and log[-1] == "close"


def test_loo_served_restates_the_refusals_of_the_call(demc):
    F = demc.families

    def handle(family, mode=0, n_obs=10, shards=1):
        e = demc.HipEngine.__new__(demc.HipEngine)
        e.cfg = demc._ffi.make_config(n_groups=2, Np=4, D=2, loglike_mode=mode, n_groups_total=2 * shards)
        e.family, e.n_obs, e.h = family, n_obs, None
        return e

    for fam in (F.FAM_GAUSSIAN, F.FAM_BINOMIAL, F.FAM_LNR, F.FAM_LBA):
        for mode in (0, 1, 2):
            handle(fam, mode).loo_served()
    handle(F.FAM_MVN_ISO, 2).loo_served()
    U, E = demc._ffi.EUNSUPPORTED, demc._ffi.EINVAL
    for e, code, word in [(handle(F.FAM_MVN_FULL, 0), U, "loglike_mode = direct"), (handle(F.FAM_HIER_GAUSSIAN), U, "no per-observation"),
                          (handle(F.FAM_LBA, n_obs=0), E, "no observations"), (handle(F.FAM_GAUSSIAN, shards=2), E, "sharded handle")]:
        with pytest.raises(demc.DemcError) as err:
            e.loo_served()
        assert err.value.code == code and word in str(err.value) and "demc_loo: " in str(err.value)


# ---- the plan program -------------------------------------------------------------------------------------------------------------------
def test_plans_under_the_sanitizers():
    run = subprocess.run([LC.program()], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "looplan ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr[-4000:]


def _request(family, N, S, direct=False, n_acc=0, d=0, dp=0):
    from test_pwplan_host import FAMILY
    return f"P {FAMILY[family]} {int(direct)} {N} {n_acc} {d} {dp} {S}"


def test_python_restatement_is_the_plan(demc):
    c = LC.plans(["const"])[0]
    assert (c["kLooObs"], c["kLooTile"], c["kLooTargetWG"], c["kLooWG"], c["kLooCap"], c["kLooMaxTail"], c["kLooMaxDraws"], c["kLooMaxCells"]) == \
        (LC.LOO_OBS, LC.LOO_TILE, LC.LOO_TARGET_WG, LC.LOO_WG, LC.LOO_CAP, LC.LOO_MAX_TAIL, LC.LOO_MAX_DRAWS, LC.LOO_MAX_CELLS)
    assert (c["DEMC_LOO_NTOTAL"], c["DEMC_LOO_NPOINT"]) == (demc._ffi.LOO_NTOTAL, demc._ffi.LOO_NPOINT) == (len(demc.chains.LOO_TOTALS), len(demc.chains.LOO_POINT)) == (8, 6)
    assert demc._ffi.LOO_MAX_DRAWS == LC.LOO_MAX_DRAWS and c["kLooLdsBytes"] <= 160 * 1024
    shapes = sorted({(N, S) for N in (1, 5, 63, 64, 65, 257, 2048, 2049, 50000, 100000) for S in (1, 3, 20, 21, 26, 130, 2000, 65536, 65537, 409600, 1 << 22)})
    for (N, S), p in zip(shapes, LC.plans([_request("lba", N, S, n_acc=3) for N, S in shapes])):
        g = LC.plan(N, S)
        assert p["refused"] == 0 and (g["M"], g["Nb"], g["blocks"], g["tiles"], g["chunks"], g["chunk_len"]) == \
            (p["M"], p["Nb"], p["blocks"], p["tiles"], p["chunks"], p["chunk_len"]), (N, S, g, p)
        assert g["M"] == demc.chains.loo_tail_len(S) * (S > 20) and g["cuts"][0][0] == 0 and g["cuts"][-1][1] == N
        assert p["n_terms"] == g["Nb"] * S and p["n_point"] == 6 * N and p["n_total"] == 8 and p["n_cst"] == 13 * S
    # the refusals reach the caller through the plan, with their texts; the cap on the draws is tested here, not with a 4M-draw history
    refused = LC.plans([_request("gaussian", 10, (1 << 22) + 1), _request("mvn_full", 65, 70, d=8), _request("hier_gaussian", 65, 70), _request("sim", 10, 5),
                        _request("lba", 0, 12, n_acc=3), _request("gaussian", 10, 0)])
    assert [r["refused"] for r in refused] == [1, 5, 5, 5, 1, 1]
    assert refused[0]["message"] == ("demc_loo: S = 4194305 draws are above the cap of 4194304 (DEMC_LOO_MAX_DRAWS: the tail of an observation is sorted in LDS); "
                                     "pass a narrower window")
    assert refused[1]["message"].startswith("demc_loo: the MvNormal families") and "loglike_mode = direct" in refused[1]["message"]
    assert refused[2]["message"] == "demc_loo: DEMC_FAM_HIER_GAUSSIAN has no per-observation log-density on the device"
    assert "simulation likelihood" in refused[3]["message"] and refused[4]["message"] == "demc_loo: the model holds no observations (N < 1)"
    assert refused[5]["message"] == "demc_loo: no draws (S < 1)"
    assert LC.plans([_request("gaussian", 10, 1 << 22)])[0]["refused"] == 0


def test_plan_is_written_in_the_host_only_header():
    header = open(os.path.join(CSRC, "demc_looplan.hpp")).read()
    for word in ("hip/", "hipStream", "ALLOC", "demc_handle", "getenv"):
        assert word not in header, word
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".hpp"))}
    texts = re.findall(r'"((?:[^"\\]|\\.)*)"', re.sub(r"//.*", "", header))
    refusals = [t for t in texts if len(t) >= 28 and " " in t]
    assert len(refusals) >= 5, refusals
    for t in refusals:
        for name, text in sources.items():
            if name != "demc_looplan.hpp":
                assert '"' + t + '"' not in text, (name, t)
    assert sources["demc_hip.cpp"].count("plan_loo(") == 1
    assert sum(text.count("plan_loo(") for name, text in sources.items() if name not in ("demc_hip.cpp", "demc_looplan.hpp")) == 0
    unit = sources["demc_loo.cpp"]
    assert unit.count("finish(who, st,") == 1 and "hipStreamSynchronize" not in unit
    for word in ("atomicAdd(double", "unsafeAtomicAdd", "atomicAdd_system"):  # integer LDS atomics only
        assert word not in unit
    # the text of a term exists once: both units take it from demc_pwterm.hpp
    assert "pw_term(" in sources["demc_pwterm.hpp"].replace("pw_term<F, X>(", "pw_term(") or "pw_term(const PwKParams" in sources["demc_pwterm.hpp"]
    for name in ("demc_pointwise.cpp", "demc_loo.cpp"):
        assert '#include "demc_pwterm.hpp"' in sources[name] and "lba_trial<" not in sources[name] and "log_Phi_neg_table(" not in sources[name]
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "demc_loo.cpp" in makefile and "$(OBJ).loo.o" in makefile


# ---- the header, the library and both bindings ------------------------------------------------------------------------------------------
def _loo_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demc_loo.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return text, protos


def test_header_library_and_python_binding_agree(demc):
    import ctypes as C
    text, protos = _loo_prototypes()
    assert sorted(protos) == sorted(demc._ffi.LOO_EXPORTS) == ["demc_loo"]
    for other in (demc._ffi.EXPORTS, demc._ffi.SUMMARY_EXPORTS, demc._ffi.QUANTILE_EXPORTS, demc._ffi.COV_EXPORTS, demc._ffi.PW_EXPORTS):
        assert not set(protos) & set(other), "declared in another header as well"
    for h in ("demc.h", "demc_summary.h", "demc_quantile.h", "demc_cov.h", "demc_pointwise.h"):
        assert "demc_loo" not in open(os.path.join(ROOT, "include", h)).read(), h
    lib = demc._ffi.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "demc_handle*": C.c_void_p}
    ret, args = protos["demc_loo"]
    fn = lib.demc_loo
    assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args] and len(args) == 5
    assert "#define DEMC_LOO_NTOTAL 8" in text and "#define DEMC_LOO_NPOINT 6" in text and "#define DEMC_LOO_MAX_DRAWS 4194304" in text
    assert '#include "demc.h"' in text and "demc_pointwise.h" not in text
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "demc_loo.h")])
    assert callable(getattr(demc._ffi.HipEngine, "loo")) and callable(getattr(demc._ffi.HipEngine, "loo_served"))


def test_julia_ccall_matches_the_prototype(demc):
    import test_julia_shim as J
    _, protos = _loo_prototypes()
    main_jl = open(os.path.join(ROOT, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPLoo.jl")' in main_jl and "demc_loo" not in main_jl
    jl = open(os.path.join(ROOT, "julia", "DEMCHIPLoo.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= {"demc_loo"}
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
    names = re.search(r"const LOO_TOTALS = \(([^)]*)\)", jl).group(1)
    assert tuple(n.strip().lstrip(":") for n in names.split(",")) == demc.chains.LOO_TOTALS


def test_loo_kernels_use_no_scratch(tmp_path, demc):
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_loo_" in k[0]]
    assert len(ks) == 3 + 14, [k[0] for k in ks]  # prepare, column, totals; terms for each of the 14 instances
    assert sum("k_loo_terms" in k[0] for k in ks) == 14
    for name, regs, _, wg, scratch in ks:
        assert scratch == 0 and regs <= 512 // -(-wg // 256), (name, regs, wg, scratch)


# ---- the select's path restated, and the twin on tied, crowded and constant columns ----------------------------------------------------
@pytest.mark.parametrize("name", list(LC.HOST_FAMILIES))
def test_select_path_restatements_agree(name):
    """select_path (the kernel's walk) against select_path_direct (the closed form) on every column family, with what each outcome
    means: early -> M < nc <= 8192; unresolved after a counted digit -> nc <= M and more than 8192 keys up to the cutoff; no digit
    counted at all -> a constant column (LC.select_paths asserts all three)"""
    y, th = LC.HOST_FAMILIES[name]()
    assert y.shape == (LC.N_FAMILY,) and th.shape[1] == 2
    paths = LC.select_paths(LC.gaussian_terms(y, th))
    print(name, "S =", th.shape[0], "stop digits:", LC.reach(paths), "nc > 4096:", sum(p["nc"] > 4096 for p in paths),
          "nc == 0:", sum(p["nc"] == 0 for p in paths), "skipped:", sorted({p["skipped"] for p in paths}))


def test_select_path_on_hand_made_keys():
    """the two forms on columns whose path is known by construction"""
    M = LC.tail_len(9216)
    col = np.full(9216, -1.0)
    col[:100] = -np.linspace(2.0, 3.0, 100)  # 100 < M distinct terms under 9116 equal ones: unresolved, the 100 compacted
    for f in (LC.select_path, LC.select_path_direct):
        p = f(col, M)
        assert not p["early"] and p["nc"] == 100 and p["stop_digit"] is None, p
    col[:100] = np.nextafter(-1.0, -2.0)  # one ulp under the crowd: only the nine-bit last digit differs
    for f in (LC.select_path, LC.select_path_direct):
        assert f(col, M) == dict(early=False, stop_digit=None, counted=1, skipped=5, nc=100)
    col[:1000] = np.nextafter(-1.0, -2.0)  # the cutoff now lies among the 1000: they fit, stop at the last digit
    for f in (LC.select_path, LC.select_path_direct):
        assert f(col, M) == dict(early=True, stop_digit=5, counted=1, skipped=5, nc=1000)
    col = np.concatenate([np.linspace(-3.0, -2.0, 5000), np.linspace(0.5, 1.0, 4216)])  # both signs: the first digit separates them
    for f in (LC.select_path, LC.select_path_direct):
        assert f(col, M) == dict(early=True, stop_digit=0, counted=1, skipped=0, nc=5000)


SMALL_TIES = {  # scaled-down copies: the twin has no 8192-key cap, so the proportions matter and the sizes do not
    "crowd k=12": lambda: LC.crowd(12, S=520, copies=160), "crowd k=51": lambda: LC.crowd(51, S=520, copies=160),
    "one draw 850 of 1000": lambda: LC.one_draw(S=1000, copies=850), "every draw four times": lambda: LC.four_times(S=520),
    "two values": LC.two_values, "constant S=130": lambda: LC.constant(130), "constant S=26": lambda: LC.constant(26),
}
SMALL_COLS = [0, 1, 2, 3, 4, 5]  # y = 50 first


@pytest.mark.parametrize("name", list(SMALL_TIES))
def test_numpy_twin_on_ties_against_the_definition_at_40_digits(demc, name):
    y, th = SMALL_TIES[name]()
    S = th.shape[0]
    assert S <= 2000
    ll = LC.gaussian_terms(y[SMALL_COLS], th)
    got = demc.loo_from_loglik(ll).pointwise
    ref = LC.ref_table(ll)
    worst = LC.check_table(got, ref, name)  # n_tail and l_cut exactly
    print(name, "S =", S, "worst error in units of 1e-9 max(1, |ref|):", worst, "n_tail:", ref[:, 4].astype(int).tolist())
    assert all(v <= 1.0 for v in worst.values()), worst
    M = LC.tail_len(S)
    assert len(np.unique(th, axis=0)) < S, "no repeated draw"
    if name.startswith("crowd"):
        assert S - 3 * 160 < M and (ref[:, 4] < M).all()  # the cutoff falls in the crowd
    elif name.startswith("one draw"):
        assert S - 850 > M and (ref[:, 4] < M).any() and (ref[:, 4] == M).any()  # ... in some columns, among the distinct draws in others
    elif name.startswith("every draw"):
        assert M % 4 and (ref[1:, 4] == M - M % 4).all() and ref[0, 4] < M - M % 4  # inside a run; y = 50: the floor besides
    elif name == "two values":
        assert (ref[:, 4] == 0).all() and np.isposinf(ref[:, 2]).all() and np.array_equal(ref[:, 5], ll.min(axis=0))
    else:
        assert np.array_equal(got[:, 0], ll[0]) and np.array_equal(got[:, 3], ll[0]) and np.array_equal(got[:, 5], ll[0])
        assert (got[:, 1] == 0).all() and (got[:, 4] == 0).all() and np.isposinf(got[:, 2]).all()


def test_narrow_columns_keep_a_fit(demc):
    """the reference alone: every quartile excess of the narrow family is at least 2^-40, so one ulp of exp cannot switch a fit off"""
    y, th = LC.narrow()
    ll = LC.gaussian_terms(y, th)
    eq = LC.quartile_excess(ll)
    assert np.isfinite(eq).all() and eq.min() >= 2.0 ** -40, eq.min()
    assert np.isfinite(demc.loo_from_loglik(ll).pointwise[:, 2]).all()
