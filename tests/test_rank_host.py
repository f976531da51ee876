"""Rank-normalised chain diagnostics (demc_rankstats / demc_rank_series on the device, Chains.rankstats on the host)
against an independent restatement of the definition in plain loops -- Python's sorted() on integer keys, counting for L and E,
then the plain-loop restatements of test_summary_host.py and test_quantile_host.py for the rest; nothing below is shared with
chains.py --, the inverse normal against mpmath at 40 digits, the plan program of csrc/demc_rankplan.hpp (tests/rankplan_host.cpp)
under the sanitizers and held to its Python restatement, the header against the library and both bindings, and the inputs the GPU
tests of the same feature import (tests/test_gpu_rank.py).  No GPU here."""
import atexit
import functools
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import test_quantile_host as Q
import test_summary_host as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
NAN = float("nan")
COLS = ("rhat", "ess_bulk", "ess_tail", "rhat_bulk", "rhat_folded", "ess_q05", "ess_q95", "distinct")
PROBS = (0.5, 0.05, 0.95)
# The largest relative error of ppnd16 against mpmath at 40 digits over the arguments of test_inverse_normal_against_mpmath, as
# that test measured and printed it (5.72e-16, also in DESIGN.md 5.11), rounded up.  The bar of every comparison of normal scores is four times
# this: the device's log and sqrt may differ from the host's by an ulp.
PPND_MEASURED = 5.8e-16
PPND_BAR = 4 * PPND_MEASURED


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def restate_ranks(values):
    """steps 1 and 2 for one pool -> ([r_i], distinct, has_nan): integer keys, sorted, L and E by counting"""
    ks = [Q.key(float(v)) for v in values]
    count = {}
    for k in ks:
        count[k] = count.get(k, 0) + 1
    below, seen = {}, 0
    for k in sorted(count):
        below[k] = seen
        seen += count[k]
    order = sorted(ks)
    return [below[k] + (count[k] + 1) / 2 for k in ks], len(count), order[0] < Q.KEY_NEG_INF or order[-1] > Q.KEY_POS_INF


def _ndtri(p):  # the second witness: scipy's inverse normal, another algorithm
    from scipy.special import ndtri
    return float(ndtri(p))


def restate_scores(ranks, N):
    return [_ndtri((r - 0.375) / (N + 0.25)) for r in ranks]


def restate(x, max_lag=0):
    """DESIGN.md 5.11 for one series x[n][m], one step after the other -> dict over COLS, with pmin = the smallest |P_k| over the
    Geyer pairs of the four derived series (None if there were none) and the derived series themselves"""
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    N = n * m
    flat = [float(v) for v in x.reshape(-1)]
    ranks, distinct, has_nan = restate_ranks(flat)
    out = dict.fromkeys(COLS, NAN)
    out["pmin"], out["ranks"] = None, np.array(ranks).reshape(n, m)
    if has_nan:
        return out
    out["distinct"] = float(distinct)
    z = np.array(restate_scores(ranks, N)).reshape(n, m)
    med, q05, q95 = Q.restate(flat, PROBS)
    with np.errstate(all="ignore"):
        zeta = [abs(float(np.float64(v) - np.float64(med))) for v in flat]
    ranks2, _, nan2 = restate_ranks(zeta)
    z2 = np.array(restate_scores(ranks2, N)).reshape(n, m)
    i05 = np.array([1.0 if v <= q05 else 0.0 for v in flat]).reshape(n, m)
    i95 = np.array([1.0 if v <= q95 else 0.0 for v in flat]).reshape(n, m)
    rs = [R.restate(s, max_lag) for s in (z, i05, i95, z2)]
    pm = [r["pmin"] for r in rs[:3] + ([] if nan2 else rs[3:]) if r["pmin"] is not None]
    out["pmin"] = min(pm) if pm else None
    out["z"], out["ranks_folded"] = z, np.array(ranks2).reshape(n, m)
    out["rhat_bulk"], out["ess_bulk"] = rs[0]["rhat"], rs[0]["ess"]
    out["ess_q05"], out["ess_q95"] = rs[1]["ess"], rs[2]["ess"]
    out["rhat_folded"] = NAN if nan2 else rs[3]["rhat"]
    a, b = out["rhat_bulk"], out["rhat_folded"]
    out["rhat"] = NAN if a != a or b != b else max(a, b)
    a, b = out["ess_q05"], out["ess_q95"]
    out["ess_tail"] = NAN if a != a or b != b else min(a, b)
    return out


def compare(got, ref, rtol, label=""):
    """one row of eight against a restatement: R-hat and ESS at rtol, distinct and the NaN pattern exactly; returns the worst error"""
    worst = 0.0
    for k, col in enumerate(COLS):
        g, w = float(got[k]), ref[col]
        assert math.isnan(g) == math.isnan(w), (label, col, g, w)
        if math.isnan(w):
            continue
        if col == "distinct":
            assert g == w, (label, g, w)
            continue
        err = 0.0 if g == w else abs(g - w) / abs(w)
        worst = max(worst, err)
        assert err <= rtol, (label, col, g, w, err)
    return worst


# ---- the inputs of the GPU tests: the AR(1) cases of the summary tests, made heavy-tailed or skewed by a monotone map --------------
CASES = R.AR1_CASES[:4]  # phi in {0, 0.9, -0.5, 0.5} at n in {64, 65, 129, 200}
TRANSFORMS = ("exp", "cauchy")


def transformed(x, how):
    """a monotone map of the AR(1) input (mean 100): exp of the centred value, or the Cauchy quantile of its normal probability"""
    c = x - 100.0
    if how == "exp":
        return np.exp(c)
    from scipy.special import ndtr
    sd = c.std()
    return np.tan(math.pi * (ndtr(c / (1.5 * sd)) - 0.5))


# ---- the geometry of the device code, restated (csrc/demc_rankplan.hpp; held to the planner below) -------------------------------
RANK_TILE, RANK_WG, RANK_SCAN_WG, RANK_MAX_BLOCKS, RANK_MAX_BATCH, RANK_BUDGET, RANK_BYTES = 2048, 256, 1024, 4096, 16, 4 << 30, 64


def geometry(n, P, series):
    """what demc_rankstats (series = D + 2) or demc_rank_series (series = 1) launches for n rows of P chains -> dict(N, tiles,
    last_tile (pairs of the last tile), blocks, batch, batches, last_batch, scan_chunk, passes)"""
    N = n * P
    tiles = -(-N // RANK_TILE)
    per = N * RANK_BYTES + tiles * 256 * 4
    batch = min(max(1, RANK_BUDGET // per), min(series, RANK_MAX_BATCH))
    batches = -(-series // batch)
    return dict(N=N, tiles=tiles, last_tile=N - (tiles - 1) * RANK_TILE, blocks=min(-(-N // RANK_WG), RANK_MAX_BLOCKS), batch=batch,
                batches=batches, last_batch=series - (batches - 1) * batch, scan_chunk=-(-(256 * tiles) // RANK_SCAN_WG), passes=8)


@functools.lru_cache(maxsize=None)
def program():
    """tests/rankplan_host.cpp, built once per session with the sanitizers"""
    tmp = tempfile.mkdtemp(prefix="rankplan_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "rankplan_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "rankplan_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def dump(requests):
    run = subprocess.run([program(), "--dump"], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(requests)
    out = []
    for line in lines:
        head, _, message = line.partition(" message=")
        d = {}
        for tok in head.split()[1:]:
            k, v = tok.split("=", 1)
            vals = [float.fromhex(t) if "x" in t else int(t) for t in v.split(",")]
            d[k] = vals if len(vals) > 1 else vals[0]
        if message:
            d["message"] = message
        out.append(d)
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_known_answers(demc):
    C = demc.chains
    r, distinct, has_nan = restate_ranks([3.0, 1.0, 2.0, 1.0])
    assert r == [4.0, 1.5, 3.0, 1.5] and distinct == 3 and not has_nan
    got = C.series_ranks(np.array([3.0, 1.0, 2.0, 1.0]))
    assert got[0].tolist() == r and got[1] == 3 and got[2] is False
    # all equal: every rank (N + 1) / 2, z constant, every R-hat and ESS NaN
    x = np.full((10, 4), 2.5)
    r, distinct, _ = restate_ranks(x.reshape(-1))
    assert set(r) == {20.5} and distinct == 1
    z = C.normal_scores(C.series_ranks(x)[0], 40)
    assert len(set(z.reshape(-1).tolist())) == 1
    row = C.series_rankstats(x)
    assert np.isnan(row[:7]).all() and row[7] == 1.0
    ref = restate(x)
    assert all(math.isnan(ref[c]) for c in COLS[:7]) and ref["distinct"] == 1.0
    # N = 1: r = 1 and z = Phi^-1(5 / 10) = 0
    r, distinct, _ = restate_ranks([7.0])
    assert r == [1.0] and distinct == 1 and C.normal_scores(np.array([1.0]), 1).tolist() == [0.0] and (1.0 - 0.375) / (1 + 0.25) == 0.5
    # -0.0 sorts before +0.0 and does not tie with it; a NaN makes every column NaN
    assert restate_ranks([0.0, -0.0, 0.0])[0] == [2.5, 1.0, 2.5] and C.series_ranks(np.array([0.0, -0.0, 0.0]))[0].tolist() == [2.5, 1.0, 2.5]
    x = R.ar1(16, 4, 0.5, 0)
    x[3, 2] = NAN
    assert np.isnan(C.series_rankstats(x)).all() and all(math.isnan(restate(x)[c]) for c in COLS)


def _inputs():
    out = []
    for n, m, phi in CASES:
        for how in TRANSFORMS:
            out.append(((n, m, phi, how), transformed(R.ar1(n, m, phi, 0), how)))
    rng = np.random.default_rng(9)
    ties = np.round(rng.normal(size=(40, 6)) * 3.0) / 3.0  # heavy ties, signed zeros among them
    ties[ties == 0.0] = np.where(rng.random((ties == 0.0).sum()) < 0.5, -0.0, 0.0)
    out.append((("ties",), ties))
    acc = (rng.random((64, 4)) < 0.3).astype(np.float64)  # two values: acceptance
    out.append((("acceptance",), acc))
    a = R.ar1(40, 8, 0.5, 0)
    a[:, 0:4] = -np.inf  # an infinite median: zeta holds NaNs, rhat_folded and rhat are NaN, bulk and tail are reported
    out.append((("-inf chains",), a))
    b = R.ar1(40, 8, 0.5, 1)
    b[3, 2] = -np.inf
    out.append((("-inf cell",), b))
    for n in (1, 2, 3, 7, 8):
        out.append(((f"n={n}",), R.ar1(n, 4, 0.5, 2)))
    out.append((("P=1",), transformed(R.ar1(65, 1, 0.5, 1), "exp")))  # (a handle needs Np >= 3: one chain is checked here only)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(n, m, phi, how, max_lag=0):
    """the restatement of one synthetic case (how: "raw", "exp" or "cauchy"), computed once and shared; read-only"""
    x = R.ar1(n, m, phi, 0)
    return restate(x if how == "raw" else transformed(x, how), max_lag)


@pytest.mark.parametrize("max_lag", [0, 5])
def test_series_rankstats_equals_the_restatement(demc, max_lag):
    C = demc.chains
    worst = 0.0
    for label, x in _inputs():
        ref = restate(x, max_lag)
        got_r = C.series_ranks(x)
        assert np.array_equal(got_r[0], ref["ranks"]) and (math.isnan(ref["distinct"]) or got_r[1] == ref["distinct"]), label  # ranks exactly
        row = C.series_rankstats(x, max_lag)
        worst = max(worst, compare(row, ref, 1e-12, label))
        if "z" in ref:
            z = C.normal_scores(got_r[0], x.size)
            assert np.abs(z - ref["z"]).max() <= PPND_BAR * max(1.0, np.abs(ref["z"]).max()), label
            with np.errstate(all="ignore"):
                zeta = np.abs(x - C.series_quantiles(x, (0.5,))[0])
            assert np.array_equal(C.series_ranks(zeta)[0], ref["ranks_folded"]), label
    print(f"series_rankstats vs the plain-loop restatement, max_lag={max_lag}: max relative error {worst:.3g}")
    # the NaN patterns the definition states
    ref = restate(dict(_inputs())[("-inf chains",)])
    assert math.isnan(ref["rhat"]) and math.isnan(ref["rhat_folded"]) and math.isfinite(ref["rhat_bulk"]) and math.isfinite(ref["ess_bulk"])
    ref = restate(dict(_inputs())[("acceptance",)])
    assert ref["distinct"] == 2.0 and math.isfinite(ref["ess_bulk"])
    for n in (1, 2, 3, 7, 8):  # DESIGN.md 5.5's rule in each column: rhat needs h >= 2, ess h >= 4
        ref = restate(dict(_inputs())[(f"n={n}",)])
        h = n // 2
        assert math.isfinite(ref["rhat"]) == math.isfinite(ref["rhat_bulk"]) == math.isfinite(ref["rhat_folded"]) == (h >= 2), n
        assert math.isfinite(ref["ess_bulk"]) == (h >= 4), n


def test_monotone_maps_leave_the_bulk_columns_alone(demc):
    """ranks do not see a monotone map: the bulk columns of exp(x) and of the Cauchy quantile equal those of x exactly"""
    for n, m, phi in CASES:
        x = R.ar1(n, m, phi, 0)
        base = demc.chains.series_rankstats(x)
        for how in TRANSFORMS:
            row = demc.chains.series_rankstats(transformed(x, how))
            assert row[1] == base[1] and row[3] == base[3] and row[7] == base[7] == n * m, (n, m, phi, how)


def test_no_synthetic_input_sits_on_a_zero_pair():
    """the margin condition of the summary tests, on every derived series of every input of the GPU tests: a failure asks for
    another seed, never for a skip"""
    worst = math.inf
    for label, x in _inputs():
        for max_lag in (0, 5):
            ref = restate(x, max_lag)
            if ref["pmin"] is not None:
                worst = min(worst, ref["pmin"])
                assert ref["pmin"] >= R.MARGIN, (label, max_lag, ref["pmin"])
    print(f"smallest |P_k| over the derived series of the synthetic inputs: {worst:.3g}")


def _ppnd_arguments():
    args = []
    for N in (1, 2, 7, 1000):
        r = 1.0
        while r <= N:
            args.append((r - 0.375) / (N + 0.25))
            r += 0.5
    N = 2 ** 31 - 1
    for r in (1.0, 1.5, 2.0, 2.5, 3.0, N - 1.0, N - 0.5, float(N)):
        args.append((r - 0.375) / (N + 0.25))
    return args


def test_inverse_normal_against_mpmath(demc):
    """ppnd16 -- numpy's restatement and the C++ text the device compiles -- against mpmath at 40 digits ON THE FP64 ARGUMENTS
    (r - 3/8) / (N + 1/4), r in {1, 1.5, ..., N}, N in {1, 2, 7, 1000}, and both ends of N = 2^31 - 1.  The largest relative error is
    measured and printed; the bar is four times the measured value recorded above, and that must stay below 1e-13."""
    import mpmath
    from scipy.special import ndtri
    args = _ppnd_arguments()
    got = demc.chains.ppnd16(np.array(args))
    text = [d["z"] for d in dump([f"Z {float(p).hex()}" for p in args])]
    worst = worst_text = worst_scipy = 0.0
    with mpmath.workdps(40):
        for p, g, t in zip(args, got, text):
            want = mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(p) - 1)
            if want == 0:
                assert g == 0.0 and t == 0.0
                continue
            worst = max(worst, float(abs((mpmath.mpf(float(g)) - want) / want)))
            worst_text = max(worst_text, float(abs((mpmath.mpf(float(t)) - want) / want)))
            worst_scipy = max(worst_scipy, float(abs((mpmath.mpf(float(ndtri(p))) - want) / want)))
    print(f"ppnd16 against mpmath over {len(args)} arguments: numpy {worst:.3g}, the C++ text {worst_text:.3g} (scipy's ndtri: {worst_scipy:.3g})")
    assert PPND_BAR <= 1e-13
    assert worst <= PPND_MEASURED and worst_text <= PPND_MEASURED, "the measured value moved: record it (and in DESIGN.md 5.11)"
    assert worst_scipy <= 1e-13  # the second witness agrees with the reference too
    # the two texts give the same bits wherever the host's log and sqrt are the same functions
    assert np.abs(np.array(text) - got).max() <= PPND_BAR * np.abs(got).max()


def test_plans_under_the_sanitizers():
    run = subprocess.run([program()], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "rankplan ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr[-4000:]


def test_python_restatement_is_the_plan():
    c = dump(["const"])[0]
    assert (c["kRankTile"], c["kRankWG"], c["kRankScanWG"], c["kRankMaxBlocks"], c["kRankMaxBatch"], c["kRankBudget"], c["kRankBytesPerValue"]) == \
        (RANK_TILE, RANK_WG, RANK_SCAN_WG, RANK_MAX_BLOCKS, RANK_MAX_BATCH, RANK_BUDGET, RANK_BYTES)
    assert c["kRankBits"] == 8 and c["kRankPasses"] == 8 and c["kRankWave"] == 64 and c["kRankDerived"] == 4 and c["DEMC_RANK_COLS"] == len(COLS)
    shapes = sorted({(n, P, s) for n in (1, 2, 3, 7, 64, 65, 129, 200, 256, 257, 1000, 2048, 24577) for P in (1, 3, 4, 8, 16, 24, 2048, 4096, 65536)
                     for s in (1, 3, 4, 11, 16, 17, 34)})
    for (n, P, s), p in zip(shapes, dump([f"P {n} {P} {s}" for n, P, s in shapes])):
        g = geometry(n, P, s)
        assert {k: p[k] for k in ("N", "tiles", "blocks", "batch", "batches", "last_batch", "scan_chunk", "passes")} == \
            {k: g[k] for k in ("N", "tiles", "blocks", "batch", "batches", "last_batch", "scan_chunk", "passes")}, (n, P, s, g, p)
        assert [j - 1 for j in p["j"]] == [Q.targets(n * P, (q,))[0] for q in PROBS], (n, P)


def test_plan_is_written_in_the_host_only_header():
    header = open(os.path.join(CSRC, "demc_rankplan.hpp")).read()
    for word in ("hip", "ALLOC", "demc_handle", "getenv"):
        assert word not in header, word
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".hpp")) or f == "Makefile"}
    for name, text in sources.items():
        assert "getenv" not in text, name
    runtime = sources["demc_hip.cpp"]
    texts = re.findall(r'"((?:[^"\\]|\\.)*)"', re.sub(r"//.*|static_assert\(.*", "", header))
    refusals = [t for t in texts if " " in t and not t.endswith((".h", ".hpp"))]
    assert len(refusals) == 8, refusals
    for t in refusals:  # written once, in the header
        assert sum(text.count('"' + t + '"') for text in sources.values()) == 1, t
    assert runtime.count("plan_rank(") == 1 and sum(text.count("plan_rank(") for n, text in sources.items() if n not in ("demc_hip.cpp", "demc_rankplan.hpp")) == 0
    assert runtime.count("plan_summary(") == 1 and runtime.count("sum_plan(") == 4  # its definition, demc_summarize, a whole batch, the last one
    assert "$(OBJ).rank.o" in sources["Makefile"] and "demc_rank.cpp -o $@" in sources["Makefile"]
    unit = sources["demc_rank.cpp"]
    assert unit.count("finish(who, st,") == 1 and "hipStreamSynchronize" not in unit and "hipMalloc" not in unit
    for word in ("atomicAdd(double", "unsafeAtomicAdd", "atomicAdd_system"):
        assert word not in unit
    assert '#include "demc_ppnd.hpp"' in unit and "hip" not in open(os.path.join(CSRC, "demc_ppnd.hpp")).read().replace("__HIPCC__", "").lower()


def test_rank_kernels_use_no_scratch(tmp_path, demc):
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_rank_" in k[0]]
    assert len(ks) == 10, [k[0] for k in ks]
    for name, regs, agpr, wg, scratch in ks:
        assert scratch == 0 and regs <= 160 and wg in (64, 256, 1024), (name, regs, wg, scratch)


# ---- the header, the library and both bindings --------------------------------------------------------------------------------------
def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demc_rank.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return text, protos


def test_header_library_and_python_binding_agree(demc):
    import ctypes as C
    F = demc._ffi
    text, protos = _prototypes()
    assert sorted(protos) == sorted(F.RANK_EXPORTS) == ["demc_rank_series", "demc_rankstats"]
    for other in (F.EXPORTS, F.SUMMARY_EXPORTS, F.QUANTILE_EXPORTS, F.COV_EXPORTS, F.PW_EXPORTS, F.LOO_EXPORTS, F.BRIDGE_EXPORTS):
        assert not set(protos) & set(other), "declared in another header as well"
    for h in ("demc.h", "demc_summary.h", "demc_quantile.h", "demc_cov.h", "demc_pointwise.h", "demc_loo.h", "demc_bridge.h"):
        assert "demc_rank" not in open(os.path.join(ROOT, "include", h)).read(), h
    lib = F.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "demc_handle*": C.c_void_p}
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args], (name, args)
    assert len(protos["demc_rankstats"][1]) == 5 and len(protos["demc_rank_series"][1]) == 6
    assert int(re.search(r"#define DEMC_RANK_COLS (\d+)", text).group(1)) == len(demc.chains.RANK_COLS) == F.RANK_COLS == 8
    assert demc.chains.RANK_COLS == COLS and demc.chains.RANK_PROBS == PROBS
    for name, value in (("RANK", 0), ("SCORE", 1), ("FOLDED", 2)):
        assert re.search(rf"#define DEMC_RANK_KIND_{name} {value}\b", text) and getattr(F, f"RANK_KIND_{name}") == value
    assert '#include "demc.h"' in text
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "demc_rank.h")])
    assert callable(getattr(F.HipEngine, "rankstats")) and callable(getattr(F.HipEngine, "rank_series"))


def test_julia_ccall_matches_the_prototype(demc):
    import test_julia_shim as J
    _, protos = _prototypes()
    main_jl = open(os.path.join(ROOT, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPRank.jl")' in main_jl and "demc_rank" not in main_jl
    jl = open(os.path.join(ROOT, "julia", "DEMCHIPRank.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= set(protos)
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
    names = re.search(r"const RANK_COLS = \(([^)]*)\)", jl).group(1)
    assert tuple(n.strip().lstrip(":") for n in names.split(",")) == demc.chains.RANK_COLS


# ---- the public surface ---------------------------------------------------------------------------------------------------------------
def test_chains_rankstats_and_the_fallback_of_summarize(demc):
    """Chains.rankstats is series_rankstats per series; summarize(..., rank=True) through an injected engine without rankstats exports
    and ranks on the host, and equals sample(...).rankstats(); with rank=False nothing of it is there"""
    calls = []

    class Eng:  # has summarize, has no rankstats
        def __init__(self, **cfg):
            self.P, self.D, self.rows = cfg["n_groups"] * cfg["Np"], cfg["D"], cfg["n_rows"]
            rng = np.random.default_rng(1)
            self.full = np.concatenate([rng.standard_cauchy(size=(self.rows, self.D, self.P)), (rng.random((self.rows, 1, self.P)) < 0.3) * 1.0,
                                        rng.normal(size=(self.rows, 1, self.P))], axis=1)

        def __getattr__(self, name):
            if name.startswith(("set_", "step", "close")):
                return lambda *a, **k: None
            raise AttributeError(name)

        def summarize(self, *a):
            raise AssertionError("the device statistics were asked for although the rank diagnostics cannot follow them")

        def export_chains(self, r0, r1):
            calls.append("export")
            return self.full[r0:r1]

        def get_state(self):
            return np.zeros((self.P, self.D)), np.zeros(self.P), np.arange(self.P)

    D = demc

    def run(fn, **kw):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("μ", "σ"), data=np.zeros(5), prior_loglike=D.Priors(μ=D.Normal(0, 1), σ=D.TruncatedCauchy(0, 1)),
                          loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=20, Np=4, n_groups=2)
        return fn(model, de, D.HIPBackend(seed=3), 60, engine_factory=Eng, **kw)

    chains = run(D.sample)
    host = chains.rankstats()
    assert host.names == ["μ", "σ", "acceptance", "lp"] and host.values.shape == (4, 8)
    for j in range(4):
        assert Q.same_bits(host.values[j], D.chains.series_rankstats(chains.value[:, j, :]))
    s = run(D.summarize, rank=True)
    assert isinstance(s.rank, D.RankStats) and s.rank.names == host.names and Q.same_bits(s.rank.values, host.values)
    assert set(s.rank.describe()) == {"μ", "σ"} and set(s.rank["μ"]) == set(COLS) and "ess_bulk" in repr(s.rank)
    assert np.isfinite(s.rank.values[:2, :3]).all()
    assert calls == ["export", "export"]
    with pytest.raises(AssertionError, match="device statistics"):  # rank=False: the call is what it was -- it asks the engine's summarize
        run(D.summarize)
