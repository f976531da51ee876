"""Highest-density intervals (demc_hpd on the device, Chains.hpd / chains.series_hpd on the host) against an
independent restatement of the definition in plain loops -- MCMCChains' _hpd as its text reads: Python's sorted() on integer keys, the
two slices, the first minimum in a loop; nothing below is shared with chains.py --, the properties an interval of that definition
has, the NaN rule, the plan program of csrc/demc_hpdplan.hpp (tests/hpdplan_host.cpp) under the sanitizers and held to its Python
restatement, the header against the library and both bindings, and the geometry the GPU tests of the same feature assert
(tests/test_gpu_hpd.py).  No GPU here."""
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
import test_rank_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "differentialevolutionmcmc.jl_amd", "csrc")
NAN = float("nan")
INF = float("inf")
COLS = ("lower", "upper", "first", "m")
ALPHAS = (1e-9, 0.01, 0.05, 0.2, 1.0 / 3.0, 0.5, 0.8, 0.95, 0.999, 1.0 - 1e-9)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def candidates(N, alpha):
    """m = max(1, ceil(alpha N)): Python's float product is the one rounded double multiplication"""
    return max(1, math.ceil(float(alpha) * float(N)))


def restate(values, alphas):
    """DESIGN.md 5.12 for one pool, one step after the other -> [(lower, upper, first, m) for alpha in alphas]"""
    ks = sorted(Q.key(float(v)) for v in values)
    N = len(ks)
    assert N >= 1
    has_nan = ks[0] < Q.KEY_NEG_INF or ks[-1] > Q.KEY_POS_INF
    y = [Q.unkey(k) for k in ks]
    out = []
    for alpha in alphas:
        m = candidates(N, alpha)
        assert 1 <= m <= N
        if has_nan:
            out.append((NAN, NAN, NAN, float(m)))
            continue
        lo, hi = y[:m], y[N - m:]  # a = sort(x)[1:m], b = sort(x)[(n - m + 1):n]
        best_w, best_i = None, None
        for i in range(m):  # findmin(b - a): a NaN ranks below every number, the first of equals wins
            w = hi[i] - lo[i]  # (inf - inf is NaN in Python too)
            if best_i is None:
                best_w, best_i = w, i
            elif best_w != best_w:
                break  # a NaN has been met: nothing ranks below it and it came first
            elif w != w or w < best_w:
                best_w, best_i = w, i
        out.append((lo[best_i], hi[best_i], float(best_i), float(m)))
    return out


def pools():
    """(label, values) over the shapes of a pool the definition speaks about, N from 1 to a few thousand"""
    rng = np.random.default_rng(512)
    out = []
    for N in (1, 2, 3, 7, 64, 255, 256, 257, 1000, 3001):
        x = rng.normal(size=N)
        out.append((f"normal N={N}", x))
        out.append((f"ties N={N}", np.round(rng.normal(size=N) * 2.0) / 2.0))
        out.append((f"all equal N={N}", np.full(N, 2.5)))
        out.append((f"two values N={N}", (rng.random(N) < 0.3) * 1.0))
        mixed = rng.normal(size=N)
        mixed[rng.random(N) < 0.2] = 0.0
        mixed[rng.random(N) < 0.2] = -0.0
        out.append((f"both zeros N={N}", mixed))
        for label, ends in (("-inf", (-INF,)), ("+inf", (INF,)), ("both infinities", (-INF, INF))):
            for share in (0.1, 0.6):
                y = rng.normal(size=N)
                for e in ends:
                    y[rng.random(N) < share / len(ends)] = e
                out.append((f"{label} in {share:.0%} N={N}", y))
        out.append((f"skewed N={N}", np.exp(rng.normal(size=N) * 2.0)))
        out.append((f"near 1e16 N={N}", 1e16 + 2.0 * rng.integers(0, 50, N)))  # distinct true widths round to the same double
    return out


def check_row(got, want, label):
    assert Q.same_bits(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64)), (label, list(got), list(want))


# ---- the geometry of the device code, restated (csrc/demc_hpdplan.hpp; held to the planner below) --------------------------------
HPD_WG, HPD_MAX_BLOCKS, HPD_BYTES, HPD_MAX_ALPHAS = 256, 64, 24, 16


def geometry(n, P, series, alphas):
    """what demc_hpd (series = D + 2) launches for n rows of P chains -> dict(N, tiles, last_tile, blocks, scan_chunk, passes (the sort
    of one series, as test_rank_host.geometry states it), batch, batches, last_batch, m, wgs (workgroups of the window kernel) and
    trips (candidates a thread of it takes at most) per alpha, slots)"""
    g = H.geometry(n, P, 1)
    N = g["N"]
    per = N * HPD_BYTES + g["tiles"] * 256 * 4
    batch = min(max(1, H.RANK_BUDGET // per), min(series, H.RANK_MAX_BATCH))
    batches = -(-series // batch)
    m = [candidates(N, a) for a in alphas]
    wgs = [min(-(-mk // HPD_WG), HPD_MAX_BLOCKS) for mk in m]
    return dict(N=N, tiles=g["tiles"], last_tile=g["last_tile"], blocks=g["blocks"], scan_chunk=g["scan_chunk"], passes=g["passes"], batch=batch,
                batches=batches, last_batch=series - (batches - 1) * batch, m=m, wgs=wgs, trips=[-(-mk // (w * HPD_WG)) for mk, w in zip(m, wgs)],
                slots=max(wgs))


def sort_passes(x):
    """(passes the sort of this pool runs, the buffer that holds the sorted pairs after them): a digit the whole pool shares is
    skipped -- csrc/demc_rank.cpp's rank_diff / rank_src on the host"""
    k = np.ascontiguousarray(x, dtype=np.float64).reshape(-1).view(np.uint64)
    k = k ^ np.where(k >> np.uint64(63) != 0, np.uint64(Q.ALL), np.uint64(Q.SIGN))
    diff = int(np.bitwise_or.reduce(k) & np.bitwise_or.reduce(~k))
    ran = sum(1 for d in range(8) if (diff >> (8 * d)) & 0xFF)
    return ran, ran & 1


@functools.lru_cache(maxsize=None)
def program():
    """tests/hpdplan_host.cpp, built once per session with the sanitizers; no ROCm include path"""
    tmp = tempfile.mkdtemp(prefix="hpdplan_host_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "hpdplan_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "hpdplan_host.cpp"), "-o", exe],
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
            d[k] = [int(t) for t in v.split(",")] if k in ("m", "wgs") else int(v)
        if message:
            d["message"] = message
        out.append(d)
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_known_answers(demc):
    C = demc.chains
    # six values, alpha = 0.5: m = 3 candidates [1, 2.6], [2, 3], [2.5, 10]; the narrowest is the second
    x = [3.0, 1.0, 2.0, 10.0, 2.5, 2.6]
    assert restate(x, (0.5,)) == [(2.0, 3.0, 1.0, 3.0)]
    check_row(C.series_hpd(np.array(x), (0.5,))[0], (2.0, 3.0, 1.0, 3.0), "six values")
    # m = 1: the whole range; m = N: the first value twice, width zero
    assert restate(x, (1e-9, 0.9)) == [(1.0, 10.0, 0.0, 1.0), (1.0, 1.0, 0.0, 6.0)]
    # all equal: every width ties at zero and the first candidate wins; a ramp: every width ties at N - m
    assert restate([2.5] * 40, (0.05, 0.5)) == [(2.5, 2.5, 0.0, 2.0), (2.5, 2.5, 0.0, 20.0)]
    assert restate(list(range(40)), (0.25,)) == [(0.0, 30.0, 0.0, 10.0)]
    # -0.0 sorts before +0.0: m = 3 candidates [-0, +0], [+0, 5], [5, 7]; the interval of the two zeros starts at the negative one
    row = C.series_hpd(np.array([0.0, -0.0, 5.0, 7.0]), (0.75,))[0]
    assert row[0] == 0.0 == row[1] and math.copysign(1.0, row[0]) == -1.0 and math.copysign(1.0, row[1]) == 1.0 and row[2] == 0.0 and row[3] == 3.0
    lo, hi, first, m = restate([0.0, -0.0, 5.0, 7.0], (0.75,))[0]
    assert lo == 0.0 == hi and math.copysign(1.0, lo) == -1.0 and math.copysign(1.0, hi) == 1.0 and (first, m) == (0.0, 3.0)
    # alpha is used as passed: 0.05 x 100 rounds to 5.0 exactly, although 0.05 is above 1 / 20 and 1 - 0.95 is not 0.05
    assert candidates(100, 0.05) == 5 == C.hpd_candidates(100, 0.05) and candidates(100, 1 - 0.95) == 6 == C.hpd_candidates(100, 1 - 0.95)
    assert C.HPD_COLS == COLS
    with pytest.raises(ValueError):
        C.series_hpd(np.array([]), (0.5,))


def test_series_hpd_equals_the_restatement_bit_for_bit(demc):
    C = demc.chains
    rows = 0
    for label, x in pools():
        got = C.series_hpd(x, ALPHAS)
        want = restate([float(v) for v in x], ALPHAS)
        assert got.shape == (len(ALPHAS), 4)
        for a, g, w in zip(ALPHAS, got, want):
            check_row(g, w, (label, a))
            assert g[3] == C.hpd_candidates(x.size, a) == candidates(x.size, a)
            rows += 1
        shaped = x.reshape(-1, 1) if x.size % 2 else x.reshape(2, -1)  # the chains are pooled: the shape does not matter
        assert Q.same_bits(C.series_hpd(shaped, ALPHAS), got), label
    print(f"series_hpd vs the plain-loop restatement: {rows} intervals, bit for bit")


def test_properties_of_an_interval(demc):
    """the interval holds at least N - m + 1 pool values, no candidate is narrower, first + (N - m) is the sorted position of upper,
    m is ceil(alpha N) clipped below at 1"""
    C = demc.chains
    for label, x in pools():
        y = np.sort(x)  # (by value: the pools of this test hold no NaN, and the counts below do not tell the zeros apart)
        N = x.size
        for alpha, (lower, upper, first, m) in zip(ALPHAS, C.series_hpd(x, ALPHAS)):
            first, m = int(first), int(m)
            assert m == max(1, math.ceil(alpha * N)) and 1 <= m <= N and 0 <= first < m, (label, alpha)
            assert y[first] == lower and y[first + N - m] == upper, (label, alpha)
            assert np.count_nonzero((x >= lower) & (x <= upper)) >= N - m + 1, (label, alpha)
            with np.errstate(all="ignore"):
                w = y[N - m:] - y[:m]
                mine = upper - lower
            if np.isnan(w).any():  # the first NaN width
                assert math.isnan(mine) and first == int(np.flatnonzero(np.isnan(w))[0]), (label, alpha)
            else:
                assert (mine <= w).all() and (w[:first] > mine).all(), (label, alpha)


def test_the_nan_rule_and_infinite_ends(demc):
    C = demc.chains
    rng = np.random.default_rng(77)
    N, alpha = 200, 0.25  # m = 50: a candidate spans 151 values
    m = candidates(N, alpha)
    assert m == 50
    for inf in (INF, -INF):
        for count in (N - m + 1, N - m + 20, N):  # more than N - m of the pool: some candidate has both ends there
            x = rng.normal(size=N)
            x[rng.permutation(N)[:count]] = inf
            row, ref = C.series_hpd(x, (alpha,))[0], restate(x.tolist(), (alpha,))[0]
            check_row(row, ref, (inf, count))
            first_nan = N - count if inf > 0 else 0  # +inf fills the top: the first candidate whose lower end is +inf; -inf the bottom
            assert row[0] == inf and row[1] == inf and row[2] == first_nan and row[3] == m, (inf, count, row)
        x = rng.normal(size=N)  # exactly N - m of them: every candidate still has a finite end, widths of +inf tie, the first wins
        x[rng.permutation(N)[:N - m]] = inf
        row = C.series_hpd(x, (alpha,))[0]
        check_row(row, restate(x.tolist(), (alpha,))[0], (inf, "N - m"))
        assert row[2] == 0.0 and np.isinf(row[[0, 1]]).sum() == 1
        x = rng.normal(size=N)  # a few: their candidates have infinite widths and never win
        x[:5] = inf
        row = C.series_hpd(x, (alpha,))[0]
        check_row(row, restate(x.tolist(), (alpha,))[0], (inf, "a few"))
        assert np.isfinite(row).all()
    x = rng.normal(size=N)
    x[17] = NAN
    for got in (C.series_hpd(x, (alpha, 0.5)), np.array(restate(x.tolist(), (alpha, 0.5)))):
        assert np.isnan(got[:, :3]).all() and got[:, 3].tolist() == [50.0, 100.0]
    x[17] = -NAN  # a NaN with the sign bit set has a key below -inf
    assert np.isnan(C.series_hpd(x, (alpha,))[0, :3]).all() and C.series_hpd(x, (alpha,))[0, 3] == 50.0


def test_plans_under_the_sanitizers():
    run = subprocess.run([program()], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "hpdplan ok" in run.stdout and "runtime error" not in run.stderr, run.stdout + run.stderr[-4000:]


def test_python_restatement_is_the_plan(demc):
    c = dump(["const"])[0]
    assert (c["kHpdWG"], c["kHpdMaxBlocks"], c["kHpdBytesPerValue"], c["DEMC_HPD_MAX_ALPHAS"]) == (HPD_WG, HPD_MAX_BLOCKS, HPD_BYTES, HPD_MAX_ALPHAS)
    assert c["DEMC_HPD_COLS"] == len(COLS) and c["kHpdFinalWG"] == 64
    alphas = (1e-9, 0.05, 0.5, 0.999)
    shapes = sorted({(n, P, s) for n in (1, 2, 3, 7, 64, 89, 256, 257, 683, 1000, 2050, 2051, 2052, 24577) for P in (1, 3, 4, 8, 23, 24, 2048, 65536)
                     for s in (1, 4, 9, 11, 16, 17, 34)})
    asked = " ".join(float(a).hex() for a in alphas)
    for (n, P, s), p in zip(shapes, dump([f"H {n} {P} {s} {asked}" for n, P, s in shapes])):
        g = geometry(n, P, s, alphas)
        keys = ("N", "tiles", "blocks", "batch", "batches", "last_batch", "scan_chunk", "passes", "slots", "m", "wgs")
        assert {k: p[k] for k in keys} == {k: g[k] for k in keys}, (n, P, s, g, p)
        assert g["m"] == [demc.chains.hpd_candidates(n * P, a) for a in alphas]
    refused = dump(["H 4 4 4", f"H 4 4 4 {(1.0).hex()}", f"H 2097152 1024 4 {(0.5).hex()}"])
    assert [r["refused"] for r in refused] == [demc._ffi.EINVAL, demc._ffi.EINVAL, demc._ffi.EUNSUPPORTED]
    assert "n_alphas" in refused[0]["message"] and "strictly inside (0, 1)" in refused[1]["message"] and "2^31" in refused[2]["message"]


def test_plan_is_written_in_the_host_only_header():
    header = open(os.path.join(CSRC, "demc_hpdplan.hpp")).read()
    for word in ("hip", "ALLOC", "demc_handle", "getenv"):
        assert word not in header, word
    sources = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".cpp", ".hpp")) or f == "Makefile"}
    runtime = sources["demc_hip.cpp"]
    texts = re.findall(r'"((?:[^"\\]|\\.)*)"', re.sub(r"//.*|static_assert\(.*", "", header))
    refusals = [t for t in texts if " " in t and not t.endswith((".h", ".hpp"))]
    assert len(refusals) == 8, refusals
    for t in refusals:  # written once, in the header
        assert sum(text.count('"' + t + '"') for text in sources.values()) == 1, t
    assert runtime.count("plan_hpd(") == 1 and sum(text.count("plan_hpd(") for n, text in sources.items() if n not in ("demc_hip.cpp", "demc_hpdplan.hpp")) == 0
    assert runtime.count("hpd_run(") == 1 and runtime.count("sort_plan(") == 3  # its definition, the rank calls, demc_hpd
    assert "demc_hpdplan.hpp" in sources["Makefile"] and "../../include/demc_hpd.h" in sources["Makefile"]
    unit = sources["demc_rank.cpp"]  # where the kernels of the sort live, and so the two of demc_hpd
    assert "k_hpd_window" in unit and "k_hpd_final" in unit and "hipStreamSynchronize" not in unit and "hipMalloc" not in unit
    window = unit[unit.index("void k_hpd_window"):unit.index("void sort_round")]
    for word in ("atomic", "asm", "__builtin_amdgcn"):  # nothing in the result may depend on arrival order; plain C++
        assert word not in window, word


def test_hpd_kernels_use_no_scratch(tmp_path, demc):
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_hpd_" in k[0]]
    assert len(ks) == 2, [k[0] for k in ks]
    for name, regs, agpr, wg, scratch in ks:
        assert scratch == 0 and regs <= 64 and wg in (64, 256), (name, regs, wg, scratch)


# ---- the header, the library and both bindings --------------------------------------------------------------------------------------
def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "demc_hpd.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return text, protos


def test_header_library_and_python_binding_agree(demc):
    import ctypes as C
    F = demc._ffi
    text, protos = _prototypes()
    assert sorted(protos) == sorted(F.HPD_EXPORTS) == ["demc_hpd"]
    for other in (F.EXPORTS, F.SUMMARY_EXPORTS, F.QUANTILE_EXPORTS, F.COV_EXPORTS, F.PW_EXPORTS, F.LOO_EXPORTS, F.BRIDGE_EXPORTS, F.RANK_EXPORTS):
        assert not set(protos) & set(other), "declared in another header as well"
    for h in ("demc.h", "demc_summary.h", "demc_quantile.h", "demc_cov.h", "demc_pointwise.h", "demc_loo.h", "demc_bridge.h", "demc_rank.h"):
        assert "demc_hpd" not in open(os.path.join(ROOT, "include", h)).read(), h
    lib = F.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "constdouble*": C.POINTER(C.c_double),
             "demc_handle*": C.c_void_p}
    (ret, args), = protos.values()
    fn = lib.demc_hpd
    assert fn.restype is ctype[ret] and list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args] and len(args) == 6
    assert int(re.search(r"#define DEMC_HPD_COLS (\d+)", text).group(1)) == len(demc.chains.HPD_COLS) == F.HPD_COLS == 4
    assert int(re.search(r"#define DEMC_HPD_MAX_ALPHAS (\d+)", text).group(1)) == demc.chains.HPD_MAX_ALPHAS == F.HPD_MAX_ALPHAS == HPD_MAX_ALPHAS
    assert demc.chains.HPD_COLS == COLS
    assert '#include "demc.h"' in text
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "demc_hpd.h")])
    assert callable(getattr(F.HipEngine, "hpd"))


def test_julia_ccall_matches_the_prototype(demc):
    import test_julia_shim as J
    _, protos = _prototypes()
    main_jl = open(os.path.join(ROOT, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPHpd.jl")' in main_jl and "demc_hpd" not in main_jl
    assert main_jl.index('include("DEMCHIPRank.jl")') < main_jl.index('include("DEMCHIPHpd.jl")')  # run_then is the rank file's
    jl = open(os.path.join(ROOT, "julia", "DEMCHIPHpd.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} == set(protos)
    for m in calls:
        end = J.balanced(jl, m.end() - 1)
        jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
        cret, ctypes_ = protos[m.group(1)]
        assert jtypes == [J.julia_type(c) for c in ctypes_], (jtypes, ctypes_)
        assert re.match(r"::([A-Za-z0-9{}]+)", jl[end:]).group(1) == J.julia_type(cret)
    names = re.search(r"const HPD_COLS = \(([^)]*)\)", jl).group(1)
    assert tuple(n.strip().lstrip(":") for n in names.split(",")) == demc.chains.HPD_COLS


# ---- the public surface ---------------------------------------------------------------------------------------------------------------
def test_chains_hpd_and_the_fallback_of_summarize(demc):
    """Chains.hpd is series_hpd per series; summarize(..., hpd=...) through an injected engine without hpd exports and takes the
    intervals on the host, and equals sample(...).hpd(...); with hpd=None nothing of it is there"""
    calls = []

    class Eng:  # has summarize, has no hpd
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
            raise AssertionError("the device statistics were asked for although the intervals cannot follow them")

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
    host = chains.hpd()
    assert isinstance(host, D.Hpd) and host.names == ["μ", "σ", "acceptance", "lp"] and host.values.shape == (4, 1, 4) and host.alphas == (0.05,)
    for j in range(4):
        assert Q.same_bits(host.values[j], D.chains.series_hpd(chains.value[:, j, :], (0.05,)))
    assert set(host.describe()) == {"μ", "σ"} and set(host["μ"]) == set(COLS) and set(host.describe()["μ"]) == {"lower", "upper"}
    assert host["μ"]["lower"] <= host["μ"]["upper"] and host["μ"]["m"] == math.ceil(0.05 * 40 * 8) and "95%" in repr(host)
    two = chains.hpd((0.05, 0.5))
    assert two.values.shape == (4, 2, 4) and Q.same_bits(two.values[:, 0], host.values[:, 0]) and set(two["σ"]) == {0.05, 0.5}
    assert set(two.describe()["σ"][0.5]) == {"lower", "upper"}
    s = run(D.summarize, hpd=0.05)
    assert isinstance(s.hpd, D.Hpd) and s.hpd.names == host.names and Q.same_bits(s.hpd.values, host.values) and s.rank is None
    s2 = run(D.summarize, hpd=(0.05, 0.5))
    assert s2.hpd.alphas == (0.05, 0.5) and Q.same_bits(s2.hpd.values, two.values)
    assert calls == ["export", "export", "export"]
    for bad in (0.0, 1.0, (), (0.5,) * 17, float("nan")):
        with pytest.raises(ValueError):
            chains.hpd(bad)
        with pytest.raises(ValueError):
            run(D.summarize, hpd=bad)
    with pytest.raises(AssertionError, match="device statistics"):  # hpd=None: the call is what it was -- it asks the engine's summarize
        run(D.summarize)
    assert D.Summary(["a"], np.zeros((1, 6))).hpd is None
