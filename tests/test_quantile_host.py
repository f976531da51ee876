"""Posterior quantiles (demc_quantiles on the device, chains.series_quantiles on the host) against an independent
restatement of the definition in plain loops -- Python `sorted` on integer keys, Python float arithmetic, nothing shared with
chains.py -- plus the launch geometry and the inputs the GPU tests of the same feature import (tests/test_gpu_quantile.py).
No GPU here."""
import math
import struct

import numpy as np
import pytest

NAN = float("nan")
DEFAULT = (0.025, 0.25, 0.5, 0.75, 0.975)
PROBS = DEFAULT + (0.0, 1.0, 1.0 / 3.0)  # what the GPU cases ask for unless they say otherwise
ALL, SIGN = (1 << 64) - 1, 1 << 63
KEY_NEG_INF, KEY_POS_INF = 0x000FFFFFFFFFFFFF, 0xFFF0000000000000


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def key(x):
    b = bits(x)
    return b ^ (ALL if b >> 63 else SIGN)


def unkey(k):
    return from_bits(k ^ (SIGN if k >> 63 else ALL))


def _mul(a, b):  # IEEE products and sums of Python floats: no exception on overflow, inf - inf and 0 * inf are NaN
    return float(np.float64(a) * np.float64(b))


def _add(a, b):
    return float(np.float64(a) + np.float64(b))


def restate(values, probs):
    """DESIGN.md 5.6 for one pool, one operation after the other -> [quantile at p for p in probs]"""
    ks = sorted(key(float(v)) for v in values)
    N = len(ks)
    assert N >= 1
    if ks[0] < KEY_NEG_INF or ks[-1] > KEY_POS_INF:
        return [NAN] * len(probs)
    x = [unkey(k) for k in ks]  # x[0] = x_(1)
    out = []
    for p in probs:
        p = float(p)
        assert 0.0 <= p <= 1.0
        if N == 1:
            out.append(x[0])
            continue
        aleph = float(N) * p  # a rounded product ...
        aleph = aleph + (1.0 - p)  # ... followed by a rounded sum
        j = max(1, min(int(math.trunc(aleph)), N - 1))
        g = min(1.0, max(0.0, aleph - float(j)))
        a, b = x[j - 1], x[j]
        with np.errstate(all="ignore"):
            if math.isfinite(a) and math.isfinite(b):
                out.append(_add(a, _mul(g, _add(b, -a))))
            elif g == 0.0:
                out.append(a)
            elif g == 1.0:
                out.append(b)
            else:
                out.append(_add(_mul(1.0 - g, a), _mul(g, b)))
    return out


def restate_all(value, probs):
    """value[n][series][m] (the Chains value array) -> [series][prob], the chains pooled"""
    return np.array([restate(value[:, j, :].reshape(-1).tolist(), probs) for j in range(value.shape[1])], dtype=np.float64).reshape(
        value.shape[1], len(probs))


def same_bits(a, b):
    """equal bit for bit, where a NaN equals any NaN (the NaN PATTERN is what is compared)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


# ---- the launch geometry of the device code, restated: the kQ* constants and plan_quantiles' arithmetic (csrc/demc_postplan.hpp;
# tests/test_postplan_host.py holds this copy to the planner).  The GPU cases assert the geometry they were chosen for, so a changed
# constant fails them instead of moving them to another path.
Q_BITS, Q_WG, Q_MAX_WG, Q_SLOTS, Q_PROBES, Q_MAX_TARGETS, Q_MAX_CHUNKS_PER_WG = 8, 512, 512, 64, 4, 32, 1 << 22


def hist_ld(D, partner_history=False):
    """doubles between two history cells: padded when partners are gathered from the history and D <= 64"""
    if partner_history and D <= 64:
        return 1 << (D - 1).bit_length() if D <= 16 else (D + 15) // 16 * 16
    return D


def targets(N, probs):
    """the distinct 0-based ranks a call selects"""
    r = set()
    for p in probs:
        aleph = float(N) * p + (1.0 - p)
        j = 1 if N == 1 else max(1, min(int(math.trunc(aleph)), N - 1))
        r.add(j - 1)
        if N > 1:
            r.add(j)
    return sorted(r)


def _slots(groups):
    s = 1
    while s < Q_SLOTS and s < groups:
        s *= 2
    return s


def geometry(n, P, D, ld, probs=PROBS):
    """what demc_quantiles launches for n rows of P chains, D parameters in cells ld doubles apart -> dict(cells_per_chunk, busy_lanes
    (of Q_WG; the rest idle in the theta phase), chunks, workgroups, chunks_per_wg_max, ragged (the last chunk is not full), targets,
    first_pass_slots / later_slots (LDS tables a workgroup's groups can claim: the power of two that holds the groups there can be,
    at most Q_SLOTS), first_pass_direct (the least number of series that find no table in the first pass and are counted in the
    global one), passes)"""
    cells, D2 = n * P, D + 2
    cpi = Q_WG // min(ld, Q_WG)
    chunks = -(-cells // cpi)
    W = min(chunks, Q_MAX_WG)
    T = len(targets(cells, probs))
    assert T <= Q_MAX_TARGETS and -(-chunks // W) <= Q_MAX_CHUNKS_PER_WG
    return dict(cells_per_chunk=cpi, busy_lanes=cpi * min(ld, Q_WG), chunks=chunks, workgroups=W, chunks_per_wg_max=-(-chunks // W),
                ragged=cells % cpi != 0, targets=T, first_pass_slots=_slots(D2), later_slots=_slots(D2 * T),
                first_pass_direct=max(0, D2 - Q_SLOTS), passes=64 // Q_BITS)


def _root():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_constants_are_the_headers():
    import os
    import re
    from test_postplan_host import constants
    vals = constants()  # (as the compiler sees csrc/demc_postplan.hpp; geometry() and targets() are held to plan_quantiles there)
    want = dict(kQBits=Q_BITS, kQWG=Q_WG, kQMaxWG=Q_MAX_WG, kQSlots=Q_SLOTS, kQProbes=Q_PROBES, kQMaxTargets=Q_MAX_TARGETS, kQMaxChunksPerWG=Q_MAX_CHUNKS_PER_WG)
    for name, v in want.items():
        assert vals.get(name) == v, (name, vals.get(name), v)
    h = open(os.path.join(_root(), "include", "demc_quantile.h")).read()
    assert int(re.search(r"#define DEMC_QUANTILE_MAX_PROBS (\d+)", h).group(1)) * 2 == Q_MAX_TARGETS == vals["DEMC_QUANTILE_MAX_PROBS"] * 2
    assert vals["kQKeyNegInf"] == KEY_NEG_INF and vals["kQKeyPosInf"] == KEY_POS_INF and vals["kQPasses"] * Q_BITS == 64
    # the 32-bit counts: a workgroup counts at most chunks_per_wg_max * Q_WG values of a series per pass
    assert Q_MAX_CHUNKS_PER_WG * Q_WG <= 1 << 32 and 2 * Q_SLOTS * 257 * 4 <= 160 * 1024  # two workgroups per CU
    # ... and the rule, at the sizes DESIGN.md 5.6 names
    g = geometry(1000, 4096, 32, 32, DEFAULT)
    assert g["cells_per_chunk"] == 16 and g["workgroups"] == 512 and g["chunks_per_wg_max"] == 500 and g["targets"] == 10
    assert g["first_pass_slots"] == 64 and g["later_slots"] == 64 and g["first_pass_direct"] == 0
    assert geometry(1000, 24, 2, 2, DEFAULT)["first_pass_slots"] == 4 and geometry(1000, 24, 2, 2, DEFAULT)["later_slots"] == 64
    assert geometry(16, 8, 62, 62)["first_pass_slots"] == 64 and geometry(4, 4, 70, 70)["first_pass_direct"] == 8
    assert hist_ld(9, True) == 16 and hist_ld(9) == 9 and hist_ld(63, True) == 64 and hist_ld(17, True) == 32
    assert targets(1, DEFAULT) == [0] and targets(4, (0.5,)) == [1, 2] and targets(4, (0.0, 1.0)) == [0, 1, 2, 3]


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_known_answers_to_the_bit():
    got = restate(range(21), [0.1, 0.5, 0.9])
    assert got == [2.0, 10.0, 18.000000000000004] and bits(got[2]) == bits(18.000000000000004) != bits(18.0)
    assert restate([4, 1, 3, 2], [0.5, 0.025]) == [2.5, 1.075]
    assert restate([7.5], [0.0, 0.3, 1.0]) == [7.5] * 3 and bits(restate([-0.0], [0.5])[0]) == bits(-0.0)


def test_key_order_is_the_ieee_order_with_signed_zeros():
    xs = [-math.inf, -1e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e308, math.inf]
    ks = [key(x) for x in xs]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)
    assert key(-math.inf) == KEY_NEG_INF and key(math.inf) == KEY_POS_INF
    for x in xs:
        assert bits(unkey(key(x))) == bits(x)
    for nan_bits in (0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF):
        k = key(from_bits(nan_bits))
        assert k < KEY_NEG_INF or k > KEY_POS_INF
        assert (k < KEY_NEG_INF) == bool(nan_bits >> 63)


def random_pools():
    """pools with ties, signed zeros, infinities and subnormals"""
    rng = np.random.default_rng(56)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-310, -2.5e-310, np.inf, -np.inf, 1.0, -1.0, 1e308, -1e308])
    for N in (1, 2, 3, 4, 5, 7, 21, 64, 257, 1000):
        for kind in range(4):
            if kind == 0:
                x = rng.normal(0.0, 1.0, N)
            elif kind == 1:
                x = rng.integers(-3, 4, N).astype(np.float64)  # ties
            elif kind == 2:
                x = rng.choice(special, N)
            else:
                x = np.where(rng.uniform(size=N) < 0.3, rng.choice(special, N), rng.normal(0, 1e-3, N))
            yield (N, kind), x


def test_series_quantiles_equals_the_restatement_bit_for_bit(demc):
    probs = PROBS + (0.999, 0.5, 1e-9)
    for label, x in random_pools():
        got = demc.chains.series_quantiles(x, probs)
        want = restate(x.tolist(), probs)
        assert same_bits(got, want), (label, got, want)
    # pooled over chains: the shape of x does not matter, nor the order of its values
    x = np.random.default_rng(3).normal(size=(10, 6))
    assert same_bits(demc.chains.series_quantiles(x, DEFAULT), restate(x.T.reshape(-1).tolist(), DEFAULT))


def test_restatement_against_numpy_linear():
    """np.quantile(method="linear") takes the position as p (N - 1): a few ulp(N) |b - a| of difference are expected; the bar is
    1e-10 max|x| at N <= 1e5, that is 2 ulp(N) = 4.4e-11 times |b - a| <= 2 max|x|"""
    rng = np.random.default_rng(7)
    probs = list(DEFAULT) + [0.0, 1.0, 1.0 / 3.0, 0.1, 0.9]
    worst = 0.0
    for N in (2, 3, 10, 101, 1000, 4097, 99991):
        for scale in (1e-300, 1.0, 1e300):
            x = rng.normal(0.0, 1.0, N) * scale
            got, want = np.array(restate(x.tolist(), probs)), np.quantile(x, probs, method="linear")
            err = float(np.abs(got - want).max() / np.abs(x).max())
            worst = max(worst, err)
            assert err <= 1e-10, (N, scale, err)
    print(f"restatement against np.quantile(linear): max difference {worst:.3g} max|x|")


def test_nan_rule():
    for nan in (NAN, from_bits(0xFFF8000000000001), from_bits(0x7FF0000000000001)):
        out = restate([1.0, 2.0, nan, 3.0], PROBS)
        assert all(math.isnan(v) for v in out)
        assert all(math.isnan(v) for v in restate([nan], [0.5]))
    assert not any(math.isnan(v) for v in restate([1.0, 2.0, math.inf, -math.inf], PROBS))


def test_endpoints_with_infinities(demc):
    inf = math.inf
    assert restate([-inf, 1.0, 2.0, inf], [0.0, 1.0]) == [-inf, inf]
    pool = [-inf, -inf, -inf, -inf, 1.0, 2.0]
    # aleph = 6 p + (1 - p): up to p = 0.6 both neighbours are -inf; at 0.7 the interpolation meets -inf from the finite side; at
    # 0.8 aleph is 5 + 9e-16 in floating point, so a = 1, b = 2 and gamma is that excess
    got = restate(pool, [0.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0])
    assert got[:3] == [-inf, -inf, -inf] and got[3] == -inf and 1.0 <= got[4] < 1.0 + 1e-14 and 1.0 < got[5] < 2.0 and got[6] == 2.0
    assert not any(math.isnan(v) for v in got)
    # positions that are exact in floating point: N = 5, aleph = 4 p + 1
    got5 = restate([-inf, -inf, -inf, 1.0, 2.0], [0.5, 0.625, 0.75, 0.875])
    assert got5 == [-inf, -inf, 1.0, 1.5]  # gamma = 0 on -inf; (0.5)(-inf) + (0.5)(1); gamma = 0 on 1; 1 + 0.5 (2 - 1)
    # gamma == 0 next to an infinity: 0 * inf never happens
    assert restate([1.0, 2.0, inf], [0.5]) == [2.0] and restate([-inf, 1.0, 2.0], [0.5]) == [1.0]
    assert restate([1.0, inf, inf], [0.25]) == [inf]  # (0.5 * 1 + 0.5 * inf)
    assert math.isnan(restate([-inf, inf], [0.5])[0])  # 0.5 * -inf + 0.5 * inf: NaN by IEEE, as the definition says
    assert same_bits(demc.chains.series_quantiles(np.array(pool), [0.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]), got)
    assert same_bits(demc.chains.series_quantiles(np.array([-inf, inf]), [0.5, 0.0, 1.0]), restate([-inf, inf], [0.5, 0.0, 1.0]))


def test_chains_and_summary_quantile(demc):
    rng = np.random.default_rng(11)
    val = rng.normal(size=(50, 4, 6))
    ch = demc.Chains(val, ["a", "b", "acceptance", "lp"], ["a", "b"])
    assert demc.chains.DEFAULT_QUANTILES == DEFAULT
    q = ch.quantile()
    assert set(q) == {"a", "b"} and tuple(q["a"]) == DEFAULT
    for j, nm in enumerate(("a", "b")):
        assert same_bits(list(q[nm].values()), restate(val[:, j, :].reshape(-1).tolist(), DEFAULT))
    assert tuple(ch.quantile((0.5, 0.1))["b"]) == (0.5, 0.1)
    table = np.stack([demc.chains.series_quantiles(val[:, j, :], DEFAULT) for j in range(4)])
    s = demc.Summary(ch.names, np.zeros((4, 6)), quantiles=table, probs=DEFAULT)
    assert s.quantile() == q and s.probs == DEFAULT
    plain = demc.Summary(ch.names, np.zeros((4, 6)))
    assert plain.quantiles is None and plain.probs is None
    with pytest.raises(ValueError):
        plain.quantile()
    assert set(plain.describe()["a"]) == {"mean", "std", "rhat", "ess", "mcse", "pairs"}
    with pytest.raises(ValueError):
        demc.chains.series_quantiles(val[:, 0, :], (1.5,))


def test_summarize_with_an_injected_engine_falls_back_to_the_host(demc):
    """an engine that has summarize but no quantiles: the rows are exported and both tables come from the host functions"""
    calls = []

    class Eng:
        def __init__(self, **cfg):
            self.P, self.D, self.rows = cfg["n_groups"] * cfg["Np"], cfg["D"], cfg["n_rows"]
            self.rng = np.random.default_rng(1)
            self.full = np.concatenate([self.rng.normal(size=(self.rows, self.D, self.P)), np.zeros((self.rows, 1, self.P)),
                                        self.rng.normal(size=(self.rows, 1, self.P))], axis=1)

        def __getattr__(self, name):
            if name.startswith(("set_", "step", "close")):
                return lambda *a, **k: None
            raise AttributeError(name)

        def summarize(self, *a):
            calls.append("summarize")
            raise AssertionError("the device statistics were asked for although the quantiles cannot follow them")

        def export_chains(self, r0, r1):
            calls.append("export")
            return self.full[r0:r1]

        def get_state(self):
            return np.zeros((self.P, self.D)), np.zeros(self.P), np.arange(self.P)

    D = demc
    rng = np.random.default_rng(5)
    prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
    model = D.DEModel(sample_prior=prior, names=("mu", "sigma"), data=np.zeros(5), prior_loglike=D.Priors(mu=D.Normal(0, 1), sigma=D.TruncatedCauchy(0, 1)),
                      loglike=D.GaussianLikelihood())
    de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=10, Np=4)
    s = D.summarize(model, de, D.HIPBackend(seed=3), 30, quantiles=DEFAULT, engine_factory=Eng)
    assert calls == ["export"] and s.probs == DEFAULT and s.quantiles.shape == (4, 5)
    assert set(s.quantile()) == {"mu", "sigma"}


# ---- the header of the entry point, held to the library and to both bindings as test_summary_host.py holds demc_summary.h
def _quantile_prototypes():
    import os
    import re
    root = _root()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "demc_quantile.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return root, text, protos


def test_quantile_header_library_and_python_binding_agree(demc):
    import ctypes as C
    import subprocess
    root, text, protos = _quantile_prototypes()
    assert sorted(protos) == sorted(demc._ffi.QUANTILE_EXPORTS) == ["demc_quantiles"]
    assert not set(protos) & set(demc._ffi.EXPORTS), "declared in demc.h as well"
    assert not set(protos) & set(demc._ffi.SUMMARY_EXPORTS), "declared in demc_summary.h as well"
    lib = demc._ffi.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "constdouble*": C.POINTER(C.c_double),
             "demc_handle*": C.c_void_p}
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret]
        assert list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args], (name, args)
    assert demc._ffi.QUANTILE_MAX_PROBS == 16 and "#define DEMC_QUANTILE_MAX_PROBS 16" in text
    # the header is C99, and stands on demc.h alone
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", root + "/include", root + "/include/demc_quantile.h"])
    assert '#include "demc.h"' in text and "demc_summary.h" not in text


def test_quantile_ccall_matches_its_prototype():
    import os
    import re
    import test_julia_shim as J
    root, _, protos = _quantile_prototypes()
    main_jl = open(os.path.join(root, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPQuantile.jl")' in main_jl and "demc_quantiles" not in main_jl
    jl = open(os.path.join(root, "julia", "DEMCHIPQuantile.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= {"demc_quantiles"}
    main = J.c_prototypes()
    for m in calls:
        end = J.balanced(jl, m.end() - 1)
        jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
        if m.group(1) in protos:
            cret, ctypes_ = protos[m.group(1)]
            assert jtypes == [J.julia_type(c) for c in ctypes_], (jtypes, ctypes_)
            assert re.match(r"::([A-Za-z0-9{}]+)", jl[end:]).group(1) == J.julia_type(cret)
        elif m.group(1) in main:  # the calls of this file into demc.h itself, against demc.h
            assert jtypes == [J.julia_type(c) for c in main[m.group(1)][1]], (m.group(1), jtypes)
        else:  # demc_summarize: held to its header by test_summary_host.py's reading of DEMCHIPSummary.jl; here by name only
            assert m.group(1) == "demc_summarize", m.group(1)


def test_quantile_kernels_use_no_scratch(demc, tmp_path):
    """the k_q_* kernels keep everything in registers and LDS"""
    import os
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_q_" in k[0]]
    assert len(ks) == 5, [k[0] for k in ks]  # init, hist<first>, hist<later>, scan, final
    for name, regs, _, _, scratch in ks:
        assert scratch == 0 and regs <= 128, (name, regs, scratch)
