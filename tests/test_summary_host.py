"""Chain summaries (demc_summarize on the device, Chains.summarystats on the host) against an independent
restatement of the definition in plain loops -- nothing below is shared with chains.py -- plus the deterministic inputs the GPU
tests of the same feature import (tests/test_gpu_summary.py).  No GPU here."""
import math

import numpy as np
import pytest

LAG_BLOCK = 64  # the device evaluates lags in blocks of this many (include/demc_summary.h)
NAN = float("nan")


def restate(x, max_lag=0, rho_len=0):
    """DESIGN.md 5.5 for one series x[n][m], one operation after the other -> dict(mean, std, rhat, ess, mcse, pairs, rho, pmin):
    rho[t] for the lags a call evaluates (whole blocks of LAG_BLOCK lags up to the block in which Geyer's sequence ends, never
    past L), NaN beyond; pmin = min |P_k| over the pairs that were looked at (None if there were none)."""
    x = [[float(v) for v in row] for row in np.asarray(x, dtype=np.float64)]
    n, m = len(x), len(x[0])
    tot = 0.0
    for i in range(n):
        for c in range(m):
            tot += x[i][c]
    mean = tot / (n * m)
    ss = 0.0
    for i in range(n):
        for c in range(m):
            ss += (x[i][c] - mean) ** 2
    std = math.sqrt(ss / (n * m - 1)) if n * m > 1 and ss == ss else NAN
    out = dict(mean=mean, std=std, rhat=NAN, ess=NAN, mcse=NAN, pairs=0.0, rho=[NAN] * rho_len, pmin=None)
    h = n // 2
    if h < 2:
        return out
    M = 2 * m
    chains = [[x[s * h + i][c] for i in range(h)] for c in range(m) for s in (0, 1)]  # split chain 2c + s
    mus = [sum(ch) / h for ch in chains]
    ys = [[v - mu for v in ch] for ch, mu in zip(chains, mus)]

    def gamma_mean(t):
        g = 0.0
        for y in ys:
            a = 0.0
            for i in range(h - t):
                a += y[i] * y[i + t]
            g += a / h
        return g / M

    W = gamma_mean(0) * h / (h - 1)
    mubar = sum(mus) / M
    bh = sum((mu - mubar) ** 2 for mu in mus) / (M - 1)
    vplus = W * (h - 1) / h + bh
    L = min(h - 1, max_lag) if max_lag > 0 else h - 1
    cache = {}

    def rho(t):
        if t not in cache:
            if t == 0:
                cache[t] = 1.0
            elif vplus == 0:  # W = 0 and B = 0: every gamma is 0 and rho is 0 / 0, a NaN by IEEE (Python would raise)
                cache[t] = NAN
            else:
                cache[t] = 1.0 - (W - gamma_mean(t)) / vplus
        return cache[t]

    def fill(b_last):
        for t in range(min(rho_len, L + 1, LAG_BLOCK * (b_last + 1))):
            out["rho"][t] = rho(t)

    if W == 0:
        fill(0)
        return out
    out["rhat"] = math.sqrt(vplus / W) if W == W else NAN
    if h < 4:
        fill(0)
        return out
    K, total, prev, b_last, bad, pmin = 0, 0.0, None, L // LAG_BLOCK, False, None
    while 2 * K + 1 <= L:
        P = rho(2 * K) + rho(2 * K + 1)
        if P == P:
            pmin = abs(P) if pmin is None else min(pmin, abs(P))
        if not P >= 0:
            bad = P != P
            b_last = (2 * K) // LAG_BLOCK
            break
        if prev is not None:
            P = min(P, prev)
        total += P
        prev = P
        K += 1
    fill(b_last)
    tau = max(-1.0 + 2.0 * total, 1.0 / math.log10(M * h))
    out["pairs"] = float(K)
    out["pmin"] = pmin
    if not bad:
        out["ess"] = M * h / tau
        out["mcse"] = std / math.sqrt(out["ess"])
    return out


def restate_all(value, max_lag=0, rho_len=0):
    """value[n][series][m] (the Chains value array) -> one restate() per series"""
    return [restate(value[:, j, :], max_lag, rho_len) for j in range(value.shape[1])]


def restate_np(x, max_lag=0, rho_len=0):
    """the definition restate() states, once more: every chain at a time with numpy, in np.longdouble, for the sizes at which plain
    loops take minutes.  Same dict, same pmin, same rule for which rho[t] are filled; nothing is shared with chains.py.  The CPU
    test below holds it to restate() at rtol 1e-12."""
    LD = np.longdouble
    with np.errstate(all="ignore"):  # (inf - inf and 0 / 0 are NaNs by IEEE, which is what the definition asks for)
        x = np.asarray(x, dtype=np.float64).astype(LD)
        n, m = x.shape
        mean = x.sum() / LD(n * m)
        ss = np.square(x - mean).sum()
        std = np.sqrt(ss / LD(n * m - 1)) if n * m > 1 and ss == ss else LD(NAN)
        out = dict(mean=float(mean), std=float(std), rhat=NAN, ess=NAN, mcse=NAN, pairs=0.0, rho=[NAN] * rho_len, pmin=None)
        h = n // 2
        if h < 2:
            return out
        M = 2 * m
        s = x[:2 * h].reshape(2, h, m).transpose(1, 0, 2).reshape(h, M)  # a column per split chain (their order does not matter)
        mu = s.sum(axis=0) / LD(h)
        y = s - mu

        def gamma_mean(t):
            return ((y[:h - t] * y[t:]).sum(axis=0) / LD(h)).sum() / LD(M)

        W = gamma_mean(0) * LD(h) / LD(h - 1)
        bh = np.square(mu - mu.sum() / LD(M)).sum() / LD(M - 1)
        vplus = W * LD(h - 1) / LD(h) + bh
        L = min(h - 1, max_lag) if max_lag > 0 else h - 1
        cache = {}

        def rho(t):
            if t not in cache:
                cache[t] = LD(1.0) if t == 0 else (LD(NAN) if vplus == 0 else LD(1.0) - (W - gamma_mean(t)) / vplus)
            return cache[t]

        def fill(b_last):
            for t in range(min(rho_len, L + 1, LAG_BLOCK * (b_last + 1))):
                out["rho"][t] = float(rho(t))

        if W == 0:
            fill(0)
            return out
        out["rhat"] = float(np.sqrt(vplus / W)) if W == W else NAN
        if h < 4:
            fill(0)
            return out
        K, total, prev, b_last, bad, pmin = 0, LD(0.0), None, L // LAG_BLOCK, False, None
        while 2 * K + 1 <= L:
            P = rho(2 * K) + rho(2 * K + 1)
            if P == P:
                pmin = abs(P) if pmin is None else min(pmin, abs(P))
            if not P >= 0:
                bad = bool(P != P)
                b_last = (2 * K) // LAG_BLOCK
                break
            if prev is not None and prev < P:
                P = prev
            total += P
            prev = P
            K += 1
        fill(b_last)
        tau = max(LD(-1.0) + LD(2.0) * total, LD(1.0) / np.log10(LD(M * h)))
        out["pairs"] = float(K)
        out["pmin"] = None if pmin is None else float(pmin)
        if not bad:
            ess = LD(M * h) / tau
            out["ess"] = float(ess)
            out["mcse"] = float(std / np.sqrt(ess))
        return out


# ---- the launch geometry of the device code, restated: the kSum* constants and plan_summary's arithmetic (csrc/demc_postplan.hpp;
# tests/test_postplan_host.py holds this copy to the planner).  The GPU cases assert the geometry they were chosen for, so a changed
# constant fails them instead of moving them to another path.
SUM_LAG_BLOCK, SUM_MAX_JT, SUM_MAX_WORKERS = 64, 8, 1024
SUM_LDS_SMALL, SUM_LDS_MAX, SUM_GLOBAL_TILE = 64 * 1024, 144 * 1024, 64 << 20


def geometry(n, P, D):
    """what demc_summarize launches for n rows of P chains and D parameters (max_lag = 0) -> dict(mode: "lds64" | "lds144" |
    "global", JT: series per tile, tiles: the width of every series tile, workers, chains_per_worker_max, lag_blocks)"""
    D2, h = D + 2, n // 2
    per_series = (n + 2 * SUM_LAG_BLOCK) * 8
    workers = min(P, SUM_MAX_WORKERS)
    if per_series <= SUM_LDS_SMALL:
        mode, JT = "lds64", min(D2, SUM_MAX_JT, SUM_LDS_SMALL // per_series)
    elif per_series <= SUM_LDS_MAX:
        mode, JT = "lds144", 1
    else:
        mode, JT = "global", 1
        workers = max(1, min(workers, SUM_GLOBAL_TILE // (n * D2 * 8)))
    return dict(mode=mode, JT=JT, tiles=[min(JT, D2 - j0) for j0 in range(0, D2, JT)], workers=workers,
                chains_per_worker_max=-(-P // workers), lag_blocks=(h - 1) // SUM_LAG_BLOCK + 1 if h >= 2 else 0)


# ---- the deterministic inputs of the GPU tests: x_0 = e_0, x_i = phi x_{i-1} + e_i, shifted by 100 (|mean| / sd <= 100)
AR1_CASES = [(64, 4, 0.0), (65, 4, 0.9), (129, 3, -0.5), (200, 8, 0.5), (1000, 16, 0.95)]
# the inputs of the GPU cases that leave the smallest launch geometry (a list of its own: plain loops run over AR1_CASES), with
# the lag caps each is summarised under and the number of series that are scaled (below)
AR1_LARGE = [(16, 1024, 0.5), (16, 1025, 0.5), (130, 1025, 0.9), (130, 4096, 0.9), (2000, 8, 0.5), (3900, 8, 0.5), (18305, 64, 0.5),
             (16, 8, 0.5)]
LARGE_MAX_LAGS = {(1000, 16, 0.95): (63, 64, 65, 127, 128)}
LARGE_SCALED = {(16, 1025, 0.5): 7, (130, 1025, 0.9): 7, (130, 4096, 0.9): 7, (18305, 64, 0.5): 6, (16, 8, 0.5): 70}
SEEDS = (0, 1, 2)
MARGIN = 1e-6  # an error of 1e-12 in rho cannot flip a pair that is this far from zero


def ar1(n, m, phi, seed):
    e = np.random.default_rng(seed).normal(size=(n, m))
    x = np.empty((n, m))
    x[0] = e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    return x + 100.0


def scaled(x, j):
    """series j of a case with more than three parameters: two series fed by the same seed still differ in mean and std"""
    return x * (1.0 + j / 8.0)


def nonfinite_inputs():
    """a chain that never left the outside of the bounds (lp = -inf throughout), one such cell, one NaN cell"""
    a, b, c = (ar1(40, 8, 0.5, 0) for _ in range(3))
    a[:, 0:4] = -np.inf
    b[3, 2] = -np.inf
    c[3, 2] = np.nan
    return [(("-inf chains",), a), (("-inf cell",), b), (("nan cell",), c)]


def _pairs_numpy(x, max_lag=0):
    """the pairs Geyer's sequence looks at, with numpy (the margin condition at sizes plain loops are too slow for)"""
    n, m = x.shape
    h = n // 2
    s = np.concatenate([x[:h], x[h:2 * h]], axis=1)
    y = s - s.mean(axis=0)
    W = (y * y).sum(axis=0).mean() / h * h / (h - 1)
    vplus = W * (h - 1) / h + s.mean(axis=0).var(ddof=1)
    L = min(h - 1, max_lag) if max_lag > 0 else h - 1
    rho = lambda t: 1.0 if t == 0 else 1.0 - (W - ((y[:h - t] * y[t:]).sum(axis=0) / h).mean()) / vplus
    out, k = [], 0
    while 2 * k + 1 <= L:
        out.append(rho(2 * k) + rho(2 * k + 1))
        if out[-1] < 0:
            break
        k += 1
    return out


def test_known_answer():
    x = np.array([1, -1, 1, -1, 1, -1, 1, -1], dtype=np.float64).reshape(8, 1)
    r = restate(x, rho_len=4)
    assert r["mean"] == 0.0
    assert abs(r["rhat"] - math.sqrt(3) / 2) <= 1e-15
    assert abs(r["rho"][1] - (-13 / 12)) <= 1e-15 and r["rho"][0] == 1.0
    assert r["pairs"] == 0.0
    assert abs(r["ess"] - 8 * math.log10(8)) <= 1e-15 * 8
    assert abs(r["std"] - math.sqrt(8 / 7)) <= 1e-15
    assert abs(r["mcse"] - r["std"] / math.sqrt(r["ess"])) <= 1e-15


def _small_inputs(cases=AR1_CASES[:4]):
    for n, m, phi in cases:
        for seed in SEEDS:
            yield (n, m, phi, seed), ar1(n, m, phi, seed)


def test_restatement_rhat_equals_chains_rhat(demc):
    for key, x in _small_inputs(AR1_CASES):
        a, b = restate(x, max_lag=1)["rhat"], demc.Chains._rhat(x)
        assert abs(a - b) <= 1e-15 * abs(b), (key, a, b)
    for n in (1, 2, 3):
        assert math.isnan(restate(ar1(n, 2, 0.0, 0))["rhat"]) and math.isnan(demc.Chains._rhat(ar1(n, 2, 0.0, 0)))


def _close(a, b, rtol):
    return a == b or (math.isnan(a) and math.isnan(b)) or abs(a - b) <= rtol * abs(b)


@pytest.mark.parametrize("max_lag", [0, 5, 16])
def test_summarystats_equals_the_restatement(demc, max_lag):
    cases = list(_small_inputs()) + [(("edge", n), ar1(n, 3, 0.5, 7)) for n in (1, 2, 3, 7, 8, 9)]
    cases.append((("const",), np.full((40, 3), 2.5)))
    cases += nonfinite_inputs()
    for key, x in cases:
        val = np.stack([x, 2.0 - x], axis=1)  # two series
        ch = demc.Chains(val, ["a", "b"], ["a", "b"], internals=())
        s = ch.summarystats(max_lag=max_lag, rho_len=70)
        for j, nm in enumerate(("a", "b")):
            r = restate(val[:, j, :], max_lag, 70)
            got = s[nm]
            for col in ("mean", "std", "rhat", "ess", "mcse"):
                assert _close(got[col], r[col], 1e-12), (key, nm, col, got[col], r[col])
            assert got["pairs"] == r["pairs"], (key, nm)
            ref = np.array(r["rho"])
            assert np.array_equal(np.isnan(s.rho[j]), np.isnan(ref)), (key, nm)
            np.testing.assert_allclose(s.rho[j], ref, rtol=0, atol=1e-12)
        d = s.describe()
        assert set(d["a"]) == {"mean", "std", "rhat", "ess", "mcse", "pairs"}
    c = restate(np.full((40, 3), 2.5))
    assert c["std"] == 0.0 and math.isnan(c["rhat"]) and math.isnan(c["ess"]) and math.isnan(c["mcse"])


@pytest.mark.parametrize("max_lag", [0, 5, 16])
def test_vectorised_restatement_equals_the_plain_loops(max_lag):
    """restate_np (the reference of the large GPU cases) against restate: numbers to rtol 1e-12, the bar between two host forms
    above; `pairs` and the NaN pattern of every column and of rho exactly"""
    cases = list(_small_inputs()) + [(("edge", n), ar1(n, 3, 0.5, 7)) for n in (1, 2, 3, 7, 8, 9)]
    cases.append((("const",), np.full((40, 3), 2.5)))
    cases += nonfinite_inputs()
    worst = 0.0
    for key, x in cases:
        a, b = restate_np(x, max_lag, 70), restate(x, max_lag, 70)
        assert set(a) == set(b)
        for col in ("mean", "std", "rhat", "ess", "mcse"):
            assert type(a[col]) is float and math.isnan(a[col]) == math.isnan(b[col]), (key, col, a[col], b[col])
            assert _close(a[col], b[col], 1e-12), (key, col, a[col], b[col])
            if math.isfinite(b[col]) and b[col] != 0:
                worst = max(worst, abs(a[col] - b[col]) / abs(b[col]))
        assert a["pairs"] == b["pairs"], key
        assert (a["pmin"] is None) == (b["pmin"] is None) and (b["pmin"] is None or _close(a["pmin"], b["pmin"], 1e-9)), key
        ra, rb = np.array(a["rho"]), np.array(b["rho"])
        assert np.array_equal(np.isnan(ra), np.isnan(rb)), (key, ra, rb)
        np.testing.assert_allclose(ra, rb, rtol=1e-12, atol=1e-12)
    print(f"restate_np against restate, max_lag={max_lag}: max relative difference {worst:.3g}")
    for key, x in nonfinite_inputs():  # what the definition gives for them, said once
        r = restate_np(x, max_lag, 70)
        assert (math.isnan(r["mean"]) if key == ("nan cell",) else r["mean"] == -math.inf), key
        assert all(math.isnan(r[col]) for col in ("std", "rhat", "ess", "mcse")) and r["pairs"] == 0.0 and r["pmin"] is None, key
        assert r["rho"][0] == 1.0 and np.isnan(r["rho"][1:]).all() and restate(x, max_lag, 70)["rho"][0] == 1.0, key


def test_geometry_constants_are_the_headers():
    from test_postplan_host import constants
    c = constants()  # (as the compiler sees csrc/demc_postplan.hpp; geometry() itself is held to plan_summary there)
    want = dict(kSumLagBlock=SUM_LAG_BLOCK, kSumMaxJT=SUM_MAX_JT, kSumMaxWorkers=SUM_MAX_WORKERS, kSumLdsSmall=SUM_LDS_SMALL,
                kSumLdsMax=SUM_LDS_MAX, kSumGlobalTile=SUM_GLOBAL_TILE)
    for name, v in want.items():
        assert c[name] == v, (name, c.get(name), v)
    assert LAG_BLOCK == SUM_LAG_BLOCK
    # ... and the rule, at the sizes the header's comments and DESIGN.md 5.5 name
    assert [geometry(n, 4, 1)["mode"] for n in (8064, 8065, 18304, 18305)] == ["lds64", "lds144", "lds144", "global"]
    assert geometry(200, 8, 2) == dict(mode="lds64", JT=4, tiles=[4], workers=8, chains_per_worker_max=1, lag_blocks=2)
    assert geometry(1000, 4096, 32)["JT"] == 7 and geometry(1000, 4096, 32)["tiles"] == [7, 7, 7, 7, 6]
    assert geometry(1000, 4096, 32)["workers"] == 1024 and geometry(1000, 4096, 32)["chains_per_worker_max"] == 4
    assert geometry(1, 3, 1)["lag_blocks"] == 0 and geometry(130, 3, 1)["lag_blocks"] == 2 and geometry(128, 3, 1)["lag_blocks"] == 1


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_ess_of_ar1_has_the_textbook_value(demc, phi):
    """sign and index conventions: ess / (n m) of AR(1) is (1 - phi) / (1 + phi)"""
    n, m = 20000, 4
    x = ar1(n, m, phi, 11)
    s = demc.Chains(x[:, None, :], ["x"], ["x"], internals=()).summarystats()["x"]
    want = (1 - phi) / (1 + phi)
    assert abs(s["ess"] / (n * m) / want - 1) <= 0.15, (phi, s["ess"] / (n * m), want)


def test_no_synthetic_input_sits_on_a_zero_pair():
    """A condition on the inputs of the GPU tests, not a measurement: near a zero pair an error of 1e-12 in rho flips K and ess
    jumps.  Every case and seed is held to it -- a seed that fails is replaced, never skipped."""
    worst = math.inf
    for n, m, phi in AR1_CASES:
        for seed in SEEDS:
            for max_lag in (0, 16):
                ps = _pairs_numpy(ar1(n, m, phi, seed), max_lag)
                assert ps, (n, m, phi, seed)
                worst = min(worst, min(abs(p) for p in ps))
                assert min(abs(p) for p in ps) >= MARGIN, (n, m, phi, seed, max_lag)
    print(f"smallest |P_k| over the synthetic inputs: {worst:.3g}")
    # the inputs of the large GPU cases: the new lag caps on the slow-mixing case, max_lag = 0 on the others -- each as it is and
    # with the factors its series are scaled by
    for key in list(LARGE_MAX_LAGS) + AR1_LARGE:
        worst = math.inf
        for seed in SEEDS:
            x = ar1(*key, seed)
            for max_lag in LARGE_MAX_LAGS.get(key, (0,)):
                for j in {0} | set(range(seed, LARGE_SCALED.get(key, 0), len(SEEDS))):  # series j is fed seed j % 3
                    ps = _pairs_numpy(scaled(x, j), max_lag)
                    assert ps, (key, seed)
                    worst = min(worst, min(abs(p) for p in ps))
                    assert min(abs(p) for p in ps) >= MARGIN, (key, seed, max_lag, j)
        print(f"smallest |P_k| of {key}: {worst:.3g}")
    # ... and the numpy form used here names the same pairs as the restatement
    x = ar1(*AR1_CASES[1], 0)
    r = restate(x)
    ps = _pairs_numpy(x)
    assert len(ps) == int(r["pairs"]) + (1 if ps[-1] < 0 else 0) and abs(min(abs(p) for p in ps) - r["pmin"]) <= 1e-12


def test_new_kernels_use_no_scratch(demc, tmp_path):
    """the chain-summary kernels keep everything in registers and LDS"""
    import os
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_sum_" in k[0]]
    assert len(ks) == 10, [k[0] for k in ks]
    for name, regs, _, _, scratch in ks:
        assert scratch == 0 and regs <= 128, (name, regs, scratch)


# ---- the header of the entry point, held to the library and to both bindings as test_abi.py / test_julia_shim.py hold demc.h
def _summary_prototypes():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "demc_summary.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return root, text, protos


def test_summary_header_library_and_python_binding_agree(demc):
    import ctypes as C
    import re
    import subprocess
    root, text, protos = _summary_prototypes()
    assert sorted(protos) == sorted(demc._ffi.SUMMARY_EXPORTS) == ["demc_summarize"]
    assert not set(protos) & set(demc._ffi.EXPORTS), "declared in demc.h as well"
    lib = demc._ffi.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "demc_handle*": C.c_void_p}
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret]
        assert list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args], (name, args)
    assert int(re.search(r"#define DEMC_SUMMARY_COLS (\d+)", text).group(1)) == len(demc.chains.SUMMARY_COLS) == 6
    # the header is C, and stands on demc.h alone
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", root + "/include", root + "/include/demc_summary.h"])


def test_summary_ccall_matches_its_prototype():
    import os
    import re
    import test_julia_shim as J
    root, _, protos = _summary_prototypes()
    assert 'include("DEMCHIPSummary.jl")' in open(os.path.join(root, "julia", "DEMCHIP.jl")).read()
    jl = open(os.path.join(root, "julia", "DEMCHIPSummary.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= {"demc_summarize"}
    for m in calls:
        if m.group(1) not in protos:
            continue  # (demc.h's functions: DEMCHIP.jl's own calls are held to it by test_julia_shim.py, these by hand below)
        end = J.balanced(jl, m.end() - 1)
        jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
        cret, ctypes_ = protos[m.group(1)]
        assert jtypes == [J.julia_type(c) for c in ctypes_], (jtypes, ctypes_)
        assert re.match(r"::([A-Za-z0-9{}]+)", jl[end:]).group(1) == J.julia_type(cret)
    # the calls of this file into demc.h itself, against demc.h
    main = J.c_prototypes()
    for m in calls:
        if m.group(1) in main:
            end = J.balanced(jl, m.end() - 1)
            jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
            assert jtypes == [J.julia_type(c) for c in main[m.group(1)][1]], (m.group(1), jtypes)
