"""Posterior covariance and correlation (demc_covariance on the device, chains.series_cov on the host) against an
independent restatement of the definition -- explicit edge rules, sums in np.longdouble, nothing shared with chains.py -- plus the
launch geometry and the inputs the GPU tests of the same feature import (tests/test_gpu_cov.py).  No GPU here."""
import math
import os
import re

import numpy as np
import pytest

NAN = float("nan")
LD = np.longdouble


def restate(value, cols=None):
    """DESIGN.md 5.7 for value[n][series][chains], one pair of series after the other -> (mean[K], cov[K][K], cor[K][K], S[K][K]);
    the sums in np.longdouble, S rounded to double once, the last operations (division by N - 1; two square roots, a product and
    a division) in double as the definition has them.  The edge rules are applied as rules, not left to IEEE propagation."""
    value = np.asarray(value, dtype=np.float64)
    cols = list(range(value.shape[1])) if cols is None else list(cols)
    K = len(cols)
    x = [value[:, c, :].reshape(-1) for c in cols]
    N = x[0].size
    assert N >= 1 and K >= 1
    bad = [not np.isfinite(v).all() for v in x]
    mhat = [NAN if bad[j] else float(np.sum(x[j].astype(LD), dtype=LD) / LD(N)) for j in range(K)]  # a first mean, a double
    c = [None if bad[j] else x[j].astype(LD) - LD(mhat[j]) for j in range(K)]
    s = [None if bad[j] else np.sum(c[j], dtype=LD) for j in range(K)]
    mean = np.array([NAN if bad[j] else float(LD(mhat[j]) + s[j] / LD(N)) for j in range(K)])
    S = np.full((K, K), NAN)
    for i in range(K):
        for j in range(i, K):
            if bad[i] or bad[j]:
                continue
            Q = np.sum(c[i] * c[j], dtype=LD)
            S[i, j] = S[j, i] = float(Q - s[i] * s[j] / LD(N))
    cov, cor = np.full((K, K), NAN), np.full((K, K), NAN)
    if N == 1:
        return mean, cov, cor, S
    for i in range(K):
        for j in range(K):
            if bad[i] or bad[j]:
                continue
            cov[i, j] = S[i, j] / float(N - 1)
            if S[i, i] == 0.0 or S[j, j] == 0.0:  # a constant series: zeros in cov (S is zero there), NaN in cor
                assert S[i, j] == 0.0
                continue
            if i == j:
                cor[i, j] = 1.0
                continue
            a, b = min(i, j), max(i, j)
            r = S[a, b] / (math.sqrt(S[a, a]) * math.sqrt(S[b, b]))
            cor[i, j] = max(-1.0, min(1.0, r))
    return mean, cov, cor, S


def same_bits(a, b):
    """equal bit for bit, where a NaN equals any NaN (the NaN PATTERN is what is compared)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def scaled_errors(got, want, N):
    """(mean, cov, cor) against restate()'s (mean, cov, cor, S) -> the three figures the bars are set on: max |mean - mean_ref| /
    |mean_ref|, max |cov - cov_ref|_ij (N - 1) / (d_i d_j) with d = sqrt(diag S_ref), max |cor - cor_ref|; NaN patterns must agree"""
    mean, cov, cor = got
    rmean, rcov, rcor, S = want
    for a, b, what in ((mean, rmean, "mean"), (cov, rcov, "cov"), (cor, rcor, "cor")):
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"NaN pattern of {what}:\n{np.isnan(a).astype(int)}\n{np.isnan(b).astype(int)}"
    ok = ~np.isnan(rmean)
    e_mean = float(np.max(np.abs(mean[ok] - rmean[ok]) / np.maximum(np.abs(rmean[ok]), 1e-300), initial=0.0))
    d = np.sqrt(np.where(np.diag(S) > 0, np.diag(S), np.nan))
    scale = d[:, None] * d[None, :]
    okc = ~np.isnan(rcov) & ~np.isnan(scale)
    e_cov = float(np.max(np.abs(cov[okc] - rcov[okc]) * max(N - 1, 1) / scale[okc], initial=0.0))
    zero = ~np.isnan(rcov) & np.isnan(scale)  # rows and columns of constant series: exact zeros
    assert (cov[zero] == 0.0).all()
    okr = ~np.isnan(rcor)
    e_cor = float(np.max(np.abs(cor[okr] - rcor[okr]), initial=0.0))
    return e_mean, e_cov, e_cor


def kat(N, K, seed):
    """integer data whose column sums are divisible by N: value[N][K][1] -- every c, product and partial sum is an exact double in
    any order, so every correct implementation returns the same S, and cov / cor are the same few correctly rounded operations"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (N, K)).astype(np.int64)
    if N > 1:
        x[:, 1 % K] = x[:, 0] + rng.integers(-1, 2, N)  # (a correlated pair)
    x[-1] += (-x.sum(axis=0)) % N  # in [0, N): the sums are multiples of N
    x += 3 * (np.arange(K) % 5) - 6  # means that differ; the sums stay multiples of N
    assert (x.sum(axis=0) % N == 0).all() and np.abs(x).max() < 1 << 20
    return x.astype(np.float64).reshape(N, K, 1)


# ---- the launch geometry of the device code, restated: the kCov* constants and plan_cov's arithmetic (csrc/demc_postplan.hpp;
# tests/test_postplan_host.py holds this copy to the planner).  The GPU cases assert the geometry they were chosen for, so a changed
# constant fails them instead of moving them to another path.
COV_MAX_COLS, COV_WG, COV_CHUNK, COV_MAX_WORKERS, COV_FINAL_WG = 64, 512, 512, 512, 1024


def geometry(n, P, D, ld, K):
    """what demc_covariance launches for n rows of P chains (cells ld doubles apart) and K selected series -> dict(cells, blocks (of
    16 columns: the k_cov_syrk instance), tiles, ksteps (of 4 cells), ragged_kstep (the last holds fewer than 4), chunks, workers,
    chunks_per_worker_max, ragged_chunk, idle_waves (waves of the last chunk's workgroup without a k-step), partial (doubles a
    worker writes in pass 2), scratch_bytes)"""
    cells = n * P
    assert 1 <= K <= COV_MAX_COLS and K <= D + 2 and cells >= 1 and ld >= D
    nb = -(-K // 16)
    tiles = nb * (nb + 1) // 2
    ksteps = -(-cells // 4)
    chunks = -(-cells // COV_CHUNK)
    W = min(chunks, COV_MAX_WORKERS)
    last = -(-(cells - (chunks - 1) * COV_CHUNK) // 4)  # k-steps of the last chunk
    partial = tiles * 256 + nb * 16
    return dict(cells=cells, blocks=nb, tiles=tiles, ksteps=ksteps, ragged_kstep=cells % 4 != 0, chunks=chunks, workers=W,
                chunks_per_worker_max=-(-chunks // W), ragged_chunk=cells % COV_CHUNK != 0, idle_waves=max(0, COV_WG // 64 - last),
                partial=partial, scratch_bytes=8 * (W * (partial + COV_MAX_COLS) + COV_MAX_COLS + K + 2 * K * K) + 4 * COV_MAX_COLS)


def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_constants_are_the_headers():
    from test_postplan_host import constants
    # (as the compiler sees csrc/demc_postplan.hpp; geometry() itself is held to plan_cov there)
    vals = {name: v for name, v in constants().items() if name.startswith("kCov")}
    want = dict(kCovMaxCols=COV_MAX_COLS, kCovWG=COV_WG, kCovChunk=COV_CHUNK, kCovMaxWorkers=COV_MAX_WORKERS, kCovFinalWG=COV_FINAL_WG)
    assert vals == want, (vals, want)
    h = open(os.path.join(_root(), "include", "demc_cov.h")).read()
    assert int(re.search(r"#define DEMC_COV_MAX_COLS (\d+)", h).group(1)) == COV_MAX_COLS == constants()["DEMC_COV_MAX_COLS"]
    assert COV_CHUNK % (4 * (COV_WG // 64)) == 0  # every wave has the same number of k-steps in a full chunk
    # the LDS of k_cov_final: the totals of a worker's partial at K = 64 and the 64 x 64 triangle
    assert 8 * (geometry(1, 1, 62, 62, 64)["partial"] + 64 * 64) <= 64 * 1024
    # ... and the rule, at the sizes DESIGN.md 5.7 names
    g = geometry(1000, 4096, 32, 32, 34)
    assert g["blocks"] == 3 and g["tiles"] == 6 and g["chunks"] == 8000 and g["workers"] == 512 and g["chunks_per_worker_max"] == 16
    assert g["partial"] == 1584 and g["scratch_bytes"] < 8 << 20
    g = geometry(1000, 24, 2, 2, 4)
    assert g["blocks"] == 1 and g["tiles"] == 1 and g["chunks"] == 47 and g["workers"] == 47 and g["ragged_chunk"]
    assert geometry(1, 5, 2, 2, 4)["idle_waves"] == 6 and geometry(1, 5, 2, 2, 4)["ragged_kstep"]
    assert geometry(3, 4, 600, 600, 64)["tiles"] == 10 and geometry(1, 1, 2, 2, 1)["ksteps"] == 1


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def finite_cases():
    rng = np.random.default_rng(57)
    for n, K, P in ((1, 3, 2), (2, 2, 1), (5, 4, 3), (40, 6, 5), (250, 34, 4)):
        v = rng.normal(0.0, 1.0, (n, K, P)) * (1.0 + np.arange(K)[None, :, None])
        v[:, 0, :] = v[:, 0, :] * 3.0 - 4.5e6  # lp-like: a mean far from zero
        if K > 2:
            v[:, 2, :] = 0.9 * v[:, 1, :] / 2.0 + math.sqrt(1 - 0.81) * v[:, 2, :] / 3.0  # a 0.9-correlated pair
            v[:, K - 1, :] = (rng.uniform(size=(n, P)) < 0.3).astype(np.float64)  # acceptance-like
        yield (n, K, P), v


def test_series_cov_against_the_restatement(demc):
    worst = [0.0, 0.0, 0.0]
    for label, v in finite_cases():
        for cols in (None, [v.shape[1] - 1, 0], [1]):
            got = demc.chains.series_cov(v, cols)
            errs = scaled_errors(got, restate(v, cols), v.shape[0] * v.shape[2])
            worst = [max(a, b) for a, b in zip(worst, errs)]
            assert max(errs) <= 1e-12, (label, cols, errs)
            assert got[1].tobytes() == got[1].T.copy().tobytes() and got[2].tobytes() == got[2].T.copy().tobytes()
    print(f"series_cov against the restatement: mean {worst[0]:.3g}, cov {worst[1]:.3g} scaled, cor {worst[2]:.3g}")


def test_restatement_against_numpy():
    for label, v in finite_cases():
        n, K, P = label
        if n * P < 2:
            continue
        x = np.transpose(v, (0, 2, 1)).reshape(-1, K)  # [N][K]
        mean, cov, cor, S = restate(v)
        d = np.sqrt(np.diag(S))
        live = (d[:, None] * d[None, :]) > 0  # (an acceptance-like series of a tiny pool can be constant: zeros here, 0 / 0 in numpy)
        with np.errstate(all="ignore"):
            ncov, ncor = np.cov(x, rowvar=False), np.corrcoef(x, rowvar=False)
        assert np.max(np.abs(cov - ncov)[live] * (n * P - 1) / (d[:, None] * d[None, :])[live]) <= 1e-12, label
        assert np.max(np.abs(cor - ncor)[live]) <= 1e-12 and (cov[~live] == 0.0).all() and (ncov[~live] == 0.0).all(), label
        assert np.allclose(mean, x.mean(axis=0), rtol=1e-12, atol=0)


@pytest.mark.parametrize("N,K", [(24, 5), (24, 4), (24, 17), (24, 34), (24, 64), (2051, 8)])
def test_known_answers_to_the_bit(demc, N, K):
    v = kat(N, K, 100 + K)
    mean, cov, cor, S = restate(v)
    x = v[:, :, 0]
    m = x.sum(axis=0) / N
    assert (m == np.round(m)).all() and same_bits(mean, m)
    Sint = (x - m).T @ (x - m)  # integers: exact
    assert same_bits(S, Sint) and same_bits(cov, Sint / (N - 1))
    got = demc.chains.series_cov(v)
    assert same_bits(got[0], mean) and same_bits(got[1], cov) and same_bits(got[2], cor)
    assert abs(cor[0, 1]) > 0.5 and (np.diag(cor) == 1.0).all()
    # a chunked float64 two-pass with another first mean gives the same S: the corrected form does not depend on the shift
    shift = m + 0.5
    c = x - shift
    s = sum(c[k:k + 7].sum(axis=0) for k in range(0, N, 7))
    Q = sum(c[k:k + 7].T @ c[k:k + 7] for k in range(0, N, 7))
    assert same_bits(Q - np.outer(s, s) / N, Sint)


def test_nan_and_zero_rules(demc):
    rng = np.random.default_rng(8)
    base = rng.normal(0.0, 1.0, (16, 6, 4))
    base[:, 2, :] = 2.5  # a constant series
    for what, bad in (("nan", NAN), ("+inf", math.inf), ("-inf", -math.inf), ("both", None)):
        v = base.copy()
        v[5, 4, 3] = math.inf if bad is None else bad
        if bad is None:
            v[9, 4, 0] = -math.inf
        for fn in (lambda a: restate(a)[:3], demc.chains.series_cov):
            mean, cov, cor = fn(v)
            nanrow = np.zeros((6, 6), bool)
            nanrow[4, :] = nanrow[:, 4] = True
            assert np.array_equal(np.isnan(cov), nanrow), (what, np.isnan(cov).astype(int))
            const = nanrow.copy()
            const[2, :] = const[:, 2] = True
            assert np.array_equal(np.isnan(cor), const), (what, np.isnan(cor).astype(int))
            assert (cov[2, [0, 1, 2, 3, 5]] == 0.0).all() and (cov[[0, 1, 2, 3, 5], 2] == 0.0).all()
            assert math.isnan(mean[4]) and mean[2] == 2.5 and np.isfinite(mean[[0, 1, 3, 5]]).all()
            assert (np.diag(cor)[[0, 1, 3, 5]] == 1.0).all()
        assert max(scaled_errors(demc.chains.series_cov(v), restate(v), 64)) <= 1e-12
    one = base[:1, :, :1]  # N = 1
    for fn in (lambda a: restate(a)[:3], demc.chains.series_cov):
        mean, cov, cor = fn(one)
        assert np.isnan(cov).all() and np.isnan(cor).all() and same_bits(mean, one[0, :, 0])


# ---- the host surface ---------------------------------------------------------------------------------------------------------------
def test_chains_and_summary_cov(demc):
    rng = np.random.default_rng(11)
    val = rng.normal(size=(50, 4, 6))
    val[:, 1, :] += 0.8 * val[:, 0, :]
    ch = demc.Chains(val, ["a", "b", "acceptance", "lp"], ["a", "b"])
    names, cov = ch.cov()
    names2, cor = ch.cor()
    assert names == names2 == ["a", "b"] and cov.shape == cor.shape == (2, 2)
    _, rcov, rcor, _ = restate(val, [0, 1])
    assert np.allclose(cov, rcov, rtol=1e-12, atol=0) and np.allclose(cor, rcor, rtol=1e-12, atol=0) and cor[0, 1] > 0.4
    names, cor3 = ch.cor(("lp", "a"))
    assert names == ["lp", "a"] and np.allclose(cor3, restate(val, [3, 0])[2], rtol=1e-12, atol=1e-15)
    s = demc.Summary(ch.names, np.zeros((4, 6)), cov=cov, cor=cor, cov_names=["a", "b"])
    assert s.cov()[0] == ["a", "b"] and s.cov()[1].tobytes() == cov.tobytes() and s.cor()[1].tobytes() == cor.tobytes()
    plain = demc.Summary(ch.names, np.zeros((4, 6)))
    assert plain.cov_matrix is None and plain.cor_matrix is None and plain.cov_names is None
    for f in (plain.cov, plain.cor):
        with pytest.raises(ValueError):
            f()
    for bad in ([], [0, 0], [4], [-1]):
        with pytest.raises(ValueError):
            demc.chains.series_cov(val, bad)


def test_summarize_with_an_injected_engine_falls_back_to_the_host(demc):
    """an engine that has summarize and quantiles but no covariance: the rows are exported and every table comes from the host"""
    calls = []

    class Eng:
        def __init__(self, **cfg):
            self.P, self.D, self.rows = cfg["n_groups"] * cfg["Np"], cfg["D"], cfg["n_rows"]
            rng = np.random.default_rng(1)
            self.full = np.concatenate([rng.normal(size=(self.rows, self.D, self.P)), (rng.uniform(size=(self.rows, 1, self.P)) < 0.5) * 1.0,
                                        rng.normal(size=(self.rows, 1, self.P))], axis=1)

        def __getattr__(self, name):
            if name.startswith(("set_", "step", "close")):
                return lambda *a, **k: None
            raise AttributeError(name)

        def summarize(self, *a):
            raise AssertionError("the device statistics were asked for although the covariance cannot follow them")

        def quantiles(self, *a):
            raise AssertionError("the device quantiles were asked for although the covariance cannot follow them")

        def export_chains(self, r0, r1):
            calls.append("export")
            return self.full[r0:r1]

        def get_state(self):
            return np.zeros((self.P, self.D)), np.zeros(self.P), np.arange(self.P)

    D = demc

    def run(**kw):
        rng = np.random.default_rng(5)
        prior = lambda: [rng.normal(0, 1), abs(rng.standard_cauchy())]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("mu", "sigma"), data=np.zeros(5),
                          prior_loglike=D.Priors(mu=D.Normal(0, 1), sigma=D.TruncatedCauchy(0, 1)), loglike=D.GaussianLikelihood())
        de = D.DE(sample_prior=prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=10, Np=4)
        return D.summarize(model, de, D.HIPBackend(seed=3), 30, engine_factory=Eng, **kw), de

    s, de = run(cor=True)
    assert calls == ["export"] and s.cor()[0] == ["mu", "sigma"] and s.cov()[1].shape == (2, 2) and s.quantiles is None
    kept = Eng(n_groups=de.n_groups, Np=4, D=2, n_rows=30).full[10:30]
    assert s.cor()[1].tobytes() == D.chains.series_cov(kept, [0, 1])[2].tobytes()
    s, _ = run(cor=("lp", "mu", "acceptance"), quantiles=(0.5,))
    assert s.cor()[0] == ["lp", "mu", "acceptance"] and s.cor()[1].shape == (3, 3) and s.quantiles.shape == (4, 1)
    assert s.cov()[1].tobytes() == D.chains.series_cov(kept, [3, 0, 2])[1].tobytes()
    with pytest.raises(ValueError):
        run(cor=("nu",))
    with pytest.raises(ValueError):
        run(cor=("mu", "mu"))


# ---- the header of the entry point, held to the library and to both bindings as test_quantile_host.py holds demc_quantile.h
def _cov_prototypes():
    root = _root()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "demc_cov.h")).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"((?:const\s+)?[a-z_0-9]+\s*\**)\s*\b(demc_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", text):
        protos[name] = (ret.strip(), [re.match(r"(.*?[\s\*])([A-Za-z_0-9]+)$", a.strip()).group(1).strip() for a in args.split(",")])
    return root, text, protos


def test_cov_header_library_and_python_binding_agree(demc):
    import ctypes as C
    import subprocess
    root, text, protos = _cov_prototypes()
    assert sorted(protos) == sorted(demc._ffi.COV_EXPORTS) == ["demc_covariance"]
    for other in (demc._ffi.EXPORTS, demc._ffi.SUMMARY_EXPORTS, demc._ffi.QUANTILE_EXPORTS):
        assert not set(protos) & set(other), "declared in another header as well"
    assert "demc_covariance" not in open(os.path.join(root, "include", "demc.h")).read()
    lib = demc._ffi.load()
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double*": C.POINTER(C.c_double), "constdouble*": C.POINTER(C.c_double),
             "constint32_t*": C.POINTER(C.c_int32), "demc_handle*": C.c_void_p}
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is ctype[ret]
        assert list(fn.argtypes) == [ctype[a.replace(" ", "")] for a in args], (name, args)
    assert len(protos["demc_covariance"][1]) == 8
    assert demc._ffi.COV_MAX_COLS == demc.chains.COV_MAX_COLS == 64 and "#define DEMC_COV_MAX_COLS 64" in text
    assert callable(getattr(demc._ffi.HipEngine, "covariance"))
    # the header is C99, and stands on demc.h alone
    subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", "-I", root + "/include", root + "/include/demc_cov.h"])
    assert '#include "demc.h"' in text and "demc_summary.h" not in text and "demc_quantile.h" not in text


def test_cov_ccall_matches_its_prototype():
    import test_julia_shim as J
    root, _, protos = _cov_prototypes()
    main_jl = open(os.path.join(root, "julia", "DEMCHIP.jl")).read()
    assert 'include("DEMCHIPCov.jl")' in main_jl and "demc_covariance" not in main_jl and "demc_quantiles" not in main_jl
    jl = open(os.path.join(root, "julia", "DEMCHIPCov.jl")).read()
    calls = list(re.finditer(r"@ccall LIB\.(demc_[a-z_0-9]+)\(", jl))
    assert {m.group(1) for m in calls} >= {"demc_covariance"}
    main = J.c_prototypes()
    for m in calls:
        end = J.balanced(jl, m.end() - 1)
        jtypes = [a[a.rindex("::") + 2:].strip() for a in J.split_top(jl[m.end():end - 1])]
        if m.group(1) in protos:
            cret, ctypes_ = protos[m.group(1)]
            assert jtypes == [J.julia_type(c) for c in ctypes_], (jtypes, ctypes_)
            assert re.match(r"::([A-Za-z0-9{}]+)", jl[end:]).group(1) == J.julia_type(cret)
        else:  # the calls of this file into demc.h itself, against demc.h
            assert m.group(1) in main, m.group(1)
            assert jtypes == [J.julia_type(c) for c in main[m.group(1)][1]], (m.group(1), jtypes)


def test_cov_kernels_use_no_scratch(demc, tmp_path):
    """the k_cov_* kernels keep everything in registers and LDS, within the registers their workgroups can be given"""
    from test_abi import kernel_descriptors
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_cov_" in k[0]]
    assert len(ks) == 7, [k[0] for k in ks]  # mean, mean_final, syrk<1..4>, final
    assert sum("k_cov_syrk" in k[0] for k in ks) == 4
    for name, regs, _, wg, scratch in ks:
        assert scratch == 0 and regs <= 512 // -(-wg // 256), (name, regs, wg, scratch)
