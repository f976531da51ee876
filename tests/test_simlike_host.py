"""Simulation-based likelihoods (include/demc.h: demc_set_model_sim) without a GPU: the numpy restatement of the estimator that
tests/test_gpu_simlike.py holds the kernel to, checked against itself; the Python surface; the code objects of k_sim_loglike.

The restatement regenerates the draws with a vectorised Philox4x32-10 that is itself compared with the oracle's (`oracle.philox`,
counter layout of draw_block: (block, entity, iteration, stream << 24 | sweep), key = seed)."""
import math
import os
import re

import numpy as np
import pytest

S_SIM, S_PART = 7, 3
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
def philox_np(ctr, seed):
    """Philox4x32-10 of counters [n][4] (uint32) under key = (seed lo, seed hi) -> words [n][4]"""
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, 1).astype(np.uint32)


def counters(stream, sweep, it, entity, blocks):
    blocks = np.asarray(blocks, dtype=np.uint64)
    c = np.empty((blocks.size, 4), np.uint32)
    c[:, 0] = blocks
    c[:, 1] = entity
    c[:, 2] = it & 0xFFFFFFFF
    c[:, 3] = (stream << 24) | (sweep & 0xFFFF)
    return c


def draw_blocks(seed, stream, sweep, it, entity, blocks):
    return philox_np(counters(stream, sweep, it, entity, blocks), seed)


def u32unit(w):
    return (np.asarray(w, dtype=np.float64) + 0.5) * (1.0 / 4294967296.0)


def u53(lo, hi):
    return float(((int(hi) << 32) | int(lo)) >> 11) * (1.0 / 9007199254740992.0)


def box_muller(w0, w1):
    rad = np.sqrt(-2.0 * np.log(1.0 - u32unit(w0)))
    ang = 2.0 * np.pi * u32unit(w1)
    return rad * np.cos(ang), rad * np.sin(ang)


def std_normals(seed, sweep, it, entity, n):
    """z_0 .. z_{n-1}: block b gives z[4b .. 4b+3] = box_muller(x, y).{x, y}, box_muller(z, w).{x, y}"""
    w = draw_blocks(seed, S_SIM, sweep, it, entity, np.arange((n + 3) // 4))
    ax, ay = box_muller(w[:, 0], w[:, 1])
    bx, by = box_muller(w[:, 2], w[:, 3])
    return np.stack([ax, ay, bx, by], 1).ravel()[:n]


def sim_normal(theta, seed, sweep, it, entity, n):
    return theta[0] + theta[1] * std_normals(seed, sweep, it, entity, n)


def sim_binomial(p, n_trials, seed, sweep, it, entity, n):
    """count i = successes among the first n_trials words of the blocks [i B, (i+1) B), B = ceil(n_trials / 4)"""
    B = (n_trials + 3) // 4
    w = draw_blocks(seed, S_SIM, sweep, it, entity, np.arange(n * B)).reshape(n, 4 * B)[:, :n_trials]
    return (u32unit(w) < p).sum(1).astype(np.float64)


def user_words(seed, sweep, it, entity, n, n_blocks):
    """the words a user simulator's generator hands out for value i: blocks (i << 8) | k, k = 0 .. n_blocks-1, in order"""
    blocks = (np.arange(n)[:, None] << 8) | np.arange(n_blocks)[None, :]
    return draw_blocks(seed, S_SIM, sweep, it, entity, blocks.ravel()).reshape(n, 4 * n_blocks)


def kde_density(sample, x, bandwidth=0.0):
    """f(x_j) = 1/(n h) sum_i 3/4 max(0, 1 - ((x_j - s_i)/h)^2); h = bandwidth if > 0 else 0.9 sd n^(-1/5), sd two-pass (n - 1)"""
    n = sample.size
    h = bandwidth
    if not h > 0:
        mean = sample.sum() / n
        sd = math.sqrt(((sample - mean) ** 2).sum() / (n - 1))
        if not sd > 0:
            return None, h
        h = 0.9 * sd * n ** (-0.2)
    x = np.asarray(x, dtype=np.float64)
    f = np.empty(x.size)
    for lo in range(0, x.size, 4096):  # (in slices: a fine grid times 10^4 values does not fit in memory at once)
        u = (x[lo:lo + 4096, None] - sample[None, :]) / h
        f[lo:lo + 4096] = 0.75 * np.maximum(0.0, 1.0 - u * u).sum(1) / (n * h)
    return f, h


def kde_loglike(sample, x, bandwidth=0.0):
    if not np.all(np.isfinite(sample)):
        return -np.inf, None
    f, _ = kde_density(sample, x, bandwidth)
    if f is None:
        return -np.inf, None
    return float(np.log(np.maximum(1e-10, f)).sum()), f


def sum_as_the_kernel(terms):
    """observations in tiles of four, tile T on wave T mod 4, a wave adds its terms in index order, (w0 + w1) + (w2 + w3)"""
    acc = [0.0, 0.0, 0.0, 0.0]
    for j, t in enumerate(terms):
        acc[(j // 4) % 4] += t
    return (acc[0] + acc[1]) + (acc[2] + acc[3])


def freq_loglike(sample, x):
    """sum_j log(#{s_i == x_j} / n): one division, one log (the host's libm) per observation; a count of zero -> -Inf"""
    if not np.all(np.isfinite(sample)):
        return -np.inf
    n = sample.size
    terms = []
    for xj in np.asarray(x, dtype=np.float64):
        c = int((sample == xj).sum())
        terms.append(math.log(c / n) if c > 0 else -math.inf)
    return sum_as_the_kernel(terms)


def log_prior(kind, a, b, x):
    """the prior entries the GPU tests use: 0 flat, 1 Normal(a, b), 2 truncated(Cauchy(a, b), 0, Inf), 4 Beta(a, b)"""
    if kind == 0:
        return 0.0
    if kind == 1:
        return -0.5 * ((x - a) / b) ** 2 - 0.5 * math.log(2 * math.pi) - math.log(b)
    if kind == 2:
        z = (x - a) / b
        return -math.log(math.pi) - math.log(b) - math.log1p(z * z) - math.log(1.0 - (math.atan((0.0 - a) / b) / math.pi + 0.5))
    if kind == 4:
        return (a - 1) * math.log(x) + (b - 1) * math.log1p(-x) - (math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b))
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement checks itself
def test_philox_words_of_the_sim_stream_equal_the_oracles(orc):
    seed = 0x123456789ABCDEF
    for sweep, it, entity in ((0, 0, 0), (1, 7, 23), (3, 2**32 + 5, 4095)):
        blocks = [0, 1, 2, 255, 256, (9999 << 8) | 3, 2**31 + 11]
        ctr = counters(S_SIM, sweep, it, entity, blocks)
        got = philox_np(ctr, seed)
        for row, c in zip(got, ctr):
            assert c[3] == (S_SIM << 24) | sweep
            assert [int(v) for v in row] == orc.philox([int(v) for v in c], [seed & 0xFFFFFFFF, seed >> 32])
    # ... and the PART stream's accept uniform, which the teacher-forced GPU test regenerates
    w = draw_blocks(seed, S_PART, 0, 3, 5, [3])[0]
    assert [int(v) for v in w] == orc.philox([3, 5, 3, S_PART << 24], [seed & 0xFFFFFFFF, seed >> 32])


def test_kde_integrates_to_one():
    for n, bw in ((257, 0.0), (4096, 0.0), (1000, 0.37)):
        s = sim_normal([0.3, 1.7], 11, 0, 0, 5, n)
        _, h = kde_density(s, [0.0], bw)
        grid = np.linspace(s.min() - 1.5 * h, s.max() + 1.5 * h, 200_001)
        f, _ = kde_density(s, grid, bw)
        integral = float(((f[1:] + f[:-1]) * 0.5 * np.diff(grid)).sum())
        assert abs(integral - 1.0) < 1e-6, (n, bw, integral)


def test_kde_floor_and_degenerate_samples():
    s = sim_normal([0.0, 1.0], 3, 0, 0, 0, 500)
    _, h = kde_density(s, [0.0])
    ll, f = kde_loglike(s, [0.1, s.max() + 10 * h])
    assert f[1] == 0.0 and ll == math.log(f[0]) + math.log(1e-10)
    assert kde_loglike(np.full(100, 2.0), [2.0])[0] == -np.inf            # sd == 0
    assert kde_loglike(np.array([0.0, np.inf, 1.0]), [0.5])[0] == -np.inf  # a non-finite simulated value


def test_frequency_estimator_approaches_the_binomial_pmf():
    n, N, p = 100_000, 10, 0.5
    s = sim_binomial(p, N, 99, 0, 0, 1, n)
    assert s.min() >= 0 and s.max() <= N
    try:
        from scipy.stats import binom
        pmfs = [float(binom.pmf(k, N, p)) for k in range(N + 1)]
    except ImportError:  # (the same numbers in closed form)
        pmfs = [math.comb(N, k) * p ** k * (1 - p) ** (N - k) for k in range(N + 1)]
    for k, pmf in enumerate(pmfs):
        est = math.exp(freq_loglike(s, [float(k)]))
        assert abs(est - pmf) <= 4.0 * math.sqrt(pmf * (1 - pmf) / n), (k, est, pmf)
    assert freq_loglike(s, [3.0, 11.0]) == -np.inf  # a count of zero
    assert freq_loglike(s, [3.0, 4.0, 5.0]) == (math.log((s == 3).sum() / n) + math.log((s == 4).sum() / n)) + math.log((s == 5).sum() / n)


def test_box_muller_normals_have_unit_moments():
    z = std_normals(5, 2, 9, 77, 100_000)
    assert abs(z.mean()) < 4 / math.sqrt(z.size) and abs(z.std() - 1.0) < 4 / math.sqrt(2 * z.size)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the Python surface
def test_enums_python_equals_header(demc):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "demc.h")).read()
    F = demc.families
    for name, val in (("SIM_NORMAL", F.SIM_NORMAL), ("SIM_BINOMIAL", F.SIM_BINOMIAL), ("SIM_USER", F.SIM_USER),
                      ("SIMEST_KDE_EPANECHNIKOV", F.SIMEST_KDE_EPANECHNIKOV), ("SIMEST_FREQUENCY", F.SIMEST_FREQUENCY)):
        assert int(re.search(rf"DEMC_{name} = (\d+)", header).group(1)) == val
    assert "demc_set_model_sim" in demc._ffi.EXPORTS
    assert hasattr(demc._ffi.load(), "demc_set_model_sim")
    assert F.SimNormal.code == F.SIM_NORMAL and F.SimBinomial(10).code == F.SIM_BINOMIAL and F.SimSource("x").code == F.SIM_USER


def test_simulated_likelihood_pack_validation(demc):
    F = demc.families
    lk = F.SimulatedLikelihood(F.SimNormal(), n_sim=500, bandwidth=0.25)
    x, dims, hyper = lk.pack([0.5, -1.0, 2.0], [(), ()])
    assert x.tolist() == [0.5, -1.0, 2.0] and dims == [3] and hyper == [0.25]
    with pytest.raises(ValueError):
        lk.pack([0.5], [()])                                   # SimNormal reads (mu, sigma)
    ab = F.SimulatedLikelihood(F.SimBinomial(10), estimator="frequency")
    assert ab.n_sim == 10_000
    x, dims, hyper = ab.pack(dict(N=10, k=4), [()])            # the reference's (N = ..., k = ...)
    assert x.tolist() == [4.0] and dims == [1] and hyper == [0.0, 10.0]
    with pytest.raises(ValueError):
        ab.pack([2.5], [()])                                   # frequency needs integer-valued data
    with pytest.raises(ValueError):
        F.SimulatedLikelihood(F.SimNormal(), n_sim=1)
    with pytest.raises(ValueError):
        F.SimulatedLikelihood(F.SimNormal(), n_sim=F.SIM_MAX_N + 1)
    with pytest.raises(ValueError):
        F.SimulatedLikelihood(F.SimNormal(), estimator="histogram")
    with pytest.raises(ValueError):
        F.SimulatedLikelihood(F.SimNormal(), bandwidth=-1.0)
    with pytest.raises(TypeError):
        F.SimulatedLikelihood("normal")
    with pytest.raises(ValueError):
        F.SimBinomial(2000)
    with pytest.raises(ValueError):
        F.SimSource("")
    src = F.SimulatedLikelihood(F.SimSource("__device__ double demc_user_sim(...);", hyper=[2.0, 3.0]), n_sim=64)
    assert src.pack([1.0], [(), (), ()])[2] == [0.0, 2.0, 3.0]
    assert demc.SimulatedLikelihood is F.SimulatedLikelihood and demc.SimNormal is F.SimNormal


def test_without_a_gpu_the_engine_still_fails_loudly(demc):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    F = demc.families
    rng = np.random.default_rng(1)
    model = demc.DEModel(sample_prior=lambda: [rng.normal(), abs(rng.normal()) + 0.5], names=("mu", "sigma"), data=rng.normal(size=20),
                         prior_loglike=demc.Priors(mu=demc.Normal(0, 1), sigma=demc.TruncatedCauchy(0, 1)),
                         loglike=F.SimulatedLikelihood(F.SimNormal(), n_sim=256))
    de = demc.DE(sample_prior=model.sample_prior, bounds=((-np.inf, np.inf), (0.0, np.inf)), burnin=5, Np=4)
    with pytest.raises(demc.DemcError) as e:
        demc.sample(model, de, demc.HIPBackend(seed=1), 10)
    assert e.value.code == demc._ffi.EHIP


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the code objects
def test_sim_loglike_code_objects(demc, tmp_path):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    from test_abi import kernel_descriptors
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_sim_loglike" in k[0]]
    assert len(ks) == 4, [k[0] for k in ks]  # {normal, binomial} x {kde, frequency}
    for name, regs, agpr, wg, scratch in ks:
        assert wg == 256 and scratch == 0, (name, wg, scratch)
        # two 256-thread workgroups per CU (10 000 simulated values = 80 KB of LDS each) are two waves per SIMD: 256 registers
        # each would do; 128 keeps four waves per SIMD possible for small n_sim
        assert regs <= 128, (name, regs)
