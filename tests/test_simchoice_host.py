"""Likelihood-free choice and response-time models (include/demc.h: DEMC_SIM_LNR, DEMC_SIMEST_KDE_CHOICE) without a GPU: the numpy
restatement of the race simulator and of the per-choice defective kernel density that tests/test_gpu_simchoice.py holds the kernel
to, checked against itself; the Python surface; the code object of k_sim_choice.

Philox, Box-Muller, the user generator's words and the priors come from tests/test_simlike_host.py."""
import math
import os
import re

import numpy as np
import pytest

import test_simlike_host as R

LOG_FLOOR = math.log(1e-10)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
def lnr_normals(seed, sweep, it, entity, n, K):
    """z[i][k]: value i uses the blocks [i B, (i+1) B), B = ceil(K / 4); accumulator k takes normal k of those blocks, per block
    box_muller(x, y).{x, y}, box_muller(z, w).{x, y}"""
    B = (K + 3) // 4
    w = R.draw_blocks(seed, R.S_SIM, sweep, it, entity, np.arange(n * B))
    ax, ay = R.box_muller(w[:, 0], w[:, 1])
    bx, by = R.box_muller(w[:, 2], w[:, 3])
    return np.stack([ax, ay, bx, by], 1).reshape(n, 4 * B)[:, :K]


def race(T):
    """choice = 1 + argmin_k T_k with ties to the lower k (a strict <, as the kernel compares), time = min_k T_k"""
    best, arg = T[:, 0].copy(), np.zeros(T.shape[0], np.int64)
    for k in range(1, T.shape[1]):
        upd = T[:, k] < best
        best[upd], arg[upd] = T[upd, k], k
    return arg + 1, best


def sim_lnr(theta, sigma, seed, sweep, it, entity, n):
    """theta = (nu[K], tau): T_k = exp(nu_k + sigma z_k), c = 1 + argmin_k T_k, t = tau + min_k T_k -> (c[n], t[n])"""
    theta = np.asarray(theta, dtype=np.float64)
    K = theta.size - 1
    with np.errstate(all="ignore"):
        T = np.exp(theta[None, :K] + sigma * lnr_normals(seed, sweep, it, entity, n, K))
    c, best = race(T)
    return c, theta[K] + best


def choice_bandwidth(c, t, choice, bandwidth=0.0):
    """h of one choice: the caller's when > 0, else 0.9 sd_c n_c^(-1/5) with sd_c the two-pass standard deviation (n_c - 1) and
    n_c^(-1/5) one pow; None: no estimate (n_c < 2 or sd_c == 0 under the rule of thumb)"""
    if bandwidth > 0:
        return bandwidth
    sel = t[c == choice]
    n_c = sel.size
    if n_c < 2:
        return None
    mean = sel.sum() / n_c
    sd = math.sqrt(((sel - mean) ** 2).sum() / (n_c - 1))
    if not (sd > 0 and math.isfinite(sd)):
        return None
    return (0.9 * sd) * math.pow(float(n_c), -0.2)


def choice_kde_density(c, t, choice, x, bandwidth=0.0):
    """the DEFECTIVE density f(choice, x_j) = 1/(n h_c) sum_{i: c_i = choice} 3/4 max(0, 1 - ((x_j - t_i)/h_c)^2): the
    normaliser is n = ALL simulated values; 0 everywhere for a choice without an estimate -> (f, h_c or None)"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    h = choice_bandwidth(c, t, choice, bandwidth)
    if h is None:
        return np.zeros(x.size), None
    sel, f = np.sort(t[c == choice]), np.empty(x.size)
    for lo in range(0, x.size, 2048):  # (in slices, each against the values within h of it: the others add exact zeros)
        xs = x[lo:lo + 2048]
        near = sel[np.searchsorted(sel, xs.min() - h, "left"):np.searchsorted(sel, xs.max() + h, "right")]
        u = (xs[:, None] - near[None, :]) / h
        f[lo:lo + 2048] = 0.75 * np.maximum(0.0, 1.0 - u * u).sum(1) / (c.size * h)
    return f, h


def choice_kde_loglike(c, t, obs_c, obs_x, bandwidth=0.0):
    """sum_j log max(1e-10, f(c_j, x_j)), summed in the kernel's order -> (loglike, f[N]); -Inf for a choice outside [0, 255] or a
    non-finite t_i with c_i >= 1 (the t of a choice-0 value is not looked at)"""
    c, t = np.asarray(c), np.asarray(t, dtype=np.float64)
    if np.any((c < 0) | (c > 255)) or not np.all(np.isfinite(t[c >= 1])):
        return -np.inf, None
    obs_c, obs_x = np.atleast_1d(np.asarray(obs_c)).astype(np.int64), np.atleast_1d(np.asarray(obs_x, dtype=np.float64))
    f = np.empty(obs_x.size)
    for k in np.unique(obs_c):
        f[obs_c == k] = choice_kde_density(c, t, int(k), obs_x[obs_c == k], bandwidth)[0]
    return R.sum_as_the_kernel([math.log(max(1e-10, v)) for v in f]), f


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement checks itself
@pytest.mark.parametrize("bw", [0.0, 0.04])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n", [257, 4096])
def test_choice_density_integrates_to_the_choice_share(n, K, bw):
    theta = [-1.0, -0.8, -0.9][:K] + [0.2]
    c, t = sim_lnr(theta, 0.3, 11 + K, 0, 0, 5, n)
    total = 0.0
    for k in range(1, K + 1):
        n_c = int((c == k).sum())
        assert n_c >= 2
        h = choice_bandwidth(c, t, k, bw)
        sel = t[c == k]
        grid = np.linspace(sel.min() - 1.5 * h, sel.max() + 1.5 * h, 100_001)
        f, _ = choice_kde_density(c, t, k, grid, bw)
        integral = float(((f[1:] + f[:-1]) * 0.5 * np.diff(grid)).sum())
        print(f"n={n} K={K} bw={bw} choice {k}: h = {h:.4g}, integral - n_c/n = {integral - n_c / n:+.3g}")
        assert abs(integral - n_c / n) < 1e-6, (n, K, bw, k, integral, n_c / n)
        total += integral
    assert abs(total - 1.0) < 3e-6  # (every value has a choice >= 1 here: the defective densities add up to one)


def test_lnr_choice_share_is_the_normal_cdf():
    n = 100_000
    for nu, sigma in (((-1.0, -0.7), 1.0), ((-0.5, -1.4), 0.6)):
        c, t = sim_lnr(list(nu) + [0.25], sigma, 2718, 1, 3, 9, n)
        p = 0.5 * (1.0 + math.erf((nu[1] - nu[0]) / (sigma * math.sqrt(2.0)) / math.sqrt(2.0)))
        share = float((c == 1).mean())
        assert abs(share - p) <= 4.0 * math.sqrt(p * (1 - p) / n), (nu, sigma, share, p)
        assert set(np.unique(c)) == {1, 2} and t.min() > 0.25


def test_lnr_uses_two_blocks_per_value_from_five_accumulators():
    z5 = lnr_normals(5, 0, 2, 3, 10, 5)
    w = R.draw_blocks(5, R.S_SIM, 0, 2, 3, [6, 7])  # value 3: blocks 6 and 7
    assert z5.shape == (10, 5)
    assert z5[3, 1] == R.box_muller(w[0, 0], w[0, 1])[1] and z5[3, 4] == R.box_muller(w[1, 0], w[1, 1])[0]
    c, best = race(np.array([[2.0, 1.0, 1.0], [1.0, 1.0, 3.0], [np.nan, 1.0, 2.0]]))
    assert c.tolist() == [2, 1, 1] and best[0] == 1.0 and np.isnan(best[2])  # ties to the lower k; a NaN time stays a NaN


def test_choices_without_an_estimate_sit_exactly_at_the_floor():
    c, t = sim_lnr([-1.0, -0.8, 0.2], 0.5, 3, 0, 0, 0, 500)
    x1 = float(np.median(t[c == 1]))
    f1 = choice_kde_density(c, t, 1, [x1])[0][0]
    assert f1 > 1e-2
    # a choice never simulated: exactly log(1e-10) per observation, the row finite
    ll, f = choice_kde_loglike(c, t, [1, 3, 3], [x1, 0.5, 0.6])
    assert f[1] == 0.0 and f[2] == 0.0 and ll == R.sum_as_the_kernel([math.log(f1), LOG_FLOOR, LOG_FLOOR]) and math.isfinite(ll)
    ll, f = choice_kde_loglike(c, t, [3], [0.5], 0.1)  # ... under a fixed bandwidth too
    assert ll == LOG_FLOOR
    # n_c = 1: no estimate under the rule of thumb, a real one under a fixed bandwidth
    c1, t1 = np.append(c, 3), np.append(t, 0.7)
    assert choice_kde_loglike(c1, t1, [3], [0.7])[0] == LOG_FLOOR
    ll, f = choice_kde_loglike(c1, t1, [3], [0.72], 0.1)
    assert f[0] == 0.75 * (1.0 - ((0.72 - 0.7) / 0.1) ** 2) / (501 * 0.1) and ll == math.log(f[0])
    # sd_c == 0: no estimate under the rule of thumb
    c2, t2 = np.append(c1, 3), np.append(t1, 0.7)
    assert choice_kde_loglike(c2, t2, [3, 1], [0.7, x1])[0] == R.sum_as_the_kernel([LOG_FLOOR, math.log(choice_kde_density(c2, t2, 1, [x1])[0][0])])
    assert choice_kde_loglike(c2, t2, [3], [0.7], 0.1)[1][0] > 0
    # a non-finite time of a choice >= 1: -Inf; a choice outside [0, 255]: -Inf
    tb = t.copy()
    tb[7] = np.inf
    assert choice_kde_loglike(c, tb, [1], [x1])[0] == -np.inf
    assert choice_kde_loglike(np.append(c, 256), np.append(t, 0.5), [1], [x1])[0] == -np.inf


@pytest.mark.parametrize("bw", [0.0, 0.07])
def test_choice_zero_values_only_scale_the_densities(bw):
    c, t = sim_lnr([-1.0, -0.8, 0.2], 0.5, 4, 0, 0, 1, 1000)
    x = np.quantile(t, [0.2, 0.5, 0.8])
    m = 250
    c0, t0 = np.concatenate([c, np.zeros(m, np.int64)]), np.concatenate([t, np.full(m, np.nan)])  # (their t is never looked at)
    for k in (1, 2):
        f, h = choice_kde_density(c, t, k, x, bw)
        f0, h0 = choice_kde_density(c0, t0, k, x, bw)
        assert h0 == h and f.min() > 0
        assert np.allclose(f0, f * (1000 / (1000 + m)), rtol=1e-14, atol=0.0)  # every density lower by the same factor n / (n + m)
    assert math.isfinite(choice_kde_loglike(c0, t0, [1, 2], x[:2], bw)[0])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the Python surface
def test_enums_python_equals_header(demc):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "demc.h")).read()
    F = demc.families
    for name, val in (("SIM_LNR", F.SIM_LNR), ("SIMEST_KDE_CHOICE", F.SIMEST_KDE_CHOICE), ("SIM_NORMAL", F.SIM_NORMAL),
                      ("SIM_USER", F.SIM_USER)):
        assert int(re.search(rf"DEMC_{name} = (\d+)", header).group(1)) == val
    assert F.SIM_LNR == 2 and F.SIMEST_KDE_CHOICE == 2
    assert F.SimLNR().code == F.SIM_LNR and F.SimLNR().pairs and F.SimSource("x", choice=True).pairs and not F.SimSource("x").pairs
    assert F.SimulatedLikelihood.ESTIMATORS["kde_choice"] == F.SIMEST_KDE_CHOICE
    assert demc.SimLNR is F.SimLNR
    csrc = os.path.join(os.path.dirname(demc._ffi.LIB_PATH), "csrc", "demc_simlike.hpp")
    cap = int(re.search(r"constexpr int kSimChoiceMaxN = (\d+);", open(csrc).read()).group(1))
    assert F.SIM_CHOICE_MAX_N == cap and 10_000 <= cap <= F.SIM_MAX_N
    assert len(demc._ffi.EXPORTS) == 51  # no new entry point


def test_simulated_likelihood_pack_of_pairs(demc):
    F = demc.families
    lk = F.SimulatedLikelihood(F.SimLNR(sigma=0.8), estimator="kde_choice", n_sim=500, bandwidth=0.05)
    x, dims, hyper = lk.pack(([1, 2, 2], [0.5, 0.6, 0.7]), [(2,), ()])
    assert x.tolist() == [1.0, 2.0, 2.0, 0.5, 0.6, 0.7] and dims == [3] and hyper == [0.05, 0.8]  # [choices..., rts...]
    ref = F.LNRLikelihood().pack(([1, 2, 2], [0.5, 0.6, 0.7]), [(2,), ()])[0]
    assert x.tolist() == ref.tolist()
    for bad in (([1, 3], [0.5, 0.6]),        # choice above K = 2
                ([0, 1], [0.5, 0.6]),        # choice 0 is not an observation
                ([1.5, 1], [0.5, 0.6]),      # not an integer
                ([1, 2], [0.5]),             # lengths differ
                ([1, 2], [0.5, np.inf])):    # a non-finite response time
        with pytest.raises(ValueError):
            lk.pack(bad, [(2,), ()])
    with pytest.raises(ValueError):
        lk.pack(([1], [0.5]), [(1,), ()])    # K = 1: no race
    with pytest.raises(ValueError):
        lk.pack(([1], [0.5]), [(9,), ()])    # K = 9
    # pairs and scalars do not mix
    for sim, est in ((F.SimLNR(), "kde"), (F.SimLNR(), "frequency"), (F.SimNormal(), "kde_choice"), (F.SimBinomial(10), "kde_choice"),
                     (F.SimSource("x"), "kde_choice"), (F.SimSource("x", choice=True), "kde")):
        with pytest.raises(ValueError):
            F.SimulatedLikelihood(sim, estimator=est)
    with pytest.raises(ValueError):
        F.SimulatedLikelihood(F.SimLNR(), estimator="kde_choice", n_sim=F.SIM_CHOICE_MAX_N + 1)
    with pytest.raises(ValueError):
        F.SimLNR(sigma=0.0)
    assert F.SimulatedLikelihood(F.SimLNR(), estimator="kde_choice").n_sim == 10_000
    usr = F.SimulatedLikelihood(F.SimSource("__device__ double demc_user_sim_choice(...);", hyper=[2.0], choice=True), "kde_choice", n_sim=64)
    x, dims, hyper = usr.pack(([255, 1], [0.1, 0.2]), [(), ()])
    assert x.tolist() == [255.0, 1.0, 0.1, 0.2] and hyper == [0.0, 2.0]
    with pytest.raises(ValueError):
        usr.pack(([256], [0.1]), [()])


def test_set_model_sim_passes_half_the_length_for_pairs(demc):
    calls = []

    class Lib:
        def demc_set_model_sim(self, h, sim, est, n_sim, src, data, n_obs, hyper, nhyper):
            calls.append((sim, est, n_sim, n_obs, nhyper))
            return 0

    e = object.__new__(demc.HipEngine)
    e.L, e.h = Lib(), None
    e.set_model_sim(2, 2, 100, [1, 2, 1, 0.5, 0.6, 0.7], hyper=[0.0, 1.0])
    e.set_model_sim(0, 0, 100, [0.5, 0.6, 0.7, 0.8])
    assert calls == [(2, 2, 100, 3, 2), (0, 0, 100, 4, 0)]
    with pytest.raises(ValueError):
        e.set_model_sim(2, 2, 100, [1, 2, 0.5], hyper=[0.0, 1.0])


def test_the_embedded_kernel_text_declares_the_pair_simulator(demc):
    """what hiprtc compiles around a user simulator is built into the library as a string (csrc/Makefile: demc_simlike_src.inc)"""
    assert b"demc_user_sim_choice" in open(demc._ffi.LIB_PATH, "rb").read()
    inc = os.path.join(os.path.dirname(demc._ffi.LIB_PATH), "csrc", "demc_simlike_src.inc")
    assert "demc_user_sim_choice" in open(inc).read()


def test_julia_shim_names_the_pair_codes():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jl = open(os.path.join(root, "julia", "DEMCHIP.jl")).read()
    assert re.search(r":lnr\s*=>\s*Int32\(2\)", jl) and re.search(r":kde_choice\s*=>\s*Int32\(2\)", jl)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the code object
def test_sim_choice_code_objects(demc, tmp_path):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    from test_abi import kernel_descriptors
    ks = [k for k in kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path)) if "k_sim_choice" in k[0]]
    assert len(ks) == 1, [k[0] for k in ks]  # the log-normal race; user simulators are compiled at demc_set_model_sim
    for name, regs, agpr, wg, scratch in ks:
        assert wg == 256 and scratch == 0 and regs <= 128, (name, regs, wg, scratch)
