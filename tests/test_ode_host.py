"""ODE-trajectory likelihoods (include/demc.h: DEMC_FAM_ODE_LV, DEMC_PRIOR_TRUNCNORMAL; csrc/demc_ode.hpp: k_ode_loglike) without a
GPU: the numpy restatement that tests/test_gpu_ode.py holds the kernel to -- classical RK4 in the operation order the head comment of
demc_ode.hpp states, one rounded operation per line, and the log-likelihood with its -Inf rules --, checked against itself (order
of convergence, the first integral); the Python surface; the truncated Normal's constant; the code object.

The CPU oracle does not know this family: this file and the project's whole-row source plug-in are its yardsticks."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_2PI = 1.8378770664093454835606594728112  # kLog2Pi of csrc/demc_dimtab.hpp: the double the kernel adds
TRUTH = (1.5, 1.0, 3.0, 1.0)       # Examples/Predator_Prey_Example.jl:14
U0, DT, T_EXAMPLE = (1.0, 1.0), 0.1, 101


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement (rows of proposals side by side: every numpy call below is one IEEE operation per element, none is fused)
def lv_rhs(x, y, al, be, ga, de):
    a = be * y
    a = al - a
    fx = a * x
    b = de * x
    b = b - ga
    fy = b * y
    return fx, fy


def rk4_step(x, y, par, h, h2, h6):
    k1x, k1y = lv_rhs(x, y, *par)
    k2x, k2y = lv_rhs(x + h2 * k1x, y + h2 * k1y, *par)
    k3x, k3y = lv_rhs(x + h2 * k2x, y + h2 * k2y, *par)
    k4x, k4y = lv_rhs(x + h * k3x, y + h * k3y, *par)
    out = []
    for u, k1, k2, k3, k4 in ((x, k1x, k2x, k3x, k4x), (y, k1y, k2y, k3y, k4y)):
        s = 2.0 * k2
        s = k1 + s
        t = 2.0 * k3
        s = s + t
        s = s + k4
        s = h6 * s
        out.append(u + s)
    return out[0], out[1]


def trajectory(theta, T, u0=U0, dt=DT, substeps=10):
    """theta [rows][>= 4] -> the states at t_j = j dt, [T][rows][2]; h = dt / substeps, `substeps` steps between observations, the
    state at t_0 is u0 itself"""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    par = [theta[:, i].copy() for i in range(4)]
    h = dt / float(substeps)
    h2, h6 = 0.5 * h, h / 6.0
    x, y = np.full(theta.shape[0], float(u0[0])), np.full(theta.shape[0], float(u0[1]))
    out = np.empty((T, theta.shape[0], 2))
    with np.errstate(all="ignore"):
        for j in range(T):
            out[j, :, 0], out[j, :, 1] = x, y
            if j + 1 < T:
                for _ in range(substeps):
                    x, y = rk4_step(x, y, par, h, h2, h6)
    return out


def lv_loglike(theta, Y, u0=U0, dt=DT, substeps=10):
    """theta [rows][5] = (alpha, beta, gamma, delta, sigma), Y [T][2] -> loglike [rows]: squared residuals added in (j, c) order
    into one accumulator; -Inf for sigma <= 0, a non-finite sigma, a non-finite sum of squares, or a NaN result"""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    T = Y.shape[0]
    u = trajectory(theta, T, u0, dt, substeps)
    sg = theta[:, 4]
    with np.errstate(all="ignore"):
        ss = np.zeros(theta.shape[0])
        for j in range(T):
            for c in range(2):
                r = Y[j, c] - u[j, :, c]
                q = r * r
                ss = ss + q
        l = np.log(sg)
        l = 2.0 * l
        l = LOG_2PI + l
        l = float(T) * l
        v = sg * sg
        v = 2.0 * v
        e = ss / v
        ll = (-l) - e
    bad = ~(sg > 0.0) | ~(sg < np.inf) | ~(ss < np.inf) | np.isnan(ll)
    return np.where(bad, -np.inf, ll)


def truncnormal_log_mass_erf(mu, sd, lo, hi):
    """the closed form, with erf: log(Phi((hi - mu) / sd) - Phi((lo - mu) / sd))"""
    Phi = lambda z: 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))  # noqa: E731
    return math.log(Phi((hi - mu) / sd) - Phi((lo - mu) / sd))


def log_truncnormal(mu, sd, lo, hi, x):
    """logpdf(truncated(Normal(mu, sd), lo, hi), x) inside the bounds"""
    return -0.5 * ((x - mu) / sd) ** 2 - 0.5 * LOG_2PI - math.log(sd) - truncnormal_log_mass_erf(mu, sd, lo, hi)


def example_data(seed=42, noise=0.5, T=T_EXAMPLE, substeps=640):
    """the example's data: the trajectory at the true parameters from the restatement at fine steps, plus Normal(0, 0.5) noise"""
    u = trajectory([TRUTH], T, substeps=substeps)[:, 0, :]
    return u + noise * np.random.default_rng(seed).normal(0.0, 1.0, u.shape)


def global_errors(substeps_list=(1, 2, 5, 10, 20, 40), fine=640):
    """max over the observation times and both species of |u_substeps - u_fine| at the true parameters: the table of DESIGN.md 5.4"""
    ref = trajectory([TRUTH], T_EXAMPLE, substeps=fine)
    return {s: float(np.abs(trajectory([TRUTH], T_EXAMPLE, substeps=s) - ref).max()) for s in substeps_list}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatement checks itself
def test_halving_the_step_cuts_the_end_point_error_sixteenfold():
    ref = trajectory([TRUTH], T_EXAMPLE, substeps=640)[-1, 0]
    err = {s: float(np.abs(trajectory([TRUTH], T_EXAMPLE, substeps=s)[-1, 0] - ref).max()) for s in (5, 10, 20)}
    for coarse, fine in ((5, 10), (10, 20)):
        ratio = err[coarse] / err[fine]
        print(f"end-point error substeps {coarse}: {err[coarse]:.3e}, {fine}: {err[fine]:.3e}, ratio {ratio:.2f}")
        assert 12.0 <= ratio <= 20.0, (coarse, fine, ratio)  # fourth order: 2^4, give or take the next term


def test_the_first_integral_drifts_less_at_the_finer_step():
    al, be, ga, de = TRUTH

    def drift(s):
        u = trajectory([TRUTH], T_EXAMPLE, substeps=s)[:, 0, :]
        V = de * u[:, 0] - ga * np.log(u[:, 0]) + be * u[:, 1] - al * np.log(u[:, 1])
        return float(np.abs(V - V[0]).max())

    d = {s: drift(s) for s in (1, 2, 5, 10, 20)}
    print("first-integral drift over (0, 10):", ", ".join(f"substeps {s}: {v:.3e}" for s, v in d.items()))
    for coarse, fine in ((1, 2), (2, 5), (5, 10), (10, 20)):
        assert d[fine] < d[coarse], (coarse, fine, d)


def test_global_error_table_stays_under_the_noise():
    """the deviation table of DESIGN.md 5.4 (fixed-step RK4 instead of the reference's Tsit5()): printed for the record; the default
    substeps of LotkaVolterraLikelihood must sit at least four orders of magnitude under the example's noise level 0.5"""
    import demc_amd
    errs = global_errors()
    for s, e in errs.items():
        print(f"substeps {s:3d}: h = {DT / s:.5f}, max |u - u_640| over (0, 10) = {e:.3e}")
    default = demc_amd.families.LotkaVolterraLikelihood().substeps
    assert default in errs and errs[default] < 0.5e-4
    assert errs[1] < 0.5 and all(errs[a] > errs[b] for a, b in ((1, 2), (2, 5), (5, 10), (10, 20), (20, 40)))


def test_loglike_degenerate_rows_and_the_single_time():
    Y = example_data(T=5)
    th = np.array([list(TRUTH) + [0.5], list(TRUTH) + [0.0], list(TRUTH) + [-1.0], list(TRUTH) + [np.inf], list(TRUTH) + [np.nan],
                   [2.5, 0.0, 1.0, 2.0, 0.5]])
    ll = lv_loglike(th, Y)
    assert np.isfinite(ll[0]) and (ll[1:5] == -np.inf).all() and np.isfinite(ll[5])
    # one coarse step of 5 time units overflows the double range within a few observations: -Inf, never a NaN
    big = lv_loglike([[2.5, 0.0, 1.0, 2.0, 0.5]], example_data(T=12), dt=5.0, substeps=1)
    assert big[0] == -np.inf
    # T = 1: no step at all, the residual is taken at u0
    y0 = np.array([[1.3, 0.6]])
    want = -(LOG_2PI + 2.0 * math.log(0.7)) - ((1.3 - 1.0) ** 2 + (0.6 - 1.0) ** 2) / (2.0 * 0.7 ** 2)
    assert abs(lv_loglike([list(TRUTH) + [0.7]], y0)[0] - want) <= 1e-15 * abs(want)
    # ... and against the sum of Normal log-densities, term by term
    u = trajectory([TRUTH], 5)[:, 0, :]
    terms = sum(-0.5 * ((Y[j, c] - u[j, c]) / 0.5) ** 2 - 0.5 * LOG_2PI - math.log(0.5) for j in range(5) for c in range(2))
    assert abs(ll[0] - terms) <= 1e-13 * abs(terms)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. enums and constants
def _header_values(names):
    """the values as the C compiler sees include/demc.h"""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "v.c")
        fmt = " ".join("%d" for _ in names)
        open(src, "w").write('#include <stdio.h>\n#include "demc.h"\nint main(){printf("%s", %s);return 0;}' % (fmt, ", ".join("(int)" + n for n in names)))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(td, "v")])
        return [int(v) for v in subprocess.check_output([os.path.join(td, "v")]).split()]


def test_enums_python_equals_header(demc):
    F = demc.families
    fam, pri, cauchy, rast, user = _header_values(["DEMC_FAM_ODE_LV", "DEMC_PRIOR_TRUNCNORMAL", "DEMC_PRIOR_CAUCHY", "DEMC_FAM_RASTRIGIN", "DEMC_FAM_USER"])
    assert (fam, pri) == (9, 10) and (cauchy, rast, user) == (9, 8, 100)
    assert F.FAM_ODE_LV == fam and F.PRIOR_TRUNCNORMAL == pri
    assert F.LotkaVolterraLikelihood.family == fam and F.TruncatedNormal(1.0, 2.0).kind == pri
    assert demc.LotkaVolterraLikelihood is F.LotkaVolterraLikelihood and demc.TruncatedNormal is F.TruncatedNormal
    hpp = open(os.path.join(os.path.dirname(demc._ffi.LIB_PATH), "csrc", "demc_ode.hpp")).read()
    assert int(re.search(r"constexpr int FAM_ODE_LV = (\d+);", hpp).group(1)) == fam
    assert int(re.search(r"constexpr int kOdeMaxT = (\d+);", hpp).group(1)) == F.ODE_MAX_T == 4096
    assert int(re.search(r"constexpr int kOdeMaxSubsteps = (\d+);", hpp).group(1)) == F.ODE_MAX_SUBSTEPS == 1024
    jl = open(os.path.join(ROOT, "julia", "DEMCHIP.jl")).read()
    assert re.search(r"const FAM_ODE_LV = Int32\(9\)", jl) and re.search(r"const PRIOR_TRUNCNORMAL = Int32\(10\)", jl)


def test_no_new_entry_point(demc):
    from test_abi import declared_functions
    assert len(demc._ffi.EXPORTS) == len(declared_functions()) == 51


# ---------------------------------------------------------------------------------------------------------------------------
# 3. packing
def test_lotka_volterra_pack(demc):
    F = demc.families
    shapes = [(), (), (), (), ()]
    Y = example_data(T=7)                      # [T][2]
    lk = F.LotkaVolterraLikelihood(u0=(1.0, 2.0), dt=0.25, substeps=4)
    for given in (Y.T, Y):                     # the reference's 2 x T, or T x 2
        x, dims, hyper = lk.pack(given, shapes)
        assert x.shape == (7, 2) and x.flags["C_CONTIGUOUS"] and np.array_equal(x, Y) and dims == [7, 2] and hyper == [1.0, 2.0, 0.25, 4.0]
    d = F.LotkaVolterraLikelihood()
    assert d.u0 == (1.0, 1.0) and d.dt == 0.1 and 1 <= d.substeps <= 1024
    assert lk.pack(np.zeros((2, 1)), shapes)[1] == [1, 2] and lk.pack(np.zeros((2, 4096)), shapes)[1] == [4096, 2]
    bad_Y = Y.copy()
    bad_Y[3, 1] = np.nan
    for data, shp in ((Y, [(), (), (), ()]),                 # D != 5
                      (Y, [(5,), ()]),                        # D = 6
                      (np.zeros((3, 7)), shapes),             # dims[1] != 2
                      (np.zeros(14), shapes),                 # not two-dimensional
                      (np.zeros((2, 0)), shapes),             # T < 1
                      (np.zeros((2, 4097)), shapes),          # T > 4096
                      (bad_Y, shapes),                        # a NaN observation
                      (np.where(np.isnan(bad_Y), np.inf, bad_Y), shapes)):
        with pytest.raises(ValueError):
            lk.pack(data, shp)
    for kw in (dict(substeps=0), dict(substeps=1025), dict(substeps=2.5), dict(dt=0.0), dict(dt=-0.1), dict(dt=np.inf), dict(dt=np.nan),
               dict(u0=(1.0, np.inf)), dict(u0=(np.nan, 1.0)), dict(u0=(1.0, 1.0, 1.0))):
        with pytest.raises(ValueError):
            F.LotkaVolterraLikelihood(**kw)
    assert F.LotkaVolterraLikelihood(substeps=1).substeps == 1 and F.LotkaVolterraLikelihood(substeps=1024).substeps == 1024


def test_truncated_normal_flows_into_the_prior_table(demc):
    """Priors(...) with TruncatedNormal entries -> kind 10 with (mu, sd) in the table the sampler hands to demc_set_priors"""
    from demc_amd import sampler
    F = demc.families
    model = demc.DEModel(sample_prior=lambda: [1.0, 1.0, 3.0, 1.0, 0.5], names=("α", "β", "γ", "δ", "σ"), data=example_data().T,
                         loglike=F.LotkaVolterraLikelihood(),
                         prior_loglike=demc.Priors(α=F.TruncatedNormal(1.5, 0.5), β=F.TruncatedNormal(1.2, 0.5), γ=F.TruncatedNormal(3.0, 0.5),
                                                   δ=F.TruncatedNormal(1.0, 0.5), σ=F.LogNormal(0.4, 0.8)))
    de = demc.DE(sample_prior=model.sample_prior, bounds=((0.5, 2.5), (0, 2), (1, 4), (0, 2), (0, np.inf)), Np=12, n_groups=3)
    lay = sampler._flat_layout(model, de, model.sample_prior())
    assert lay["D"] == 5 and lay["kind"].tolist() == [10, 10, 10, 10, F.PRIOR_LOGNORMAL]
    assert lay["a"].tolist() == [1.5, 1.2, 3.0, 1.0, 0.4] and lay["b"].tolist() == [0.5, 0.5, 0.5, 0.5, 0.8]
    assert lay["lo"].tolist() == [0.5, 0.0, 1.0, 0.0, 0.0] and lay["hi"][:4].tolist() == [2.5, 2.0, 4.0, 2.0]


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the truncated Normal's constant
@pytest.mark.parametrize("mu,sd,lo,hi", [(1.5, 0.5, 0.5, 2.5), (1.2, 0.5, 0.0, 2.0), (3.0, 0.5, 1.0, 4.0), (1.0, 0.5, 0.0, math.inf)])
def test_truncated_normal_constant_is_the_erf_closed_form(demc, mu, sd, lo, hi):
    """the library takes log(Phi((hi - mu) / sd) - Phi((lo - mu) / sd)) off the Normal's constant, formed with erfc
    (TruncatedNormal.log_mass restates it; tests/test_gpu_ode.py holds the device to it): equal to math.log of the erf closed form to
    a few units in the last place of a mass of order one"""
    got = demc.families.TruncatedNormal(mu, sd).log_mass(lo, hi)
    want = truncnormal_log_mass_erf(mu, sd, lo, hi)
    print(f"truncated(Normal({mu}, {sd}), {lo}, {hi}): log mass {got!r} (erfc) {want!r} (erf)")
    assert -0.2 < want < 0.0 and abs(got - want) <= 8 * 2.0 ** -53  # |d log m| = |dm| / m, m > 0.8, a few roundings of 2^-53
    x = 0.5 * (max(lo, mu - sd) + min(hi, mu + sd))
    full = -0.5 * ((x - mu) / sd) ** 2 - 0.5 * LOG_2PI - math.log(sd)
    assert abs((full - got) - log_truncnormal(mu, sd, lo, hi, x)) <= 1e-15


def test_truncated_normal_refusals(demc):
    TN = demc.families.TruncatedNormal
    for lo, hi in ((2.0, 2.0), (3.0, 1.0), (60.0, 61.0), (-61.0, -60.0), (math.nan, 1.0)):  # empty bounds; no mass in double precision
        with pytest.raises(ValueError):
            TN(0.0, 1.0).log_mass(lo, hi)
    for mu, sd in ((0.0, 0.0), (0.0, -1.0), (math.inf, 1.0), (0.0, math.nan)):
        with pytest.raises(ValueError):
            TN(mu, sd)
    assert TN(0.0, 1.0).log_mass(-math.inf, math.inf) == 0.0
    # far in one tail the erfc form keeps its digits where 1 - Phi would have lost them
    assert abs(TN(0.0, 1.0).log_mass(8.0, 9.0) - math.log(0.5 * (math.erfc(8.0 / math.sqrt(2)) - math.erfc(9.0 / math.sqrt(2))))) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the code object
def test_ode_loglike_code_object(demc, tmp_path):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/clang-offload-bundler"):
        pytest.skip("no ROCm LLVM tools")
    from test_abi import kernel_descriptors
    all_ks = kernel_descriptors(demc._ffi.LIB_PATH, str(tmp_path))
    ks = [k for k in all_ks if "k_ode_loglike" in k[0]]
    assert len(ks) == 1, [k[0] for k in ks]  # Lotka-Volterra
    name, regs, agpr, wg, scratch = ks[0]
    print(f"{name}: {regs} registers ({agpr} AGPRs), workgroup {wg}, scratch {scratch}")
    assert wg == 256 and scratch == 0, (name, wg, scratch)
    # the simulation kernels' counts are untouched (their own tests pin them; the new symbol contains neither substring)
    assert sum("k_sim_loglike" in k[0] for k in all_ks) == 4 and sum("k_sim_choice" in k[0] for k in all_ks) == 1
