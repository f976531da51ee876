"""Likelihood-free choice and response-time models on the GPU (include/demc.h: DEMC_SIM_LNR, DEMC_SIMEST_KDE_CHOICE;
csrc/demc_simlike.hpp: k_sim_choice) against the numpy restatement of tests/test_simchoice_host.py, which regenerates every draw
from the addressed Philox stream 7.

Bars: log-likelihoods / log-posteriors at rtol 1e-9 (the project's log-posterior bar) where no observation sits at the 1e-10
floor -- asserted on the restatement, min f >= 1e-2 --; an observation of a choice without an estimate contributes exactly
log(1e-10); accept decisions exactly, except where |u - exp(w' - w)| < 1e-7; same seed, sharded or not: same bits."""
import math

import numpy as np
import pytest

import test_simchoice_host as C
import test_simlike_host as R

pytestmark = pytest.mark.gpu
INF = np.inf
SIM_NORMAL, SIM_BINOMIAL, SIM_LNR, SIM_USER, KDE, FREQ, KDE_CHOICE = 0, 1, 2, 100, 0, 1, 2
LOG_FLOOR = math.log(1e-10)


@pytest.fixture()
def D(demc):
    return demc


def rel(a, b):
    return 0.0 if a == b else abs(a - b) / max(abs(b), 1e-300)


def pack(c, x):
    return np.concatenate([np.asarray(c, dtype=np.float64), np.asarray(x, dtype=np.float64)])


def observations_in_the_bulk(rng, c, t, N):
    """the choice uniform among the choices with a share >= 0.1, the time a U(0.25, 0.75) quantile of that choice's simulated times"""
    common = [k for k in range(1, int(c.max()) + 1) if (c == k).mean() >= 0.1]
    oc = rng.choice(common, N)
    ox = np.array([np.quantile(t[c == k], rng.uniform(0.25, 0.75)) for k in oc])
    return oc, ox


def lnr_rows(rng, n_rows, K):
    return np.concatenate([rng.uniform(-1.5, -0.5, (n_rows, K)), rng.uniform(0.1, 0.3, (n_rows, 1))], 1)


# ---- 1. demc_logpost vs the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 50])
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("n_sim", [257, 4096, 10_000])
def test_logpost_kde_choice_lnr_equals_the_restatement(D, n_sim, K, N):
    rng = np.random.default_rng(100_000 * K + 1000 * N + n_sim)
    seed, n_rows = 99 + n_sim + K, 6
    theta = lnr_rows(rng, n_rows, K)
    e = D.HipEngine(n_groups=2, Np=4, D=K + 1, seed=seed, schedule=2)
    worst, fmin = 0.0, INF
    try:
        e.set_bounds([-INF] * (K + 1), [INF] * (K + 1))
        for r in range(n_rows):
            sigma = 1.0 if r % 2 == 0 else 0.6
            c, t = C.sim_lnr(theta[r], sigma, seed, 0, 0, r, n_sim)  # row r of the call is evaluated at entity r, iter = sweep = 0
            oc, ox = observations_in_the_bulk(rng, c, t, N)
            e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[0.0, sigma])
            got = e.logpost(theta)[r]
            want, f = C.choice_kde_loglike(c, t, oc, ox)
            fmin = min(fmin, f.min())
            assert f.min() >= 1e-2, f"vacuity guard: an observation near the floor (min f = {f.min():.3g})"
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-9, (r, got, want)
    finally:
        e.close()
    print(f"kde_choice/lnr n_sim={n_sim} K={K} N={N}: max relative difference {worst:.3g}, min f {fmin:.3g}")


# ---- 2. edges, forced with theta and a user simulator -------------------------------------------------------------------------
SRC_SECOND_CHOICE_BELOW = """
__device__ double demc_user_sim_choice(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng, int* choice) {
    const unsigned w = demc_sim_u32(rng);                 // choice 2 iff the value's first word is below hyper[0]
    *choice = (double)w < hyper[0] ? 2 : 1;
    return theta[0] + theta[1] * demc_sim_normal(rng);    // (words 1 and 2)
}
"""
SRC_NO_RESPONSE_BELOW = """
__device__ double demc_user_sim_choice(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng, int* choice) {
    const unsigned w = demc_sim_u32(rng);                 // no response (choice 0, a time that is not a number) below hyper[0]
    const double z = demc_sim_normal(rng);
    *choice = (double)w < hyper[0] ? 0 : (z < 0.0 ? 1 : 2);
    return (double)w < hyper[0] ? nan("") : theta[0] + theta[1] * z;
}
"""
SRC_CHOICE_OUT_OF_RANGE = """
__device__ double demc_user_sim_choice(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng, int* choice) {
    const unsigned w = demc_sim_u32(rng);
    *choice = w < 40000000u ? (int)hyper[0] : 1;          // about one value in a hundred
    return theta[0] + demc_sim_uniform(rng);
}
"""


def test_a_choice_never_simulated_contributes_exactly_the_floor(D):
    seed, n_sim = 17, 2000
    th = np.array([[-40.0, 0.0, 0.0], [-1.0, -0.8, 0.2]])  # row 0: accumulator 1 always wins (times of the order of exp(-40))
    e = D.HipEngine(n_groups=1, Np=4, D=3, seed=seed)
    try:
        e.set_bounds([-INF] * 3, [INF] * 3)
        c, t = C.sim_lnr(th[0], 1.0, seed, 0, 0, 0, n_sim)
        assert (c == 1).all() and np.isfinite(t).all()
        x1 = np.quantile(t, [0.3, 0.5, 0.6])
        e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack([2], [0.5]), hyper=[0.0, 1.0])
        assert e.logpost(th)[0] == LOG_FLOOR                       # exactly, and the row is finite
        e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack([2], [0.5]), hyper=[0.05, 1.0])
        assert e.logpost(th)[0] == LOG_FLOOR                       # n_c == 0 under a fixed bandwidth
        oc, ox = [1, 2, 1, 1, 2], [x1[0], 0.5, x1[1], x1[2], 0.7]
        e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[0.0, 1.0])
        got = e.logpost(th)[0]
        want, f = C.choice_kde_loglike(c, t, oc, ox)
        assert f[1] == 0.0 and f[4] == 0.0 and f[[0, 2, 3]].min() >= 1e-2 and math.isfinite(got)
        assert rel(got, want) <= 1e-9, (got, want)
        assert rel(got - 2 * LOG_FLOOR, want - 2 * LOG_FLOOR) <= 1e-8  # (the three real terms alone, after the cancellation)
        # sigma = Inf: exp(nu + Inf z) is 0 or Inf -- a quarter of the values have no finite time: -Inf, never a NaN
        e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack([1], [0.4]), hyper=[0.0, INF])
        got = e.logpost(th)
        assert got[0] == -INF and got[1] == -INF
    finally:
        e.close()


@pytest.mark.parametrize("bw", [0.0, 0.1])
def test_a_choice_simulated_once(D, bw):
    """n_c = 1: no estimate under the rule of thumb (exactly the floor), a real one under a fixed bandwidth"""
    seed, n_sim = 23, 1000
    th = np.array([[0.6, 0.2]])
    w = R.user_words(seed, 0, 0, 0, n_sim, 1)
    first = np.sort(w[:, 0].astype(np.float64))
    thr = 0.5 * (first[0] + first[1])                    # exactly one value's first word is below it
    c = np.where(w[:, 0].astype(np.float64) < thr, 2, 1)
    t = th[0, 0] + th[0, 1] * R.box_muller(w[:, 1], w[:, 2])[0]
    assert (c == 2).sum() == 1
    t2 = float(t[c == 2][0])
    e = D.HipEngine(n_groups=1, Np=4, D=2, seed=seed)
    try:
        e.set_bounds([-INF] * 2, [INF] * 2)
        oc, ox = [1, 2, 1], [0.55, t2 + 0.02, 0.7]
        e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[bw, thr], source=SRC_SECOND_CHOICE_BELOW)
        got = e.logpost(th)[0]
        want, f = C.choice_kde_loglike(c, t, oc, ox, bw)
        assert f[[0, 2]].min() >= 1e-2
        if bw == 0.0:
            assert f[1] == 0.0
        else:  # one kernel, 0.02 off its centre
            assert rel(f[1], 0.75 * (1.0 - (0.02 / bw) ** 2) / (n_sim * bw)) < 1e-9
        assert rel(got, want) <= 1e-9, (bw, got, want)
        e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack([2], [t2 + 0.02]), hyper=[bw, thr], source=SRC_SECOND_CHOICE_BELOW)
        alone = e.logpost(th)[0]
        if bw == 0.0:
            assert alone == LOG_FLOOR
        else:
            assert alone > LOG_FLOOR and rel(alone, math.log(f[1])) <= 1e-9, (alone, math.log(f[1]))
    finally:
        e.close()


def test_no_response_values_count_towards_n_only(D):
    seed, n_sim, frac = 29, 3000, 0.3
    thr = float(int(frac * 2 ** 32))
    th = np.array([[0.5, 0.15], [0.7, 0.1]])
    e = D.HipEngine(n_groups=1, Np=4, D=2, seed=seed)
    try:
        e.set_bounds([-INF] * 2, [INF] * 2)
        for r in range(2):
            w = R.user_words(seed, 0, 0, r, n_sim, 1)
            z = R.box_muller(w[:, 1], w[:, 2])[0]
            gone = w[:, 0].astype(np.float64) < thr
            c = np.where(gone, 0, np.where(z < 0.0, 1, 2))
            t = np.where(gone, np.nan, th[r, 0] + th[r, 1] * z)
            assert abs(gone.mean() - frac) < 0.05
            oc = [1, 2, 2, 1, 1, 2, 1]
            ox = [np.quantile(t[c == k], q) for k, q in zip(oc, (0.3, 0.4, 0.6, 0.7, 0.5, 0.5, 0.35))]
            for bw in (0.0, 0.05):
                e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[bw, thr], source=SRC_NO_RESPONSE_BELOW)
                got = e.logpost(th)[r]
                want, f = C.choice_kde_loglike(c, t, oc, ox, bw)
                assert f.min() >= 1e-2 and rel(got, want) <= 1e-9, (r, bw, got, want)
                # the same sample without the no-response values: every density higher by n / (n - n_0), nothing else
                keep = c > 0
                f_kept = C.choice_kde_loglike(c[keep], t[keep], oc, ox, bw)[1]
                assert np.allclose(f, f_kept * (keep.sum() / n_sim), rtol=1e-13, atol=0.0)
        # a choice outside [0, 255]: -Inf
        for bad_choice in (256.0, -1.0):
            e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack([1], [0.9]), hyper=[0.0, bad_choice], source=SRC_CHOICE_OUT_OF_RANGE)
            assert e.logpost(th)[0] == -INF
        e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack([1], [0.9]), hyper=[0.0, 255.0], source=SRC_CHOICE_OUT_OF_RANGE)
        assert np.isfinite(e.logpost(th)[0])
    finally:
        e.close()


# ---- 3. weights ----------------------------------------------------------------------------------------------------------------
def test_logpost_equals_the_weights_of_set_state(D):
    seed, n_sim, K = 9, 3000, 3
    rng = np.random.default_rng(2)
    th = lnr_rows(rng, 8, K)
    c0, t0 = C.sim_lnr([-1.0, -1.0, -1.0, 0.2], 1.0, 1, 0, 0, 0, 4000)
    oc = rng.integers(1, K + 1, 25)
    ox = np.array([np.quantile(t0[c0 == k], rng.uniform(0.4, 0.6)) for k in oc])
    e = D.HipEngine(n_groups=2, Np=4, D=K + 1, seed=seed)
    try:
        e.set_bounds([-INF] * K + [0.0], [INF] * K + [1.0])
        e.set_priors([1] * K + [4], [0.0] * K + [2.0], [3.0] * K + [3.0])
        e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[0.0, 1.0])
        e.set_state(th)
        w = e.get_state()[1]
        assert np.array_equal(w, e.logpost(th))
        for r in range(8):
            ll, f = C.choice_kde_loglike(*C.sim_lnr(th[r], 1.0, seed, 0, 0, r, n_sim), oc, ox)
            assert f.min() >= 1e-2
            lp = sum(R.log_prior(1, 0.0, 3.0, v) for v in th[r, :K]) + R.log_prior(4, 2.0, 3.0, th[r, K])
            assert rel(w[r], ll + lp) <= 1e-9, (r, w[r], ll + lp)
    finally:
        e.close()


# ---- 4. teacher-forced steps ---------------------------------------------------------------------------------------------------
def _race_data(rng, nu, tau, N):
    T = np.exp(rng.normal(np.asarray(nu), 1.0, (N, len(nu))))
    return T.argmin(1) + 1, T.min(1) + tau


def _setup_race(e, oc, ox, n_sim, hi_tau):
    e.set_model_sim(SIM_LNR, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[0.0, 1.0])
    e.set_priors([1, 1, 0], [0.0, 0.0, 0.0], [3.0, 3.0, 1.0])
    e.set_bounds([-INF, -INF, 0.0], [INF, INF, hi_tau])


def _expected_w(prop, oc, ox, hi_tau, n_sim, seed, sweep, it, slot):
    if not 0.0 <= prop[2] <= hi_tau:  # outside the bounds: -Inf (utilities.jl:92-99)
        return -INF
    ll, _ = C.choice_kde_loglike(*C.sim_lnr(prop, 1.0, seed, sweep, it, slot, n_sim), oc, ox)
    return R.log_prior(1, 0.0, 3.0, prop[0]) + R.log_prior(1, 0.0, 3.0, prop[1]) + ll


def _migrate(e, it):
    e.migration_pack_dev(it, None)  # NULL: the handle's own staging rows (single shard)
    e.migration_apply_dev(it, None)


def test_teacher_forced_steps(D):
    G, Np, n_sim, N, seed, n_it, burnin = 4, 6, 1000, 20, 20251, 30, 15
    rng = np.random.default_rng(8)
    oc, ox = _race_data(rng, (-1.0, -0.7), 0.2, N)
    hi_tau = float(ox.min())
    cfg = dict(n_groups=G, Np=Np, D=3, n_rows=n_it, seed=seed, burnin=burnin, alpha=0.3, beta=0.15, trace=1, schedule=2)
    th0 = np.stack([rng.normal(-1.0, 0.3, G * Np), rng.normal(-0.7, 0.3, G * Np), rng.uniform(0.3, 0.9, G * Np) * hi_tau], 1)
    e = D.HipEngine(**cfg)
    worst, n_dec, n_skip, n_acc, n_mig = 0.0, 0, 0, 0, 0
    try:
        _setup_race(e, oc, ox, n_sim, hi_tau)
        e.set_state(th0)
        for it in range(1, n_it + 1):
            if e.migration_due(it):
                _migrate(e, it)
                n_mig += 1
            tb, wb, _ = e.get_state()
            e.update(it, 1)
            tr = e.get_trace()
            ta, wa, _ = e.get_state()
            for s in range(G * Np):
                prop = tr["proposal"][s]
                want = _expected_w(prop, oc, ox, hi_tau, n_sim, seed, 0, it, s)
                got = tr["w_prop"][s]
                worst = max(worst, rel(got, want))
                assert rel(got, want) <= 1e-9, (it, s, got, want)
                ua = R.draw_blocks(seed, R.S_PART, 0, it, s, [3])[0]
                u = R.u53(ua[0], ua[1])
                ratio = math.exp(want - wb[s] + tr["log_adj"][s]) if want > -INF else 0.0
                n_dec += 1
                if abs(u - ratio) < 1e-7:
                    n_skip += 1
                else:
                    assert bool(tr["accepted"][s]) == (ratio >= 1.0 or u <= ratio), (it, s, u, ratio)
                if tr["accepted"][s]:
                    n_acc += 1
                    assert np.array_equal(ta[s], prop) and wa[s] == got
                else:
                    assert np.array_equal(ta[s], tb[s]) and wa[s] == wb[s]  # the resting particle keeps its noisy weight
        assert "k_sim_loglike<kde_choice,lnr> + k_accept_store" in e.last_kernels(), e.last_kernels()
        assert n_mig >= 3 and 0 < n_acc < n_dec
        assert n_skip < 0.01 * n_dec
    finally:
        e.close()
    print(f"teacher-forced: {n_dec} decisions, {n_acc} accepted, {n_skip} skipped, {n_mig} migrations, max relative difference of w' {worst:.3g}")


def test_teacher_forced_block_sweeps_address_the_sweep(D):
    G, Np, n_sim, N, seed = 3, 4, 600, 12, 607
    rng = np.random.default_rng(18)
    oc, ox = _race_data(rng, (-1.0, -0.7), 0.2, N)
    hi_tau = float(ox.min())
    e = D.HipEngine(n_groups=G, Np=Np, D=3, n_rows=6, seed=seed, burnin=3, alpha=0.3, beta=0.1, trace=1, schedule=2)
    worst = 0.0
    try:
        _setup_race(e, oc, ox, n_sim, hi_tau)
        e.set_blocks([[1, 1, 0], [0, 0, 1]])
        e.set_state(np.stack([rng.normal(-1.0, 0.3, G * Np), rng.normal(-0.7, 0.3, G * Np), rng.uniform(0.3, 0.9, G * Np) * hi_tau], 1))
        for it in range(1, 7):
            e.step(it, 1)
            tr = e.get_trace()  # of the LAST sweep of the iteration: sweep 1
            ta, wa, _ = e.get_state()
            for s in range(G * Np):
                want = _expected_w(tr["proposal"][s], oc, ox, hi_tau, n_sim, seed, 1, it, s)
                worst = max(worst, rel(tr["w_prop"][s], want))
                assert rel(tr["w_prop"][s], want) <= 1e-9, (it, s, tr["w_prop"][s], want)
                if np.isfinite(want):
                    assert rel(tr["w_prop"][s], _expected_w(tr["proposal"][s], oc, ox, hi_tau, n_sim, seed, 0, it, s)) > 1e-9  # not sweep 0's draws
                if tr["accepted"][s]:
                    assert np.array_equal(ta[s], tr["proposal"][s]) and wa[s] == tr["w_prop"][s]
    finally:
        e.close()
    print(f"block sweeps: max relative difference of w' {worst:.3g}")


# ---- 5. determinism, shards, geometry ------------------------------------------------------------------------------------------
def _run(make, n_it, th0, oc, ox, hi_tau, n_sim, sharded=False):
    e = make()
    try:
        e.each(lambda s: _setup_race(s, oc, ox, n_sim, hi_tau)) if sharded else _setup_race(e, oc, ox, n_sim, hi_tau)
        e.set_state(th0)
        e.step(1, n_it)
        return e.get_history(0, n_it) + e.get_state()
    finally:
        e.close()


def test_same_seed_same_bits_sharded_or_not(D):
    G, Np, n_sim, n_it = 4, 6, 512, 25
    rng = np.random.default_rng(44)
    oc, ox = _race_data(rng, (-1.0, -0.7), 0.2, 30)
    hi_tau = float(ox.min())
    th0 = np.stack([rng.normal(-1.0, 0.3, G * Np), rng.normal(-0.7, 0.3, G * Np), rng.uniform(0.3, 0.9, G * Np) * hi_tau], 1)
    cfg = dict(n_groups=G, Np=Np, D=3, n_rows=n_it, seed=31338, burnin=10, alpha=0.3, beta=0.1)
    ref = _run(lambda: D.HipEngine(**cfg), n_it, th0, oc, ox, hi_tau, n_sim)
    assert np.isfinite(ref[2]).all() and ref[1].sum() > 0
    for name, out in (("again", _run(lambda: D.HipEngine(**cfg), n_it, th0, oc, ox, hi_tau, n_sim)),
                      ("geometry_groups", _run(lambda: D.HipEngine(geometry_groups=64, **cfg), n_it, th0, oc, ox, hi_tau, n_sim)),
                      ("two shards", _run(lambda: D.MultiEngine(2, device_ids=[0, 0], **cfg), n_it, th0, oc, ox, hi_tau, n_sim, sharded=True))):
        for a, b in zip(ref, out):
            assert np.array_equal(a, b), name


# ---- 6. user simulators of pairs -----------------------------------------------------------------------------------------------
SRC_LNR = """
__device__ double demc_user_sim_choice(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng, int* choice) {
    double best = 0.0;
    int arg = 0;
    for (int k = 0; k < D - 1; ++k) {
        const double T = exp(theta[k] + hyper[0] * demc_sim_normal(rng));   // (two words a normal)
        if (k == 0 || T < best) { best = T; arg = k; }
    }
    *choice = arg + 1;
    return theta[D - 1] + best;
}
"""


def test_user_pair_simulator_equals_its_restatement(D):
    seed, n_sim, K, sigma = 12322, 4096, 3, 0.8
    rng = np.random.default_rng(3)
    th = lnr_rows(rng, 5, K)
    worst = 0.0
    e = D.HipEngine(n_groups=2, Np=4, D=K + 1, seed=seed, n_rows=2)
    try:
        e.set_bounds([-INF] * (K + 1), [INF] * (K + 1))
        for r in range(5):
            w = R.user_words(seed, 0, 0, r, n_sim, 2)  # six words a value: two blocks
            z = np.stack([R.box_muller(w[:, 2 * k], w[:, 2 * k + 1])[0] for k in range(K)], 1)
            c, best = C.race(np.exp(th[r, None, :K] + sigma * z))
            t = th[r, K] + best
            oc, ox = observations_in_the_bulk(rng, c, t, 40)
            e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack(oc, ox), hyper=[0.0, sigma], source=SRC_LNR)
            got = e.logpost(th)[r]
            want, f = C.choice_kde_loglike(c, t, oc, ox)
            assert f.min() >= 1e-2
            worst = max(worst, rel(got, want))
            assert rel(got, want) <= 1e-9, (r, got, want)
        e.set_state(np.tile(th[:4], (2, 1)))
        e.step(1, 1)
        assert "k_sim_loglike<kde_choice,user> + k_accept_store" in e.last_kernels(), e.last_kernels()
        with pytest.raises(D.DemcError) as err:
            e.set_model_sim(SIM_USER, KDE_CHOICE, n_sim, pack([1], [1.0]), source=SRC_LNR.replace("best = T;", "best = T +;"))
        assert err.value.code == D._ffi.EINVAL and "error" in str(err.value) and "does not compile" in str(err.value)
    finally:
        e.close()
    print(f"user pair simulator: max relative difference {worst:.3g}")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(D):
    ok = pack([1, 2], [0.5, 0.6])
    e = D.HipEngine(n_groups=1, Np=4, D=3, seed=1)
    e2 = D.HipEngine(n_groups=1, Np=4, D=2, seed=1)
    try:
        lnr = dict(simulator=SIM_LNR, estimator=KDE_CHOICE, n_sim=100, hyper=[0.0, 1.0])
        for kw, texts in ((dict(simulator=SIM_LNR, estimator=KDE, n_sim=100, data=[0.5], hyper=[0.0, 1.0]), ("DEMC_SIM_LNR", "DEMC_SIMEST_KDE_EPANECHNIKOV")),
                          (dict(simulator=SIM_LNR, estimator=FREQ, n_sim=100, data=[1.0], hyper=[0.0, 1.0]), ("DEMC_SIM_LNR", "DEMC_SIMEST_FREQUENCY")),
                          (dict(simulator=SIM_NORMAL, estimator=KDE_CHOICE, n_sim=100, data=ok), ("DEMC_SIM_NORMAL", "DEMC_SIMEST_KDE_CHOICE")),
                          (dict(simulator=SIM_BINOMIAL, estimator=KDE_CHOICE, n_sim=100, data=ok, hyper=[0.0, 10.0]), ("DEMC_SIM_BINOMIAL", "DEMC_SIMEST_KDE_CHOICE")),
                          (dict(lnr, n_sim=15001, data=ok), ("above the cap of 15000",)),
                          (dict(lnr, data=pack([1, 3], [0.5, 0.6])), ("observation 1", "[1, 2]")),
                          (dict(lnr, data=pack([0, 1], [0.5, 0.6])), ("observation 0", "[1, 2]")),
                          (dict(lnr, data=pack([1, 1.5], [0.5, 0.6])), ("observation 1", "integer")),
                          (dict(lnr, data=pack([1, 2], [0.5, INF])), ("observation 1", "not finite")),
                          (dict(lnr, data=ok, hyper=[0.0, 0.0]), ("sigma > 0",)),
                          (dict(lnr, data=ok, hyper=[0.0]), ("sigma > 0",)),
                          (dict(simulator=SIM_USER, estimator=KDE_CHOICE, n_sim=100, data=ok), ("needs hip_source",)),
                          (dict(simulator=SIM_USER, estimator=KDE_CHOICE, n_sim=100, data=pack([1, 256], [0.5, 0.6]), source=SRC_LNR), ("observation 1", "[1, 255]")),
                          (dict(simulator=SIM_LNR, estimator=KDE_CHOICE, n_sim=100, data=ok, hyper=[0.0, 1.0], source=SRC_LNR), ("registered simulator",)),
                          (dict(lnr, estimator=3, data=ok), ("unknown estimator",)),
                          (dict(lnr, simulator=3, data=ok), ("unknown simulator",))):
            with pytest.raises(D.DemcError) as err:
                e.set_model_sim(**kw)
            assert err.value.code == D._ffi.EINVAL and all(t in str(err.value) for t in texts), (texts, str(err.value))
        with pytest.raises(D.DemcError) as err:  # K = D - 1 = 1: no race
            e2.set_model_sim(SIM_LNR, KDE_CHOICE, 100, pack([1], [0.5]), hyper=[0.0, 1.0])
        assert err.value.code == D._ffi.EINVAL and "K = D - 1 in [2, 8]" in str(err.value)
        for h, d in ((e, 3), (e2, 2)):  # ... and the handle is left without a model, not with half of one
            with pytest.raises(D.DemcError):
                h.logpost(np.zeros((1, d)))
        e.set_model_sim(SIM_LNR, KDE_CHOICE, 15000, ok, hyper=[0.0, 1.0])  # the cap itself is accepted, and runs
        assert np.isfinite(e.logpost(np.array([[-1.0, -1.0, 0.1]]))[0])
    finally:
        e.close()
        e2.close()


# ---- 8. the posterior gate: probability density approximation against the closed-form log-normal race ----------------------------
def _mcse(x):
    """Monte-Carlo standard error of the mean from the split chains (chains.py's split): [n][chains]"""
    h = x.shape[0] // 2
    s = np.concatenate([x[:h], x[h:2 * h]], axis=1)
    return float(s.mean(axis=0).std(ddof=1) / math.sqrt(s.shape[1]))


def test_pda_posterior_sits_within_one_sd_of_the_lnr_family(D):
    """test/lognormal_race_tests.jl's model -- nu ~ N(0, 3), tau ~ U(0, min rt), bounds likewise -- on 100 trials of LNR(nu = (-2, -3),
    sigma = 1, tau = 0.3); the yardstick is LNRLikelihood.  The kernel smooths the leading edge of the time densities and that bias
    has no closed form: a coarse gate (one yardstick posterior sd per parameter); precision is carried by the 1e-9 tests above."""
    choice, rt = _race_data(np.random.default_rng(9918), (-2.0, -3.0), 0.3, 100)
    min_rt = float(rt.min())

    def run(loglike):
        rng = np.random.default_rng(7)
        prior = lambda: [rng.normal(0, 3, 2), rng.uniform(0, min_rt)]  # noqa: E731
        model = D.DEModel(sample_prior=prior, names=("ν", "τ"), data=(choice.astype(np.float64), rt), loglike=loglike,
                          prior_loglike=D.Priors(ν=D.Normal(0, 3), τ=D.Uniform(0.0, min_rt)))
        de = D.DE(sample_prior=prior, bounds=((-INF, INF), (0.0, min_rt)), burnin=1000, Np=12, n_groups=4)
        return D.sample(model, de, D.HIPBackend(seed=2025), 3000)

    yard = run(D.LNRLikelihood(sigma=1.0))
    pda = run(D.SimulatedLikelihood(D.SimLNR(sigma=1.0), estimator="kde_choice", n_sim=10_000))
    ym, pm, yd = yard.mean(), pda.mean(), yard.describe()
    names = [nm for nm in ym if nm not in ("acceptance", "lp")]
    assert len(names) == 3
    for ch, label in ((yard, "yardstick"), (pda, "PDA")):
        acc = float(np.mean(ch["acceptance"]))
        print(f"{label}: acceptance rate {acc:.4f}")
        assert 0.0 < acc < 1.0
    for nm in names:
        print(f"LNR PDA {nm}: yardstick mean {ym[nm]:.5f} sd {yd[nm]['std']:.5f}, PDA mean {pm[nm]:.5f}, difference {pm[nm] - ym[nm]:+.5f}, "
              f"yardstick MCSE {_mcse(yard[nm]):.5f}")
    for nm in names:
        assert math.isfinite(ym[nm]) and math.isfinite(pm[nm])
        assert abs(pm[nm] - ym[nm]) <= yd[nm]["std"], nm
