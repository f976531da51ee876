"""k_direct_mvn<32>'s sliced body (csrc/demc_kernels.hpp, direct_mvn_slices): a wave holds half the dimensions of twice the
proposals and asks for the next row's slice before it consumes the current one.  What can go wrong there and nowhere else: the
pairing of waves and slices, the lane's second proposal, the peeled odd row, the clamped prefetch at a chunk's end, the LDS
hand-over of the two half-sums.  Every test asserts by name that this kernel is what ran."""
import numpy as np
import pytest

from test_gpu_production import free_run

pytestmark = pytest.mark.gpu

KERNEL = "k_direct_mvn<32>"
CHAIN = ["k_propose<256,true,TAIL_PREP_MFMA,false,true>", KERNEL, "k_accept_store"]


# d = 17: slice 1 holds one real dimension and fifteen zeros; 24: half a slice; 32: both full.
# N = 64: one chunk of even length (the shortest admissible); 65: one chunk of odd length (the peeled row); 129: two chunks of
# unequal lengths (65 + 64); 2049: 32 chunks of 65 rows but the last, which has 34 and ends at the buffer's last row.
# 300 particles: two proposal blocks, the second with 44 proposals -- lanes with one valid and one invalid proposal in its first
# wave pair, and a wave pair with none.
@pytest.mark.parametrize("N", [64, 65, 129, 2049])
@pytest.mark.parametrize("d", [17, 24, 32])
def test_sliced_direct_log_posteriors_match_the_oracle(demc, orc, d, N):
    from conftest import make_problem, setup_engine
    prob = make_problem("mvn_full", np.random.default_rng(1000 * d + N), N=N, d=d)
    G, Np = 3, 100
    th = prob["init"](G * Np)
    o = orc.Oracle(n_groups=G, Np=Np, D=prob["D"], schedule=1)
    setup_engine(o, prob)
    want = o.logpost(th)
    o.close()
    e = demc.HipEngine(n_groups=G, Np=Np, D=prob["D"], schedule=1, loglike_mode=2)
    setup_engine(e, prob)
    got = e.logpost(th)
    ran = e.last_kernels()
    e.close()
    assert KERNEL in ran, f"expected {KERNEL}, the engine ran {ran}"
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-9)


# cfg3(N = 2048, G = 16) x 256 particles: a colour phase is 2048 proposals = 8 blocks, 32 chunks of 64 rows -- a chunk count that is
# a multiple of 8, the re-mapped (block, chunk) branch the headline takes.
# cfg3(N = 2050, G = 16) x 254 particles: 127 moving particles a group, 2032 proposals -- the last block ends in the middle of the
# second proposal of its fourth wave's lanes; chunks of 65 rows with a short last one.
@pytest.mark.parametrize("beta", [0.0, 0.1])
@pytest.mark.parametrize("N,Np", [(2048, 256), (2050, 254)])
def test_sliced_direct_free_run_against_the_oracle(demc, orc, N, Np, beta):
    from demc_amd import workloads as W
    w = W.cfg3(N=N, G=16)
    free_run(demc, orc, w, 8, CHAIN, 16, Np, theta_exact=beta == 0.0, beta=beta, loglike_mode=2, geometry_groups=256)


def test_sliced_direct_repeats_bit_for_bit(demc):
    """no atomics, a fixed order of the two half-sums and of the chunks: the same engine and seed on fresh handles"""
    from demc_amd import workloads as W
    w = W.cfg3(N=2050, G=16)
    G, Np, n_it = 16, 254, 6
    th0 = w["init"](G * Np, np.random.default_rng(5))
    runs = []
    for _ in range(2):
        cfg = dict(n_groups=G, Np=Np, D=w["D"], n_rows=n_it, schedule=2, seed=4242, burnin=n_it // 2, trace=0)
        cfg.update(w["engine"])
        cfg.update(beta=0.1, loglike_mode=2, geometry_groups=256)
        eng = demc.HipEngine(**cfg)
        W.configure(eng, w)
        eng.set_state(th0)
        eng.step(1, n_it)
        ran = eng.last_kernels()
        assert KERNEL in ran, f"expected {KERNEL}, the engine ran {ran}"
        runs.append(eng.get_state())
        eng.close()
    (ta, wa, ia), (tb, wb, ib) = runs
    assert not np.array_equal(ta, th0), "nothing moved: the comparison would be vacuous"
    assert np.array_equal(ta, tb) and np.array_equal(wa, wb) and np.array_equal(ia, ib)
