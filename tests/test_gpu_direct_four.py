"""k_direct_mvn<32>x4 (csrc/demc_kernels.hpp, direct_mvn_slices<4>): the sliced DIRECT MvNormal body with FOUR proposals per
lane, a workgroup of 512 proposals, which plan_loglike (csrc/demc_geometry.hpp) takes where ceil(proposals / 512) x chunks still
reach its resident workgroups on the chip -- on 256 CUs from 6 144 proposals x 64 chunks.  What can go wrong there and nowhere
else: the lane's third and fourth proposal, the 512-entry LDS hand-over of the half-sums and slots, the (block, chunk) re-map on
a grid half as wide, a last block with a single proposal.  Chunks, row order and the chains per proposal are k_direct_mvn<32>'s,
so the two bodies must agree bit for bit.  Every test asserts by name that this instance is what ran."""
import numpy as np
import pytest

from test_gpu_production import free_run

pytestmark = pytest.mark.gpu

KERNEL = "k_direct_mvn<32>x4"
CHAIN = ["k_propose<256,true,TAIL_PREP_MFMA,false,true>", KERNEL, "k_accept_store"]


def logpost_pair(demc, orc, prob, G, Np, th, oracle=True):
    """log-posteriors of the rows th on a G x Np engine in DIRECT mode [and on the oracle], with the kernels the engine ran"""
    from conftest import setup_engine
    want = None
    if oracle:
        o = orc.Oracle(n_groups=G, Np=Np, D=prob["D"], schedule=1)
        setup_engine(o, prob)
        want = o.logpost(th)
        o.close()
    e = demc.HipEngine(n_groups=G, Np=Np, D=prob["D"], schedule=1, loglike_mode=2)
    setup_engine(e, prob)
    got = e.logpost(th)
    ran = e.last_kernels()
    e.close()
    return got, want, ran


# 6144 = 24 x 256 proposals, N = 4096: 12 blocks of 512 x 64 chunks of 64 rows -- an even length, a chunk count that is a multiple
# of 8 (the re-mapped (block, chunk) branch).  N = 4161: chunks of 66 rows, the last of 3 (the peeled odd row, the prefetch clamped
# at the buffer's end).  N = 4159: chunks of 65 rows (every chunk peels its odd row), the last of 64, ending at the buffer's last row.
# (A last chunk of ONE row -- the loop skipped, the peel only -- cannot be planned: it needs rows per chunk <= chunks, and the rule
# keeps chunks >= 64 rows and <= 64 in number; N = 63 * 64 + 1 gets 63 chunks.)
# 6145 = 1229 x 5: 13 blocks x 61 chunks -- not a multiple of 8, the plain mapping -- and the last block holds one proposal: a lane
# with one valid proposal of four, waves with none.
# d = 17: slice 1 holds one real dimension and fifteen zeros; 32: both slices full.
@pytest.mark.parametrize("G,Np,N", [(24, 256, 4096), (24, 256, 4161), (24, 256, 4159), (1229, 5, 4096)])
@pytest.mark.parametrize("d", [17, 32])
def test_four_per_lane_log_posteriors_match_the_oracle(demc, orc, d, G, Np, N):
    from conftest import make_problem
    prob = make_problem("mvn_full", np.random.default_rng(1000 * d + N + G), N=N, d=d)
    th = prob["init"](G * Np)
    got, want, ran = logpost_pair(demc, orc, prob, G, Np, th)
    assert KERNEL in ran, f"expected {KERNEL}, the engine ran {ran}"
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got, want, rtol=1e-9)


# cfg3(N = 4096, G = 48) x 256 particles: a colour phase is 48 x 128 = 6144 proposals, 12 blocks x 64 chunks
def test_four_per_lane_free_run_against_the_oracle(demc, orc):
    from demc_amd import workloads as W
    w = W.cfg3(N=4096, G=48)
    free_run(demc, orc, w, 3, CHAIN, 48, 256, theta_exact=False, beta=0.1, loglike_mode=2)


def test_four_per_lane_repeats_bit_for_bit(demc):
    """no atomics, a fixed order of the two half-sums and of the chunks: the same engine and seed on fresh handles"""
    from demc_amd import workloads as W
    w = W.cfg3(N=4096, G=48)
    G, Np, n_it = 48, 256, 3
    th0 = w["init"](G * Np, np.random.default_rng(5))
    runs = []
    for _ in range(2):
        cfg = dict(n_groups=G, Np=Np, D=w["D"], n_rows=n_it, schedule=2, seed=4242, burnin=n_it // 2, trace=0)
        cfg.update(w["engine"])
        cfg.update(beta=0.1, loglike_mode=2)
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


def test_both_bodies_give_the_same_bits(demc, orc):
    """24 x 256 = 6144 rows at N = 4096 run four per lane (12 x 64 = 768 workgroups); 22 x 256 = 5632 rows -- the most whose 11 x 64
    fat workgroups fall short of 768 -- run two per lane on the same 64 chunks (tests/direct_four_plan.cpp pins both plans).  Slot,
    chunking and per-proposal arithmetic are the same, so the rows the two engines share must agree in every bit."""
    from conftest import make_problem
    prob = make_problem("mvn_full", np.random.default_rng(32000 + 4096), N=4096, d=32)
    th = prob["init"](24 * 256)
    four, _, ran4 = logpost_pair(demc, orc, prob, 24, 256, th, oracle=False)
    two, _, ran2 = logpost_pair(demc, orc, prob, 22, 256, th[:22 * 256], oracle=False)
    assert KERNEL in ran4, f"expected {KERNEL}, the engine ran {ran4}"
    assert "k_direct_mvn<32>" in ran2 and KERNEL not in ran2, f"expected k_direct_mvn<32>, the engine ran {ran2}"
    assert np.isfinite(four).all()
    assert np.array_equal(four[:22 * 256], two)
