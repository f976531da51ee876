"""k_direct_mvn<32> keeps its lanes' slots in LDS over the row loop (csrc/demc_kernels.hpp, direct_mvn_slices: s_slot) and stores
through a per-chunk row pointer.  What can go wrong there: a slot read back by another lane than wrote it, the "no such proposal"
mark of a lane whose first proposal exists and whose second does not, a wave pair without any proposal, the partial row of a late
chunk.  test_gpu_direct_slices.py has these at grids of a few workgroups; here they are at the headline's own grid -- 128 proposal
blocks x 48 chunks, several generations of workgroups per CU, so that a workgroup finds the LDS another one left -- with the
shortest chunks that grid admits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KERNEL = "k_direct_mvn<32>"
G = 128
REF = {}   # (d, N) -> problem, theta [32768, d], sample rows, the oracle's log-posteriors of the sample (computed once, read-only)


def reference(orc, d, N):
    from conftest import make_problem, setup_engine
    if (d, N) not in REF:
        prob = make_problem("mvn_full", np.random.default_rng(1000 * d + N), N=N, d=d)
        th = prob["init"](G * 256)
        # ~600 rows: the first and the last row of the first, a middle and the last proposal block (of both population sizes), and
        # a fixed random rest
        edges = [0, 255, 63 * 256, 63 * 256 + 255, 127 * 256, 32639, 32767]
        sample = np.unique(np.concatenate([edges, np.random.default_rng(7).choice(G * 256, 600, replace=False)]))
        o = orc.Oracle(n_groups=1, Np=len(sample), D=prob["D"], schedule=1)
        setup_engine(o, prob)
        want = o.logpost(th[sample])
        o.close()
        want.setflags(write=False)
        REF[(d, N)] = (prob, th, sample, want)
    return REF[(d, N)]


# d = 17: slice 1 holds one real dimension; 32: both slices full.
# N = 3072: chunks of 64 rows (the shortest, even) on a 256-CU device; 4129: chunks of 87 rows -- an odd row peeled per chunk -- and
# a short last one.  (Another CU count gives other chunk lengths; the properties checked do not depend on them.)
# 128 x 256 = 32 768 proposals: 128 full blocks; 128 x 255 = 32 640: the last block's second half has no proposal -- lanes whose
# slots are both "none" -- and in the first half every slot exists.
@pytest.mark.parametrize("Np", [256, 255])
@pytest.mark.parametrize("N", [3072, 4129])
@pytest.mark.parametrize("d", [17, 32])
def test_direct_log_posteriors_at_the_headline_grid_match_the_oracle(demc, orc, d, N, Np):
    from conftest import setup_engine
    prob, th, sample, want = reference(orc, d, N)
    P = G * Np
    e = demc.HipEngine(n_groups=G, Np=Np, D=prob["D"], schedule=1, loglike_mode=2)
    try:
        setup_engine(e, prob)
        got = e.logpost(th[:P])
        ran = e.last_kernels()
    finally:
        e.close()
    assert KERNEL in ran, f"expected {KERNEL}, the engine ran {ran}"
    keep = sample < P
    assert keep.sum() > 500 and sample[keep][-1] == P - 1
    assert np.isfinite(want).all()
    np.testing.assert_allclose(got[sample[keep]], want[keep], rtol=1e-9)

