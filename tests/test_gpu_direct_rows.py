"""DIRECT mode (loglike_mode = 2) off the headline: k_direct_mvn's whole-row body (csrc/demc_kernels.hpp, direct_mvn_rows<DP>,
DP = 8, 16, 64 -- thread per proposal, the DP values of m in registers, a row of z per trip) and every sampler path that reaches
k_direct_mvn besides the default two_colour crossover: snooker, recombination, the other proposal kinds, the sequential and
synchronous schedules, history partners, block sweeps, subset updates and shards (slot_of's glist), the three fuse modes.

What can go wrong there and nowhere else: the chunk bounds [i0, i1) of a ragged last chunk, the re-mapped (block, chunk) of a
chunk count that is a multiple of 8 on a grid whose x extent is no power of two, the zero padding of m and of the z rows up to
DP, the isotropic family's -nd log sigma - s / 2 sigma^2 behind the same sum, m = L^-1 mu~ formed on the vector pipe for
32 < d <= 64.  The log-posterior test holds the kernel to the oracle AND to the plain longdouble definition of
tests/test_direct_host.py (the oracle's MvNormal-full likelihood is the device's own whitened form).  Every test asserts by name
that k_direct_mvn<DP> is what ran."""
import numpy as np
import pytest

from conftest import make_problem, setup_engine
from test_direct_host import ROWS_TABLE, mvn_logpost_ref
from test_gpu_parity import _run_fuse_mode, teacher_forced
from test_gpu_production import free_run

pytestmark = pytest.mark.gpu

K3 = "k_accept_store"


def dp_of(d):
    """padded row length of the whitened observations (demc_set_model, csrc/demc_hip.cpp)"""
    return 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def kernel_of(d):
    return f"k_direct_mvn<{dp_of(d)}>"


# ---------------------------------------------------------------------------------------------------------------------
# log-posteriors of 600 rows: every instance, both families, against the oracle and against the plain definition
# ---------------------------------------------------------------------------------------------------------------------
# G x Np = 3 x 200: demc_logpost evaluates the 600 rows as three proposal blocks of 256, the last with 88 valid proposals;
# gridDim.x = 3 is no power of two, which the re-map's j / gridDim.x and j % gridDim.x have not seen before.
# The chunk cap is min(N / 64, 64), at least 1.  Three blocks x at most 16 chunks are fewer workgroups than one round of resident
# workgroups on any MI355X (256 CUs), so every admissible count fills the last round equally badly and chunks_filling_rounds
# (csrc/demc_geometry.hpp) returns the cap itself:
#   N = 1, 63: one chunk shorter than 64 rows;  129: chunks of 65 and 64;  575: 8 chunks of 72 rows, the last of 71, on the
#   re-mapped branch ((n_chunks & 7) == 0);  1030: 16 chunks of 65 rows, the last of 55, re-mapped.
LOGPOST_N = [1, 63, 129, 575, 1030]
_G, _NP = 3, 200
_FIXED_ROWS = [0, 255, 256, 511, 512, 599]  # the first and last proposal of every block
_refs = {}
_worst = {}


def _reference(orc, family, d, N):
    """problem, rows, the oracle's log-posteriors of all rows and the plain reference's of a sample: computed once, never changed"""
    key = (family, d, N)
    if key not in _refs:
        rng = np.random.default_rng(7000 + 100 * d + N + (50000 if family == "mvn_iso" else 0))
        prob = make_problem(family, rng, N=N, d=d)
        th = prob["init"](_G * _NP)
        o = orc.Oracle(n_groups=_G, Np=_NP, D=prob["D"], schedule=1)
        setup_engine(o, prob)
        want = o.logpost(th)
        o.close()
        rest = np.random.default_rng(d + N).choice(np.setdiff1d(np.arange(_G * _NP), _FIXED_ROWS), 14, replace=False)
        sample = np.sort(np.concatenate([_FIXED_ROWS, rest]))
        plain = mvn_logpost_ref(prob, th[sample]).astype(np.float64)
        for a in (th, want, sample, plain):
            a.setflags(write=False)
        _refs[key] = (prob, th, want, sample, plain)
    return _refs[key]


@pytest.mark.parametrize("N", LOGPOST_N)
@pytest.mark.parametrize("family,d", ROWS_TABLE)
def test_direct_rows_log_posteriors(demc, orc, family, d, N):
    prob, th, want, sample, plain = _reference(orc, family, d, N)
    e = demc.HipEngine(n_groups=_G, Np=_NP, D=prob["D"], schedule=1, loglike_mode=2)
    setup_engine(e, prob)
    got = e.logpost(th)
    ran = e.last_kernels()
    e.close()
    kernel = kernel_of(d)
    assert kernel in ran, f"expected {kernel}, the engine ran {ran}"
    assert np.isfinite(want).all() and np.isfinite(plain).all()
    vs_oracle = float(np.max(np.abs((got - want) / want)))
    vs_plain = float(np.max(np.abs((got[sample] - plain) / plain)))
    w = _worst.setdefault((kernel, family), [0.0, 0.0])
    w[0], w[1] = max(w[0], vs_oracle), max(w[1], vs_plain)
    print(f"\n{kernel} {family} d={d} N={N}: largest relative difference {vs_oracle:.2e} to the oracle (600 rows), "
          f"{vs_plain:.2e} to the plain reference ({sample.size} rows); this instance and family so far {w[0]:.2e} / {w[1]:.2e}")
    np.testing.assert_allclose(got, want, rtol=1e-9)
    np.testing.assert_allclose(got[sample], plain, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# K1 -> k_direct_mvn<DP> -> K3 free-running against the oracle, DP = 8, 16, 64
# ---------------------------------------------------------------------------------------------------------------------
# d = 5 stands for DP = 8 (D = 8 exactly is served by the lean resident DIRECT instance, k_res_mvn<512,true,8,direct>);
# 13 and 16: DP = 16, a padded and a full row; 40 and 64: DP = 64 with m = L^-1 mu~ on the vector pipe, padded and full;
# the isotropic family at d = 12 (D = 13): TAIL_PREP in K1, -nd log sigma - s / 2 sigma^2 in K3.
# 6 groups x 100 particles: 50 moving particles a group, 300 proposals a colour phase = two blocks, the second with 44.
# N = 700: 10 chunks of 70 rows on the plain (block, chunk) mapping; N = 1030: 16 chunks on the re-mapped branch.
def _k1_of(w):
    """the PLAIN K1 instance in front (as observed on an MI355X): m = L^-1 mu~ on the matrix cores for MvNormal-full up to d = 32,
    on the vector pipe above and for the isotropic family"""
    from demc_amd import families as F
    tail = "TAIL_PREP" if w["fam"] == F.FAM_MVN_ISO or w["dims"][1] > 32 else "TAIL_PREP_MFMA"
    return f"k_propose<256,true,{tail},false,true>"


def _free_run_shape(shape, N):
    from demc_amd import workloads as W
    return W.mvn30(N=N, d=12, G=6, Np=100) if shape == "iso12" else W.cfg3(N=N, d=int(shape), G=6, Np=100)


@pytest.mark.parametrize("beta", [0.0, 0.1])
@pytest.mark.parametrize("N", [700, 1030])
@pytest.mark.parametrize("shape", ["5", "13", "16", "40", "64", "iso12"])
def test_direct_rows_free_run(demc, orc, shape, N, beta):
    w = _free_run_shape(shape, N)
    d = w["dims"][1]
    ran = free_run(demc, orc, w, 8, [_k1_of(w), kernel_of(d), K3], 6, 100, theta_exact=beta == 0.0, beta=beta, loglike_mode=2)
    print(f"\nd={d} N={N} beta={beta}: {ran}")


@pytest.mark.parametrize("d", [13, 64])
def test_direct_rows_repeat_bit_for_bit(demc, d):
    """no atomics, four chains per lane added in a fixed order, the chunks' partials summed in chunk order: the same engine and
    seed on two fresh handles give the same bits in state, weights, ids and history"""
    from demc_amd import workloads as W
    w = W.cfg3(N=1030, d=d, G=6, Np=100)
    G, Np, n_it = 6, 100, 8
    th0 = w["init"](G * Np, np.random.default_rng(5))
    runs = []
    for _ in range(2):
        eng = demc.HipEngine(n_groups=G, Np=Np, D=w["D"], n_rows=n_it, schedule=2, seed=4242, burnin=n_it // 2, trace=0, beta=0.1,
                             loglike_mode=2)
        W.configure(eng, w)
        eng.set_state(th0)
        eng.step(1, n_it)
        ran = eng.last_kernels()
        assert kernel_of(d) in ran and K3 in ran, f"expected {kernel_of(d)}, the engine ran {ran}"
        runs.append(eng.get_state() + eng.get_history(0, n_it))
        eng.close()
    assert not np.array_equal(runs[0][0], th0), "nothing moved: the comparison would be vacuous"
    for i, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a, b), f"array {i}"


# ---------------------------------------------------------------------------------------------------------------------
# DIRECT through the general sampler, teacher-forced (the generator of test_gpu_edge_cases.py never draws loglike_mode 2)
# ---------------------------------------------------------------------------------------------------------------------
def _direct_fuzz_cases(n, seed=20261042):
    """as _fuzz_cases of test_gpu_edge_cases.py, for the MvNormal families in DIRECT mode: d up to 64, N up to 1100 (up to 17
    chunks), all three schedules; one case in three with history partners (DE-MC_Z: the synchronous schedule, four initial rows),
    one in three -- drawn on its own, so some carry both -- with two block sweeps [first ceil(D / 2) scalars ; the rest].
    The default seed is the first from 20261011 on whose 24 cases give every row length DP snooker, recombination, history
    partners and block sweeps, hold a case with history partners and blocks at once, the sequential schedule at all four DP, and
    three cases of 8 or 16 chunks (the re-mapped branch): chosen from the draws alone, before any of them ran."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        fam = ("mvn_full", "mvn_iso")[i % 2]
        cfg = dict(n_groups=int(rng.integers(1, 7)), Np=int(rng.integers(6, 41)), schedule=int(rng.integers(0, 3)),
                   burnin=int(rng.integers(0, 4)), theta_snooker=float(rng.choice([0.0, 0.0, 0.3, 1.0])),
                   kappa=float(rng.choice([1.0, 1.0, 0.6])), beta=float(rng.choice([0.1, 0.5])), alpha=float(rng.choice([0.1, 1.0])),
                   proposal_kind=int(rng.integers(0, 3)), seed=int(rng.integers(1, 2**31)), loglike_mode=2)
        kw = dict(N=int(rng.integers(3, 1101)), d=int(rng.integers(1, 65)))
        hist, blocks = bool(rng.integers(0, 3) == 0), bool(rng.integers(0, 3) == 0)
        if hist:
            cfg.update(partner_kind=1, schedule=1, n_initial=4)
        tag = f"{i}-{fam}-d{kw['d']}-N{kw['N']}-s{cfg['schedule']}" + ("-hist" if hist else "") + ("-blocks" if blocks else "")
        out.append(pytest.param(fam, kw, cfg, blocks, id=tag))
    return out


def run_direct_general_case(demc, orc, fam, kw, cfg, blocks):
    prob = make_problem(fam, np.random.default_rng(cfg["seed"]), **kw)
    D = prob["D"]
    masks = None
    if blocks and D >= 2:  # (a row of one scalar has no second block)
        m0 = np.zeros(D, np.uint8)
        m0[:(D + 1) // 2] = 1
        masks = np.stack([m0, 1 - m0])
    ran = teacher_forced(demc, orc, prob, n_iter=4, exact_de=False, masks=masks, **cfg)
    assert kernel_of(kw["d"]) in ran, f"expected {kernel_of(kw['d'])}, the engine ran {ran}"
    return ran


@pytest.mark.parametrize("fam,kw,cfg,blocks", _direct_fuzz_cases(24))
def test_direct_general_sampler_teacher_forced(demc, orc, fam, kw, cfg, blocks):
    """snooker, recombination, the three proposal kinds, the three schedules, history partners and block sweeps in front of
    k_direct_mvn: indices bit for bit, proposals to 1e-11, log-posteriors to 1e-9, no accept decision differs"""
    run_direct_general_case(demc, orc, fam, kw, dict(cfg), blocks)


# ---------------------------------------------------------------------------------------------------------------------
# subset updates and shards: slot_of's glist path inside k_direct_mvn
# ---------------------------------------------------------------------------------------------------------------------
# d = 13 and 40 only: D = 8 and D = 32 take the lean resident DIRECT instance, whose workgroups wait on each other, and several
# handles of that kernel must not share a device here; these populations stay on the K1 -> k_direct_mvn -> K3 chain.
# 10 groups x 8 particles, N = 300: every launch, of all groups or of a subset, is one proposal block, and the chunk count is the
# cap of 4 on every side -- the same sums in the same order, so bit equality is the bar.
_SUB = dict(G=10, Np=8, n_it=40, cfg=dict(seed=29, alpha=0.5, burnin=10, trace=0, loglike_mode=2))


def _subset_problem(d):
    prob = make_problem("mvn_full", np.random.default_rng(71 + d), N=300, d=d)
    return prob, prob["init"](_SUB["G"] * _SUB["Np"])


def _single_handle(demc, prob, th0, **extra):
    G, Np, n_it = _SUB["G"], _SUB["Np"], _SUB["n_it"]
    e = demc.HipEngine(n_groups=G, Np=Np, D=prob["D"], n_rows=n_it, schedule=2, **_SUB["cfg"], **extra)
    setup_engine(e, prob)
    e.set_state(th0)
    e.step(1, n_it)
    ran = e.last_kernels()
    out = e.get_history(0, n_it) + e.get_state()
    e.close()
    assert out[1].mean() > 0.02, "nothing was accepted: the comparison would be vacuous"
    return out, ran


@pytest.mark.parametrize("d", [13, 40])
def test_direct_rows_world_one_communicator_equals_demc_step(demc, d):
    """demc_step with a world-1 communicator, the overlapped exchange (the groups a migration did not select update as a subset,
    through glist) and demc_migration_exchange + demc_update from the host: history and state of demc_step, bit for bit"""
    G, Np, n_it = _SUB["G"], _SUB["Np"], _SUB["n_it"]
    prob, th0 = _subset_problem(d)
    ref, ran = _single_handle(demc, prob, th0)
    assert kernel_of(d) in ran and K3 in ran, ran
    for form in ("step", "overlap", "host_loop"):
        e = demc.HipEngine(n_groups=G, Np=Np, D=prob["D"], n_rows=n_it, schedule=2, **_SUB["cfg"])
        setup_engine(e, prob)
        e.set_state(th0)
        e.comm_init(demc.HipEngine.comm_unique_id(), 0, 1)
        if form == "overlap":
            e.comm_set_overlap(True)
        if form == "host_loop":
            for it in range(1, n_it + 1):
                if e.migration_due(it):
                    e.migration_exchange_enqueue(it)
                e.update(it, 1)
        else:
            e.step(1, n_it)
        st = e.comm_stats()
        assert st["world"] == 1 and st["rank"] == 0 and st["exchanges"] >= 10
        ran = e.last_kernels()
        out = e.get_history(0, n_it) + e.get_state()
        e.comm_destroy()
        e.close()
        assert kernel_of(d) in ran, f"{form}: expected {kernel_of(d)}, the engine ran {ran}"
        for i, (x, y) in enumerate(zip(ref, out)):
            assert np.array_equal(x, y), f"{form}: array {i}"


@pytest.mark.parametrize("d", [13, 40])
def test_direct_rows_two_shard_set_equals_one_handle(demc, d):
    """demc_create_multi with two shards of five groups on one device against the single handle of all ten, bit for bit"""
    G, Np, n_it = _SUB["G"], _SUB["Np"], _SUB["n_it"]
    prob, th0 = _subset_problem(d)
    ref, ran = _single_handle(demc, prob, th0, geometry_groups=G)
    assert kernel_of(d) in ran, ran
    m = demc.MultiEngine(2, device_ids=[0, 0], n_groups=G, Np=Np, D=prob["D"], n_rows=n_it, schedule=2, **_SUB["cfg"])
    m.each(lambda e: setup_engine(e, prob))
    m.set_state(th0)
    m.step(1, 20)
    m.step(21, n_it - 20)
    out = m.get_history(0, n_it) + m.get_state()
    assert all(e.comm_stats()["exchanges"] >= 10 for e in m.shards)
    rans = [e.last_kernels() for e in m.shards]
    m.close()
    for r in rans:
        assert kernel_of(d) in r, f"expected {kernel_of(d)}, a shard ran {r}"
    for i, (x, y) in enumerate(zip(ref, out)):
        assert np.array_equal(x, y), f"array {i}"


# ---------------------------------------------------------------------------------------------------------------------
# fuse modes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,d", [("mvn_full", 13), ("mvn_iso", 12)])
def test_direct_rows_fuse_modes_give_the_same_bits(demc, monkeypatch, family, d):
    """DIRECT has no fused or resident form at these row lengths: fuse = 0, 2 and 1 all run K1 -> k_direct_mvn<16> -> K3, and
    history and state agree bit for bit"""
    names = []
    close = demc.HipEngine.close

    def close_and_tell(self):  # (_run_fuse_mode closes its engine: the names are read on the way out)
        if getattr(self, "h", None):
            names.append(self.last_kernels())
        close(self)

    monkeypatch.setattr(demc.HipEngine, "close", close_and_tell)
    prob = make_problem(family, np.random.default_rng(220 + d), N=400, d=d)
    G, Np, n_it = 6, 20, 25
    th0 = prob["init"](G * Np)
    hs = [_run_fuse_mode(demc, prob, th0, fuse, G, Np, prob["D"], n_it, loglike_mode=2, theta_snooker=0.1, alpha=0.3, burnin=10)
          for fuse in (0, 2, 1)]
    assert len(names) == 3
    for ran in names:
        assert kernel_of(d) in ran and K3 in ran, f"expected {kernel_of(d)}, the engine ran {ran}"
    assert hs[0][1].mean() > 0.02, "nothing was accepted: the comparison would be vacuous"
    for other in hs[1:]:
        for i, (a, b) in enumerate(zip(hs[0], other)):
            assert np.array_equal(a, b), f"array {i}"
