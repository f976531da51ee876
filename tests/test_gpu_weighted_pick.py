"""The weighted picks inside every kernel that restates them, against the exact rule of tests/weighted_pick_cases.py and against the
oracle (which tests/test_weighted_pick_host.py holds to the same rule on the CPU), at the pool sizes where a kernel changes its
code and on weights that reach its degenerate and underflowing branches.

select_base.  One engine and one oracle per case; per weight pattern one iteration inside burn-in: set_state(theta, w, ids) on
both with random distinct rows and the crafted weights, one step, then
  * the state and the history row equal the oracle's -- theta, ids and accept flags bit for bit (default-sampler crossover
    proposals: a fixed sequence of + - *), log-posteriors to 1e-9;
  * last_kernels() names the instance the case was written for;
  * the moved rows are the proposals formed HERE from the addressed draws (gammas and noise from Philox, partners from the oracle's
    trace) around the base row that exact_pick_base(pool weights, u_base(seed, iteration, sweep, global slot)) names -- accepted
    rows equal them bit for bit, rejected rows kept the old row -- and the neighbouring base rows would have given other bits.
The base patterns sit 1e6 below any log-posterior, so a proposal inside the bounds is accepted whatever it is and the state shows
the pick.  In two_colour the crafted pool is the resting colour of phase 0, Np - Np / 2 entries (the groups are odd, Np = 2 pool - 1,
so the two colours differ); phase 1 reads the weights phase 0 left, which are ordinary, and is compared with the oracle only.  In
the synchronous schedule the pool is the whole group.  No committed seed may put a uniform inside the ambiguity band.

Which pool sizes reach which code (csrc/demc_geometry.hpp; tests/geometry_host.cpp checks the limits by brute force):
  k_propose     any pool: wave_cdf<1> up to 64, <2> up to 128, <4> up to 256, the LDS form beyond; the search is a count over the
                particle's lanes, or -- with the plan stage, four lanes a particle and more -- a binary search.  All reachable.
  k_res_mvn     two_colour instances (SUFFSTAT, STREAMING, DIRECT): four lanes a particle on at most 512 threads, so the larger colour
                has at most 128 entries -- wave_cdf<4> is UNREACHABLE there; the streaming instances need one wave per SIMD (256
                threads; DIRECT at D = 8: 512 with at most 64 movers): at most 64 entries, wave_cdf<2> and <4> UNREACHABLE.  The
                DE-MC_Z instances (HIST) pick over the whole group, up to 256: all three reachable.
  k_res_obs     Np <= 512: pools up to 256, all three forms reachable; sixteen chunks is all its count can hold, and all it is handed.
  k_longrow     any pool: <1>, <4> (it has no <2>), the LDS form with a binary search beyond 256.  All reachable.
  k_frozen_sweep  registers only: plan_phase hands it pools up to 256 and k_longrow the rest; <1> and <4> reachable.
  k_mig_pack    one form (LDS, chunk16_prefix strided over 256 threads) at every size.
A uniform that lands exactly on a cumulative weight cannot be arranged in a free-running lean kernel (a 2^-53 event per draw): the
comparison operator is held on the knife edge through the replay path alone, which runs the general k_propose; the lean
restatements meet `<` against `<=` only through patterns (b) and (d), where the run of equal cumulative weights makes an
off-by-one of the count or of a size threshold visible, not the operator itself."""
import numpy as np
import pytest

import weighted_pick_cases as W
from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu

SEED = W.GPU_SEED


def _model(fam, **kw):
    return make_problem(fam, np.random.default_rng(23), **kw)


def _distinct_rows(prob, P, rng_seed):
    """random rows, no two equal in any scalar that matters: neighbouring base rows must give other proposals"""
    rng = np.random.default_rng(rng_seed)
    th = prob["init"](P)
    th[:, 0] = rng.permutation(P) / P + rng.uniform(0.0, 0.5 / P, P)  # (distinct by construction)
    assert len(np.unique(th[:, 0])) == P
    return th


def run_base_case(demc, orc, prob, kernel, G, Np, schedule, *, history=False, mask=None, cols=None, trace=False, **cfg):
    """the common procedure of the module docstring for one (kernel, pool size)"""
    assert (G, Np, schedule, history) in W.GPU_BASE_SHAPES  # (the CPU suite has held this shape's uniforms to the band)
    P, D = G * Np, prob["D"]
    pool_lo, n, _ = W.pool_of(Np, schedule)
    n_init = 2 if history else 0
    n_pat = len(W.base_patterns(n, W.SEED))
    base = dict(n_groups=G, Np=Np, D=D, n_rows=n_init + n_pat, schedule=schedule, seed=SEED, burnin=10 ** 6, alpha=0.0, beta=0.0,
                eps=0.001, n_initial=n_init, partner_kind=1 if history else 0, n_blocks=0 if mask is None else 1, trace=1 if trace else 0)
    base.update(cfg)
    eng = demc.HipEngine(**base)
    o = orc.Oracle(n_threads=4, **{k: v for k, v in base.items() if k in orc.CFG_KEYS})
    for e in (eng, o):
        setup_engine(e, prob)
        if mask is not None:
            e.set_blocks(np.asarray(mask, np.uint8)[None, :])
    if history:
        rows0 = np.stack([prob["init"](P) for _ in range(n_init)])
        eng.set_history_rows(0, rows0)
        o.set_history_rows(0, rows0)
    theta0 = _distinct_rows(prob, P, 7)
    ids = np.random.default_rng(8).permutation(P)
    cols = np.arange(D) if cols is None else np.asarray(cols)
    n_accepted = n_moved = 0
    for k in range(n_pat):
        name, it, w, gslot, b, _ = W.crafted_step(SEED, G, Np, schedule, n_init, k)
        eng.set_state(theta0, w, ids)
        o.set_state(theta0, w, ids)
        eng.step(it, 1)
        o.step(it, 1)
        ran = eng.last_kernels()
        assert ran == kernel, f"{name}: expected {kernel}, the engine ran {ran}"
        # ---- the engine against the oracle ----
        sg, so = eng.get_state(), o.get_state()
        hg, ho = eng.get_history(it - 1, it), o.get_history(it - 1, it)
        tr = o.get_trace()
        bad = np.flatnonzero((sg[0] != so[0]).any(1))
        assert bad.size == 0, (f"{name}: {bad.size} rows differ from the oracle's, first at slot {bad[0]}: oracle idx {tr['idx'][bad[0]]}, "
                               f"{sg[0][bad[0], :4]} != {so[0][bad[0], :4]}")
        assert np.array_equal(sg[2], so[2]) and np.array_equal(hg[3], ho[3]), name
        assert np.array_equal(hg[0], ho[0]) and np.array_equal(hg[1], ho[1]), name
        np.testing.assert_allclose(sg[1], so[1], rtol=1e-9, equal_nan=True, err_msg=name)
        np.testing.assert_allclose(hg[2], ho[2], rtol=1e-9, equal_nan=True, err_msg=name)
        if trace:
            assert np.array_equal(eng.get_trace()["idx"], tr["idx"]), name
        # ---- both against the exact pick: the rows that moved against the crafted pool ----
        assert (tr["idx"][gslot, 0] == 0).all()
        off = np.flatnonzero(tr["idx"][gslot, 3] != b % Np)
        assert off.size == 0, f"{name}: the oracle's base differs from the exact pick at slots {gslot[off][:5]}"
        gbase = (gslot // Np) * Np
        if history:  # partner cells (row, slot) of the history so far: cell = slot * (it - 1) + row
            hist = o.get_history(0, it - 1)[0]
            Pm, Pn = (hist[tr["idx"][gslot, c] % (it - 1), tr["idx"][gslot, c] // (it - 1)] for c in (1, 2))
        else:
            Pm, Pn = theta0[gbase + tr["idx"][gslot, 1]], theta0[gbase + tr["idx"][gslot, 2]]
        want = W.crossover_proposals(SEED, it, 0, gslot, theta0[gslot], Pm, Pn, theta0[b], base["eps"], cols, mask)
        acc = hg[1][0, gslot] != 0
        got = sg[0][gslot][:, cols]
        assert np.array_equal(got[acc], want[acc]), f"{name}: accepted rows are not the proposals around the exact base"
        assert np.array_equal(got[~acc], theta0[gslot][:, cols][~acc]), name
        for step in (-1, 1):  # the neighbouring base rows give other bits
            nb = gbase + pool_lo + np.clip(b - gbase - pool_lo + step, 0, n - 1)
            other = W.crossover_proposals(SEED, it, 0, gslot, theta0[gslot], Pm, Pn, theta0[nb], base["eps"], cols, mask)
            assert ((other != want).any(1) | (nb == b)).all(), name
        n_accepted += int(acc.sum())
        n_moved += gslot.size
    eng.close()
    o.close()
    assert n_accepted > 0.3 * n_moved, "too few accepted rows: the state would not show the picks"


POOLS = W.POOLS


@pytest.mark.parametrize("pool", POOLS)
def test_k_propose_per_phase_with_tile(demc, orc, pool):
    """the per-phase kernel over the LDS tile (fuse = 2 keeps the phase form), lean instance; Gaussian D = 2: one lane a particle, the
    search is a count over that lane"""
    run_base_case(demc, orc, _model("gaussian", N=64), "k_propose<256,true,TAIL_OBS,false,true>", 2, 2 * pool - 1, 2, fuse=2)


@pytest.mark.parametrize("pool", (5, 17, 65, 129, 257, 300))
def test_k_propose_plan_stage_binary_search(demc, orc, pool):
    """... and at four lanes a particle (MvNormal-full d = 8, SUFFSTAT: the update fused into K1) the plan stage picks the base once a
    particle, by binary search"""
    run_base_case(demc, orc, _model("mvn_full", N=64, d=8), "k_propose<256,true,TAIL_PREP_MFMA,false,true>", 2, 2 * pool - 1, 2, fuse=2,
                  loglike_mode=1)


@pytest.mark.parametrize("pool", POOLS)
def test_k_propose_without_tile_snapshot_weights(demc, orc, pool):
    """DE-MC_Z inside burn-in on the Gaussian model: partners from the history, no tile, the synchronous sweep in one launch with the
    base rows and select_base's weights read from the snapshot of the sweep's start (KParams::base_weight)"""
    run_base_case(demc, orc, _model("gaussian", N=64), "k_propose<256,false,TAIL_OBS,false,true>", 2, pool, 1, history=True)


@pytest.mark.parametrize("pool", POOLS)
def test_k_propose_resident(demc, orc, pool):
    """the general resident form (a trace keeps the lean kernel away): weights from the group's LDS copy; idx compared directly"""
    wg = 512 if pool > 256 else 256  # (a lane a particle: the larger colour on one pass of the workgroup)
    run_base_case(demc, orc, _model("gaussian", N=64), f"k_propose<{wg},true,TAIL_OBS,true,false>", 2, 2 * pool - 1, 2, trace=True)


@pytest.mark.parametrize("pool", (4, 16, 17, 64, 65, 128, 129, 256, 257, 300))
def test_k_propose_knife_edge_uniforms_replayed(demc, orc, pool):
    """the uniforms on which `<` against `<=` decides, handed to both engines through set_replay (the general per-phase kernel): idx
    of the trace against the oracle's and against the exact pick"""
    G, Np = 2, 2 * pool - 1
    P, half = G * Np, Np // 2
    n = Np - half
    prob = _model("gaussian", N=64)
    pats0 = W.base_patterns(n, W.SEED)
    base = dict(n_groups=G, Np=Np, D=2, n_rows=len(pats0), schedule=2, seed=SEED, burnin=10 ** 6, alpha=0.0, beta=0.0, trace=1)
    eng, o = demc.HipEngine(**base), orc.Oracle(**{k: v for k, v in base.items() if k in orc.CFG_KEYS})
    for e in (eng, o):
        setup_engine(e, prob)
    theta0 = _distinct_rows(prob, P, 7)
    for k, (name, _, unique) in enumerate(pats0):
        it = 1 + k
        w = W._typical(P, np.random.default_rng([k, 2])) + W.SHIFT
        for g in range(G):
            w[g * Np + half: (g + 1) * Np] = W.base_patterns(n, W.SEED + g)[k][1]
        u_part = np.full((P, 5), np.nan)
        u_part[:, 1] = np.resize(np.concatenate([W.knife_edge_uniforms(name, n), W.seeded_uniforms(n, W.SEED + it, 64)]), P)
        for e in (eng, o):
            e.set_replay(u_part=u_part)
            e.set_state(theta0, w, np.arange(P))
            e.step(it, 1)
        assert eng.last_kernels() == "k_propose<256,true,TAIL_OBS,false,false>"
        tg, to = eng.get_trace(), o.get_trace()
        assert np.array_equal(tg["idx"], to["idx"]), f"{name}: {np.flatnonzero((tg['idx'] != to['idx']).any(1))[:5]}"
        assert np.array_equal(tg["proposal"], to["proposal"]) and np.array_equal(tg["accepted"], to["accepted"]), name
        for g in range(G):
            tb = W.exact_table_base(w[g * Np + half: (g + 1) * Np])
            for p in range(half):
                s = g * Np + p
                pick = tb.pick(u_part[s, 1])
                assert W.agrees(tg["idx"][s, 3] - half, pick, unique, n), (name, s, u_part[s, 1], tg["idx"][s], pick)
    eng.close()
    o.close()


@pytest.mark.parametrize("pool", (4, 5, 15, 16, 17, 63, 64, 65, 127, 128))
def test_k_res_mvn_suffstat(demc, orc, pool):
    """the lean resident kernel, SUFFSTAT, d = 8: wave_cdf<1> up to 64 entries, <2> up to 128 -- the largest colour 512 threads carry
    at four lanes a particle; the base by a two-level count over the particle's four lanes"""
    wg = 512 if pool * 4 > 256 else 256
    run_base_case(demc, orc, _model("mvn_full", N=64, d=8), f"k_res_mvn<{wg},false,8>", 2, 2 * pool - 1, 2, loglike_mode=1)


@pytest.mark.parametrize("pool", (15, 16, 17, 64))
def test_k_res_mvn_streaming(demc, orc, pool):
    """... with the observation stream inside (STREAMING, d = 8): one wave per SIMD, so at most 64 entries"""
    run_base_case(demc, orc, _model("mvn_full", N=64, d=8), "k_res_mvn<256,true,8>", 2, 2 * pool - 1, 2, loglike_mode=0)


@pytest.mark.parametrize("pool", (15, 16, 17, 64, 65, 128, 129, 255, 256))
def test_k_res_mvn_de_mc_z_whole_group(demc, orc, pool):
    """the DE-MC_Z body inside burn-in (HIST = 2): the pool is the whole group, up to 256 entries -- wave_cdf<1>, <2> and <4>"""
    wg = 512 if (pool - pool // 2) * 4 > 256 else 256
    run_base_case(demc, orc, _model("mvn_full", N=64, d=8), f"k_res_mvn<{wg},false,8,2>", 2, pool, 1, history=True, loglike_mode=1)


@pytest.mark.parametrize("pool", (15, 16, 17, 64, 65, 128, 129, 256))
def test_k_res_obs(demc, orc, pool):
    """the lean kernel of the per-observation families (Gaussian, D = 2): wave_cdf<1>, <2>, <4>, a two-level count over sixteen lanes;
    256 entries (Np = 511) is the largest pool plan_lean admits"""
    run_base_case(demc, orc, _model("gaussian", N=64), "k_res_obs<256>", 2, 2 * pool - 1, 2)


LONG_S = 2048  # hierarchical Binomial, D = 2050: the shortest even row that takes a workgroup per particle (D >= 2048)
LONG_COLS = (0, 1, 2, 3, 4, 5, 6, 7, 1023, 1024, 2046, 2047, 2048, 2049)


@pytest.mark.parametrize("wg", (512, 256))
@pytest.mark.parametrize("pool", (64, 65, 256, 257))
def test_k_longrow(demc, orc, wg, pool):
    """the long-row kernel, one group: wave_cdf<1>, <4> and a ballot count, beyond 256 entries the LDS form and a binary search; the
    two-per-CU instance (<256>) through geometry_groups"""
    extra = dict(geometry_groups=1024) if wg == 256 else {}
    run_base_case(demc, orc, _model("hier_binomial", S=LONG_S), f"k_longrow<{wg}>", 1, 2 * pool - 1, 2, cols=LONG_COLS, **extra)


@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("pool", (64, 65, 256, 257))
def test_k_frozen_sweep_and_its_hand_over(demc, orc, big, pool):
    """the row-streaming kernel (a block sweep that freezes most of the row; geometry_groups gives the moving particles it asks for):
    <256> on the two hyper-parameters, <256,big> on the subject block; wave_cdf<1> and <4> in registers.  The same configuration at
    257 entries is k_longrow<256>'s, and is run right (Np = 514: both colours have 257 entries, so the launch last_kernels() names --
    the last one, phase 1 -- is that hand-over too; in the odd groups it is phase 1's, whose pool is one entry smaller)"""
    mask = np.zeros(LONG_S + 2, np.uint8)
    if big:
        mask[2:] = 1
    else:
        mask[:2] = 1
    kernel = "k_longrow<256>" if pool > 256 else "k_frozen_sweep<256,big>" if big else "k_frozen_sweep<256>"
    Np = 514 if pool > 256 else 2 * pool - 1
    run_base_case(demc, orc, _model("hier_binomial", S=LONG_S), kernel, 1, Np, 2, mask=mask, cols=LONG_COLS, geometry_groups=1024)


# ---- select_particle: k_mig_pack -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", (1, 300))
@pytest.mark.parametrize("Np", (4, 15, 16, 17, 64, 255, 256, 257, 600))
def test_k_mig_pack(demc, orc, Np, D):
    """one group per mirror pattern; column 0 of the packed row is the exact pick with u_mig of the global group and the oracle's, the
    row is that slot's theta, weight and id, exactly"""
    import torch
    prob = _model("binomial") if D == 1 else _model("hier_binomial", S=D - 2)
    pats = W.particle_patterns(Np, W.SEED)
    G, off, it = len(pats), 3, 5
    cfg = dict(n_groups=G, Np=Np, D=D, seed=SEED, group_offset=off, n_groups_total=G + off)
    eng, o = demc.HipEngine(**cfg), orc.Oracle(**cfg)
    for e in (eng, o):
        setup_engine(e, prob)
    theta = prob["init"](G * Np)
    w = np.concatenate([p[1] for p in pats])
    ids = np.random.default_rng(9).permutation(G * Np) + 1000
    eng.set_state(theta, w, ids)
    o.set_state(theta, w, ids)
    buf = torch.full((G, D + 3), -7.0, dtype=torch.float64, device="cuda")
    eng.migration_pack_dev(it, buf.data_ptr())
    torch.cuda.synchronize()
    rows, ref = buf.cpu().numpy(), o.migration_pack(it)
    for g, (name, wg, unique) in enumerate(pats):
        pick = W.exact_table_particle(wg).pick(W.u_mig(SEED, it, off + g))
        assert unique or not W.is_ambiguous(pick, Np), f"{name}: inside the band ({pick}); change SEED"
        assert rows[g, 0] == pick.index == ref[g, 0], f"{name}: device {rows[g, 0]}, oracle {ref[g, 0]}, exact {pick}"
        s = g * Np + pick.index
        assert np.array_equal(rows[g, 1: D + 1], theta[s]) and rows[g, D + 2] == ids[s], name
        assert np.array_equal(rows[g, D + 1: D + 2], w[s: s + 1], equal_nan=True), name
    assert np.array_equal(rows, ref, equal_nan=True)
    eng.close()
    o.close()


# ---- select_groups and the circular shift: k_mig_apply -------------------------------------------------------------------------------

def _apply_case(demc, ng, shards, it):
    import torch
    Np, D = 4, 2
    prob = _model("gaussian", N=16)
    P = ng * Np
    rng = np.random.default_rng(ng)
    theta, w, ids = prob["init"](P), rng.normal(-50.0, 3.0, P), rng.permutation(P)
    buf = torch.zeros((ng, D + 3), dtype=torch.float64, device="cuda")
    engs, lo = [], 0
    for n_loc in shards:
        e = demc.HipEngine(n_groups=n_loc, Np=Np, D=D, seed=SEED, group_offset=lo, n_groups_total=ng)
        setup_engine(e, prob)
        e.set_state(theta[lo * Np: (lo + n_loc) * Np], w[lo * Np: (lo + n_loc) * Np], ids[lo * Np: (lo + n_loc) * Np])
        e.migration_pack_dev(it, buf.data_ptr() + lo * (D + 3) * 8)
        engs.append(e)
        lo += n_loc
    torch.cuda.synchronize()
    rows = buf.cpu().numpy()
    for g in range(ng):  # the packed rows are the exact picks (ordinary weights: the patterns are test_k_mig_pack's)
        j = W.exact_pick_particle(w[g * Np: (g + 1) * Np], W.u_mig(SEED, it, g)).index
        assert rows[g, 0] == j and np.array_equal(rows[g, 1:3], theta[g * Np + j]) and rows[g, 3] == w[g * Np + j] and rows[g, 4] == ids[g * Np + j]
    got = []
    for e in engs:
        e.migration_apply_dev(it, buf.data_ptr())
        got.append(e.get_state())
        e.close()
    th_g, w_g, id_g = (np.concatenate([x[k] for x in got]) for k in range(3))
    # expected: group sel[i] receives, in the slot its own candidate left, the candidate of sel[i - 1] (circshift(particles, 1))
    sel = W.select_groups_ref(SEED, it, ng)
    th_e, w_e, id_e = theta.copy(), w.copy(), ids.copy()
    for i, g in enumerate(sel):
        src = sel[i - 1]
        s = g * Np + int(rows[g, 0])
        th_e[s], w_e[s], id_e[s] = rows[src, 1:3], rows[src, 3], int(rows[src, 4])
    assert np.array_equal(th_g, th_e) and np.array_equal(w_g, w_e) and np.array_equal(id_g, id_e)
    assert np.array_equal(np.sort(id_g), np.arange(P))
    return len(sel)


@pytest.mark.parametrize("ng", (2, 3, 5, 256, 257, 1025, 1030))
def test_k_mig_apply(demc, ng):
    """pack then apply on ordinary weights: the state is the circular shift over select_groups_ref applied to the packed rows, every
    other slot untouched bit for bit, the ids a permutation.  Beyond 1024 groups the shuffle words are drawn in a second trip of a loop
    strided by 256 threads x 4 words: an iteration that selects more than 1024 groups reads them"""
    sizes = {_apply_case(demc, ng, [ng], it) for it in (1, 2, 3)}
    assert all(2 <= s <= ng for s in sizes)
    if ng > 1024:
        assert _apply_case(demc, ng, [ng], W.iteration_selecting(SEED, ng, 1025)) >= 1025


def test_k_mig_apply_on_a_shard_pair(demc):
    """1030 groups on two handles (group_offset 0 and 515), one buffer: each packs its part and applies the rows of both"""
    it = W.iteration_selecting(SEED, 1030, 1025)
    assert _apply_case(demc, 1030, [515, 515], it) >= 1025
    _apply_case(demc, 1030, [515, 515], 1)
