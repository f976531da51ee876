"""The oracle's two stabilised weighted picks (select_base_stable, select_particle_stable over cdf_fixed_order: the rule every
kernel is compared with) against the rule itself -- tests/weighted_pick_cases.py: 50-digit weights, exact cumulative sums, "first i
with C_i >= u T" -- on every weight pattern (typical, one live entry behind a run of exact zeros, ramps through the denormal
weights, equal, -Inf at the borders, all -Inf, NaN, +Inf; the mirror images for select_particle) and every pool size at which an
engine changes its code (both sides of 4, 16, 64, 128 and 256 entries, and 600).  Seeded uniforms must stay outside the ambiguity
band (zero ambiguous cases: a seed in the band is changed, not the band); the knife-edge uniforms decide `<` against `<=`.  Then
the picks in place: through Oracle.step (a two_colour phase with unequal pools, a synchronous sweep) and Oracle.migration_pack, with
the uniforms rebuilt here from Philox and the counter layout, and select_groups' partial Fisher-Yates against
Oracle.migration_plan.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import weighted_pick_cases as W
from conftest import make_problem, setup_engine


def _call(fn, w, u):
    w = np.ascontiguousarray(w, np.float64)
    return int(fn(w.ctypes.data_as(C.POINTER(C.c_double)), int(w.size), float(u)))


def _hold(fn, table, patterns, n):
    """every pattern x (200 seeded uniforms: unique, equal; the knife-edge uniforms: equal, or inside the band's two ends)"""
    for name, w, unique in patterns:
        tb = table(w)
        for u in W.seeded_uniforms(n, W.SEED):
            pick = tb.pick(u)
            assert unique or not W.is_ambiguous(pick, n), f"{name} n={n} u={u!r}: distance {pick.dist:.3g} is inside the band; change the seed"
            got = _call(fn, w, u)
            assert got == pick.index, f"{name} n={n} u={u!r}: oracle {got}, exact {pick.index} (distance {pick.dist:.3g})"
        for u in W.knife_edge_uniforms(name, n):
            pick = tb.pick(u)
            got = _call(fn, w, u)
            assert W.agrees(got, pick, unique, n), f"{name} n={n} knife-edge u={u!r}: oracle {got}, exact {pick}"


@pytest.mark.parametrize("n", W.SIZES)
def test_oracle_select_base_is_the_exact_pick(orc, n):
    _hold(orc.lib().orc_select_base, W.exact_table_base, W.base_patterns(n, W.SEED), n)


@pytest.mark.parametrize("n", W.SIZES)
def test_oracle_select_particle_is_the_exact_pick(orc, n):
    _hold(orc.lib().orc_select_particle, W.exact_table_particle, W.particle_patterns(n, W.SEED), n)


def test_equal_weights_on_the_knife_edge_take_the_lower_index(orc):
    """u = k / n on n equal weights: cdf = 1 .. n and t = k exactly, so cdf[k-1] == t and "first i with cdf[i] >= t" is k - 1 (0 for
    k = 0); `cdf[i] > t` would answer k.  Written out, apart from the exact reference"""
    for n in (2, 4, 16, 64, 128, 256):
        w = np.full(n, 3.25 + W.SHIFT)
        for k in range(n):
            want = max(k - 1, 0)
            assert _call(orc.lib().orc_select_base, w, k / n) == want == W.exact_pick_base(w, k / n).index
            assert _call(orc.lib().orc_select_particle, -w, k / n) == want == W.exact_pick_particle(-w, k / n).index


def test_degenerate_branches_as_design_states_them(orc):
    """DESIGN 3.1 / the oracle's comments: select_base falls back to min(int(u n), n - 1) when the total is not a positive finite
    number; select_particle to the first argmin over the comparable entries when any weight is -Inf or NaN or all are +Inf, else 0 --
    what the reference's own fallbacks do where both are defined (orc_select_particle_ref: findmin)"""
    L = orc.lib()
    inf, nan = np.inf, np.nan
    for w in ([-inf] * 5, [0.0, nan, 1.0, 2.0, 3.0], [0.0, inf, 1.0, 2.0, 3.0]):
        for u, want in ((0.0, 0), (0.39, 1), (0.4, 2), (0.999, 4), (1 - 2.0 ** -53, 4)):
            assert _call(L.orc_select_base, w, u) == want == W.exact_pick_base(w, u).index
    for w, want in (([3.0, nan, 1.0, 1.0, 2.0], 2), ([3.0, -inf, 1.0, -inf], 1), ([inf] * 4, 0), ([nan] * 3, 0), ([nan, inf, inf], 0),
                    ([nan, 5.0, inf], 1)):
        for u in (0.0, 0.5, 0.999):
            assert _call(L.orc_select_particle, w, u) == want == W.exact_pick_particle(w, u).index
            if not np.isnan(w[0]):  # (the restated findmin starts its walk at entry 0 and never leaves a NaN there)
                assert _call(L.orc_select_particle_ref, w, u) == want
    # one +Inf weight among finite ones is just a probability of zero, not a fallback
    assert not W.exact_table_particle([1.0, inf, 2.0]).pick(0.5).degenerate
    assert _call(L.orc_select_particle, [1.0, inf, 2.0], 0.9) == 2 == W.exact_pick_particle([1.0, inf, 2.0], 0.9).index


def test_numpy_philox_is_the_oracles(orc):
    rng = np.random.default_rng(3)
    ent, blk = rng.integers(0, 2 ** 32, 40), rng.integers(0, 2 ** 20, 40)
    for seed, it, sweep, stream in ((1, 1, 0, 3), (2 ** 40 + 77, 123456, 3, 4), (2 ** 63 + 5, 2 ** 31 + 9, 0, 1)):
        got = W.philox_blocks(seed, stream, sweep, it, ent, blk)
        for e, b, g in zip(ent, blk, got):
            assert list(g) == W._block(seed, stream, sweep, it, int(e), int(b))
    assert np.array_equal(W.u_base_array(9, 4, 1, np.arange(12)), [W.u_base(9, 4, 1, s) for s in range(12)])


def _gaussian_oracle(orc, Np, G, schedule, seed, **cfg):
    prob = make_problem("gaussian", np.random.default_rng(5), N=20)
    o = orc.Oracle(n_groups=G, Np=Np, D=2, n_rows=64, schedule=schedule, seed=seed, burnin=1000, alpha=0.0, beta=0.0, **cfg)
    setup_engine(o, prob)
    return o, prob


@pytest.mark.parametrize("schedule,Np", [(2, 33), (1, 33), (2, 131), (1, 70)])
def test_oracle_step_picks_the_exact_base(orc, schedule, Np):
    """the pick in place: idx[:, 3] of the trace after one step is pool_lo + the exact pick over the pool's weights at the phase's
    start.  An odd group (the two colour pools differ in size: 17 | 16, 66 | 65), free-running with the uniform rebuilt from Philox
    (u_base, global slots of a shard with group_offset = 3) and with replayed uniforms (seeded and knife-edge)."""
    G, off, seed = 2, 3, 77
    o, prob = _gaussian_oracle(orc, Np, G, schedule, seed, group_offset=off, n_groups_total=G + off)
    P, half = G * Np, Np // 2
    theta = prob["init"](P)
    for k, (name, _, unique) in enumerate(W.base_patterns(Np - half if schedule == 2 else Np, W.SEED)):
        it = 1 + k
        w = W._typical(P, np.random.default_rng([k, 1])) + W.SHIFT
        lo, n = (half, Np - half) if schedule == 2 else (0, Np)
        for g in range(G):
            w[g * Np + lo: g * Np + lo + n] = W.base_patterns(n, W.SEED + g)[k][1]
        for replay in (False, True):
            u_in = np.full((P, 5), np.nan)
            if replay:
                kn = W.knife_edge_uniforms(name, n)
                u_in[:, 1] = np.resize(np.concatenate([kn, W.seeded_uniforms(n, W.SEED + it, P)]), P)
                o.set_replay(u_part=u_in)
            else:
                o.set_replay()
            o.set_state(theta, w, np.arange(P))
            o.step(it, 1)
            tr = o.get_trace()
            w_after = o.get_state()[1]
            for g in range(G):
                # (two_colour) phase 0 moves [0, half) against the pool [half, Np) at its starting weights; phase 1 moves the rest
                # against [0, half) as phase 0 left it -- those slots do not move again, so their final weights are that pool
                phases = [(range(0, half), half, w[g * Np + half: (g + 1) * Np]), (range(half, Np), 0, w_after[g * Np: g * Np + half])] \
                    if schedule == 2 else [(range(Np), 0, w[g * Np: (g + 1) * Np])]
                for ph, (movers, pool_lo, pool_w) in enumerate(phases):
                    tb = W.exact_table_base(pool_w)
                    crafted = ph == 0
                    for p in movers:
                        s = g * Np + p
                        u = u_in[s, 1] if replay else W.u_base(seed, it, 0, (off + g) * Np + p)
                        pick = tb.pick(u)
                        uq = unique and crafted
                        if not replay:
                            assert uq or not W.is_ambiguous(pick, len(pool_w)), (name, s, pick)
                        assert tr["idx"][s, 0] == 0
                        assert W.agrees(tr["idx"][s, 3] - pool_lo, pick, uq, len(pool_w)), (name, replay, s, u, tr["idx"][s], pick)
    o.close()


@pytest.mark.parametrize("Np", [4, 15, 16, 17, 64, 255, 256, 257, 600])
def test_oracle_migration_pack_picks_the_exact_particle(orc, Np):
    """Oracle.migration_pack: column 0 is the exact pick over the group's weights with u_mig of the GLOBAL group; the row is that
    slot's theta, weight and id.  One group per mirror pattern."""
    pats = W.particle_patterns(Np, W.SEED)
    G, off, seed, it = len(pats), 5, 99, 7
    prob = make_problem("gaussian", np.random.default_rng(5), N=20)
    o = orc.Oracle(n_groups=G, Np=Np, D=2, seed=seed, group_offset=off, n_groups_total=G + off)
    setup_engine(o, prob)
    theta = prob["init"](G * Np)
    w = np.concatenate([p[1] for p in pats])
    ids = np.random.default_rng(1).permutation(G * Np) + 1000
    o.set_state(theta, w, ids)
    rows = o.migration_pack(it)
    for g, (name, wg, unique) in enumerate(pats):
        pick = W.exact_table_particle(wg).pick(W.u_mig(seed, it, off + g))
        assert unique or not W.is_ambiguous(pick, Np), (name, pick)
        assert rows[g, 0] == pick.index, (name, rows[g, 0], pick)
        s = g * Np + pick.index
        assert np.array_equal(rows[g, 1:3], theta[s]) and rows[g, 4] == ids[s]
        assert np.array_equal(rows[g, 3:4], w[s: s + 1], equal_nan=True)
    o.close()


@pytest.mark.parametrize("ng", [2, 3, 4, 5, 255, 256, 257, 1024, 1025, 1030])
def test_select_groups_ref_is_the_oracles_plan(orc, ng):
    """the partial Fisher-Yates of migration.jl:31-35 as DESIGN section 3 states it (ns = 2 + mulhi(w2, ng - 1); word i of blocks
    1 + i / 4 of the STEP stream), over 50 iterations: an ordered subset of 2 .. ng distinct groups"""
    seed = 2026
    cfg = orc.make_config(n_groups=ng, seed=seed)
    sel, n = np.empty(ng, np.int32), C.c_int32()
    sizes = set()
    for it in range(1, 51):
        orc.lib().orc_migration_plan(C.byref(cfg), it, sel.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n))
        ref = W.select_groups_ref(seed, it, ng)
        assert 2 <= len(ref) <= ng and len(set(ref.tolist())) == len(ref) and ref.min() >= 0 and ref.max() < ng
        assert np.array_equal(sel[: n.value], ref), (ng, it)
        sizes.add(len(ref))
    assert len(sizes) >= min(ng - 1, 6)  # (ns is spread over 2 .. ng)
    if ng >= 1025:  # (more than 1024 words: a second trip of a loop strided by 256 threads x 4 words -- one iteration in 200)
        it = W.iteration_selecting(seed, ng, 1025)
        orc.lib().orc_migration_plan(C.byref(cfg), it, sel.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n))
        assert n.value >= 1025 and np.array_equal(sel[: n.value], W.select_groups_ref(seed, it, ng))


@pytest.mark.parametrize("shape", W.GPU_BASE_SHAPES, ids=lambda s: "G%d-Np%d-s%d-%s" % (s[0], s[1], s[2], "hist" if s[3] else "cur"))
def test_gpu_cases_keep_their_uniforms_outside_the_band(orc, shape):
    """every crafted step of tests/test_gpu_weighted_pick.py, formed on the CPU: crafted_step raises on an ambiguous pick, and the
    oracle's pick on each of its uniforms is the exact one"""
    G, Np, schedule, history = shape
    pool_lo, n, movers = W.pool_of(Np, schedule)
    for k in range(len(W.base_patterns(n, W.SEED))):
        name, it, w, gslot, b, unique = W.crafted_step(W.GPU_SEED, G, Np, schedule, 2 if history else 0, k)
        u = W.u_base_array(W.GPU_SEED, it, 0, gslot)
        for s, us, bs in zip(gslot, u, b):
            g = s // Np
            assert g * Np + pool_lo + _call(orc.lib().orc_select_base, w[g * Np + pool_lo: g * Np + pool_lo + n], us) == bs, (name, s)


@pytest.mark.parametrize("Np", [4, 15, 16, 17, 64, 255, 256, 257, 600])
def test_gpu_mig_pack_cases_keep_their_uniforms_outside_the_band(Np):
    """... and the uniforms of its k_mig_pack cases (group_offset 3, iteration 5)"""
    for g, (name, wg, unique) in enumerate(W.particle_patterns(Np, W.SEED)):
        pick = W.exact_table_particle(wg).pick(W.u_mig(W.GPU_SEED, 5, 3 + g))
        assert unique or not W.is_ambiguous(pick, Np), (name, pick)
