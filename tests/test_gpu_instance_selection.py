"""Which kernel instance the runtime picks, by name only: the selector branches that the production and edge-case tests do not
reach.  Every case builds a tiny engine (2 groups, 64 observations), runs two iterations and compares `last_kernels()` with a
string written out here, derived by hand from the selection rules of csrc/demc_geometry.hpp:

  * workgroup: 256 threads, 512 when the moving half of a group at four lanes a particle needs more, (Np - Np/2) * 4 > 256 --
    Np = 130 is the smallest such group -- or when a particle takes 512 lanes (D >= 4096);
  * k_res_mvn's DT: the row length where an instance has it compiled in (8 and 32 with a one-segment prior table; 31 for
    MvNormal-iso with 30 means), else 0;  its HIST: 2 inside burn-in (a base row is read), 1 past it, 3 with snooker updates;
  * k_propose's LEAN: 1 for the default sampler, 2 with snooker updates, 0 with a trace (the general instance);  TILE: the group in
    LDS, never with partners from the history;  TAIL: the MvNormal preparation on the matrix cores for MvNormal-full with d <= 32
    (TAIL_PREP_MFMA), on the vector pipe for MvNormal-iso (TAIL_PREP), the subject sums of a hierarchical family (TAIL_OBS).
Nothing numerical is checked: the instances themselves are held to the oracle elsewhere."""
import numpy as np
import pytest

from conftest import make_problem, setup_engine

pytestmark = pytest.mark.gpu


def tiny_engine(demc, fam, Np, history=False, blocks=None, n_groups=2, alpha=0.0, **cfg):
    """n_groups (2) groups of Np particles on 64 observations, ready to step (with history partners: behind two prior rows, burnin = 3)"""
    prob = make_problem(fam[0], np.random.default_rng(17), **fam[1])
    P = n_groups * Np
    if history:
        cfg = dict(schedule=1, partner_kind=1, n_initial=2, burnin=3, **cfg)
    eng = demc.HipEngine(n_groups=n_groups, Np=Np, D=prob["D"], n_rows=8, seed=11, alpha=alpha, **cfg)
    setup_engine(eng, prob)
    if blocks is not None:
        eng.set_blocks(blocks)
    if history:
        eng.set_history_rows(0, np.stack([prob["init"](P) for _ in range(2)]))
    eng.set_state(prob["init"](P))
    return eng


def names_of(demc, fam, Np, history=False, blocks=None, replay=None, groups=None, **cfg):
    """the names after each of two single-iteration steps (with history partners: iterations 3 and 4 behind two prior rows, and
    burnin = 3, so that the first lies inside burn-in and the second past it); `replay`: draws handed to set_replay first;
    `groups`: the steps are subset updates of these groups"""
    eng = tiny_engine(demc, fam, Np, history, blocks, **cfg)
    if replay:
        eng.set_replay(**replay)
    first = 3 if history else 1
    out = []
    for it in (first, first + 1):
        if groups is None:
            eng.step(it, 1)
        else:
            eng.update_groups_enqueue(it, 1, groups)
            eng.synchronize()
        out.append(eng.last_kernels())
    eng.close()
    return out


def mvn(d):
    return ("mvn_full", dict(N=64, d=d))


def iso(d):
    return ("mvn_iso", dict(N=64, d=d))


@pytest.mark.parametrize("Np,wg", [(8, 256), (130, 512)])
@pytest.mark.parametrize("d,dt", [(5, 0), (8, 8), (32, 32)])
def test_lean_suffstat_instance_by_workgroup_and_row_length(demc, Np, wg, d, dt):
    """the default sampler on MvNormal-full, SUFFSTAT, two_colour: k_res_mvn<WG, false, DT>"""
    assert names_of(demc, mvn(d), Np, loglike_mode=1) == [f"k_res_mvn<{wg},false,{dt}>"] * 2


@pytest.mark.parametrize("Np,wg", [(8, 256), (130, 512)])
@pytest.mark.parametrize("fam,dt,tag", [(mvn(5), 0, ""), (mvn(8), 8, ""), (mvn(32), 32, ""), (iso(5), 0, ",iso"), (iso(30), 31, ",iso")])
def test_lean_de_mc_z_instance_by_workgroup_row_length_and_burn_in(demc, Np, wg, fam, dt, tag):
    """DE-MC_Z (history partners, synchronous) in SUFFSTAT mode: k_res_mvn<WG, false, DT, HIST[, iso]> -- HIST = 2 at iteration 3
    (burnin = 3), 1 at iteration 4, and 3 at both with snooker updates"""
    assert names_of(demc, fam, Np, history=True, loglike_mode=1) == [f"k_res_mvn<{wg},false,{dt},2{tag}>", f"k_res_mvn<{wg},false,{dt},1{tag}>"]
    assert names_of(demc, fam, Np, history=True, loglike_mode=1, theta_snooker=0.1) == [f"k_res_mvn<{wg},false,{dt},3{tag}>"] * 2


@pytest.mark.parametrize("Np,wg", [(8, 256), (130, 512)])
@pytest.mark.parametrize("cfg,lean", [(dict(trace=1), "false"), (dict(), "true"), (dict(theta_snooker=0.1), "2")])
def test_resident_instance_by_workgroup_and_lean_level(demc, Np, wg, cfg, lean):
    """the general resident form (MvNormal-iso, SUFFSTAT, two_colour: no lean kernel serves it): k_propose<WG, true, TAIL_PREP,
    true, LEAN>"""
    assert names_of(demc, iso(5), Np, loglike_mode=1, **cfg) == [f"k_propose<{wg},true,TAIL_PREP,true,{lean}>"] * 2


def test_per_phase_general_instance_with_a_tile(demc):
    """a trace on the per-phase chain (fuse = 2; STREAMING, d = 5: two k-steps per pass): the general instance over the LDS tile"""
    chain = "k_propose<256,true,TAIL_PREP_MFMA,false,false> + k_cross_mfma<2,4> + k_accept_store"
    assert names_of(demc, mvn(5), 8, loglike_mode=0, fuse=2, trace=1) == [chain] * 2


def test_per_phase_general_instance_without_a_tile(demc):
    """history partners with a trace: no tile, the general instance; SUFFSTAT fuses the whole update into K1 past burn-in, inside it
    (the base row is another workgroup's) the accept kernel follows"""
    k1 = "k_propose<256,false,TAIL_PREP_MFMA,false,false>"
    assert names_of(demc, mvn(5), 8, history=True, loglike_mode=1, trace=1) == [k1 + " + k_accept_store", k1]


@pytest.mark.parametrize("snooker,lean", [(0.0, "true"), (0.1, "2")])
def test_per_phase_lean_instances_without_a_tile(demc, snooker, lean):
    """DE-MC_Z on the STREAMING chain (the lean DE-MC_Z body is SUFFSTAT only): the no-tile lean rows of k_propose, d = 5"""
    chain = f"k_propose<256,false,TAIL_PREP_MFMA,false,{lean}> + k_cross_mfma<2,4> + k_accept_store"
    assert names_of(demc, mvn(5), 8, history=True, loglike_mode=0, theta_snooker=snooker) == [chain] * 2


def test_per_phase_instance_of_512_threads(demc):
    """a particle of D = 4096 scalars takes a whole 512-thread workgroup (hierarchical Binomial, 4094 subjects, their terms summed in
    K1: TAIL_OBS); fuse = 2 keeps the per-phase kernel where the long-row kernel would take over"""
    assert names_of(demc, ("hier_binomial", dict(S=4094)), 8, fuse=2, trace=1) == ["k_propose<512,false,TAIL_OBS,false,false>"] * 2


# ---- the rules that depend on what is known only when a step is asked for: a replay, a subset of the groups, a trace, snooker
# updates with blocks, and how many iterations one launch may carry ----

PHASE_MVN8 = "k_propose<256,true,TAIL_PREP_MFMA,false,{lean}>"  # the per-phase K1 of MvNormal-full, d = 8, over the LDS tile


def test_replay_takes_the_per_phase_chain(demc):
    """a replay disables every kernel that carries several iterations (and the lean bodies: their draws are Philox only).  MvNormal-full
    d = 8, SUFFSTAT takes k_res_mvn<256,false,8>; under a replay each colour phase is one per-phase K1 (SUFFSTAT on two_colour fuses
    the whole update into it: no likelihood or accept kernel follows), the general instance (LEAN = 0)"""
    assert names_of(demc, mvn(8), 8, loglike_mode=1) == ["k_res_mvn<256,false,8>"] * 2
    assert names_of(demc, mvn(8), 8, loglike_mode=1, replay=dict(u_step=[0.9])) == [PHASE_MVN8.format(lean="false")] * 2


def test_subset_update_leaves_the_streaming_forms(demc):
    """an update of a subset of the groups never takes a form whose workgroups wait on each other: MvNormal-full d = 8, STREAMING
    takes k_res_mvn<256,true,8> for the whole handle and the per-phase chain (lean K1 over the tile, d = 8: two k-steps per pass)
    for one group of the two -- STREAMING has no other resident form to fall back on"""
    chain = PHASE_MVN8.format(lean="true") + " + k_cross_mfma<2,4> + k_accept_store"
    assert names_of(demc, mvn(8), 8, loglike_mode=0) == ["k_res_mvn<256,true,8>"] * 2
    got = names_of(demc, mvn(8), 8, loglike_mode=0, groups=[1])
    assert got == [chain] * 2 and not any("k_res_mvn" in g or g.endswith(",true>") for g in got)


def test_subset_update_keeps_the_lean_suffstat_kernel(demc):
    """... while the forms with one independent workgroup per group serve a subset as they serve the handle: SUFFSTAT keeps
    k_res_mvn<256,false,8>"""
    assert names_of(demc, mvn(8), 8, loglike_mode=1, groups=[1]) == ["k_res_mvn<256,false,8>"] * 2


def test_de_mc_z_with_snooker_and_blocks_takes_the_per_phase_chain(demc):
    """the lean DE-MC_Z body has a snooker instance (HIST = 3) but no block sweeps: with snooker updates AND a block mask every sweep
    is a per-phase K1 without a tile, LEAN = 2 -- one kernel inside burn-in too (SUFFSTAT: the sweep-start snapshot keeps the update
    fused), never k_res_mvn<...,3>"""
    blocks = np.array([[1, 1, 1, 0, 0], [0, 0, 0, 1, 1]], np.uint8)
    assert names_of(demc, mvn(5), 8, history=True, loglike_mode=1, theta_snooker=0.1) == ["k_res_mvn<256,false,0,3>"] * 2
    assert names_of(demc, mvn(5), 8, history=True, loglike_mode=1, theta_snooker=0.1, blocks=blocks) == \
        ["k_propose<256,false,TAIL_PREP_MFMA,false,2>"] * 2


def test_trace_on_a_per_observation_family_takes_the_general_resident_kernel(demc):
    """k_res_obs serves the default sampler only; a trace is not part of it: the Gaussian model keeps the resident form (its
    per-observation terms summed in K1: TAIL_OBS) with the general instance, LEAN = 0"""
    gauss = ("gaussian", dict(N=64))
    assert names_of(demc, gauss, 8) == ["k_res_obs<256>"] * 2
    assert names_of(demc, gauss, 8, trace=1) == ["k_propose<256,true,TAIL_OBS,true,false>"] * 2


MVN8_SUFFSTAT, MVN8_STREAM = "k_res_mvn<256,false,8>", "k_propose<256,true,TAIL_PREP_MFMA,true,2,true>"


@pytest.mark.parametrize("cfg,n,cap,kernel,alpha", [
    pytest.param(dict(loglike_mode=1), 1100, 1024, MVN8_SUFFSTAT, 0.0, id=f"cfg0-1100-1024-{MVN8_SUFFSTAT}"),
    pytest.param(dict(loglike_mode=0, theta_snooker=0.1), 200, 64, MVN8_STREAM, 0.0, id=f"cfg1-200-64-{MVN8_STREAM}"),
    pytest.param(dict(loglike_mode=1), 200, 1024, MVN8_SUFFSTAT, 0.5, id="cap1024-migrating"),
    pytest.param(dict(loglike_mode=0, theta_snooker=0.1), 200, 64, MVN8_STREAM, 0.5, id="cap64-migrating"),
    pytest.param(dict(loglike_mode=1), 200, 1024, MVN8_SUFFSTAT, 0.02, id="cap1024-migrating-rarely"),
    pytest.param(dict(loglike_mode=0, theta_snooker=0.1), 200, 64, MVN8_STREAM, 0.02, id="cap64-migrating-rarely")])
def test_iterations_per_launch_follow_the_form(demc, cfg, n, cap, kernel, alpha):
    """one launch carries at most 1024 iterations, 64 where the workgroups of a group wait on each other (the streaming-resident
    forms): n iterations without a migration (demc_update, 2 groups) are ceil(n / cap) launches.  With migrations (demc_step,
    4 groups) the launches are the segments of the call (csrc/demc_schedule.hpp; DESIGN.md "The schedule of a step call"): a launch
    ends at the form's cap, in front of the next due alpha coin, or with the call.  At alpha = 0.5 the coins end every launch; at
    alpha = 0.02 (seed 11: four coins, then more than 64 iterations without one) the cap of 64 ends some and that of 1024 none.  The
    segments are counted here from eng.migration_due by that rule and asked of the host program of the CPU tests (built here
    without its sanitizers); K1 is launched once per segment and the migration kernels once per due coin."""
    import test_schedule_host as S
    migrating = alpha > 0.0
    eng = tiny_engine(demc, mvn(8), 8, n_groups=4 if migrating else 2, alpha=alpha, **cfg)
    due = [it for it in range(1, n + 1) if migrating and eng.migration_due(it)]
    eng.timing_enable()
    (eng.step if migrating else eng.update)(1, n)
    timing = eng.timing_read()
    name = eng.last_kernels()
    eng.close()
    assert name == kernel
    runs, it = [], 1
    while it <= n:  # up to the cap, to the iteration in front of the next due coin, or to the end
        run = min([cap, n + 1 - it] + [d - it for d in due if d > it][:1])
        runs.append((run, S.LOCAL if it in due else S.NONE))
        it += run
    if not migrating:
        assert len(runs) == -(-n // cap)
    elif alpha == 0.5:
        assert 60 < len(due) < 140 and len(runs) > len(due) // 2
    else:  # a migration and the cap in one call: the cap ends a launch exactly where it is 64
        assert len(due) >= 3 and n - due[-1] > 64
        assert (max(run for run, _ in runs) == cap) == (cap == 64) and (len(runs) > len(due) + 1) == (cap == 64)
    assert runs == S.segments(sanitized=False, seed=11, alpha=alpha, n_groups_total=4 if migrating else 2, n_groups=4 if migrating else 2, iter0=1, n_iters=n,
                              with_migration=migrating, cap=cap)
    assert timing["propose"]["launches"] == len(runs)
    assert timing["migration"]["launches"] == len(due)
