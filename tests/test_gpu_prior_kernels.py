"""Every registered prior kind INSIDE each kernel that carries a particle update, against the CPU oracle.

Six hand-written kernels each hold their own copy of "find this scalar's prior-table entry, check its bounds, add its prior
term": k_propose and its fused tails, k_res_mvn (three look-ups: the ISO instance's fixed sigma slot, the one-segment row's
register copy of entry 0 with the LDS entry handed to the out-of-line call, the many-segment nibble decode), k_res_obs,
k_longrow (span loops gated per segment by seg_plain, the scalar-per-lane and general bodies behind them) and k_frozen_sweep
(seg_fast's raw-sum form next to term()).  The fixtures of the rest of the suite put Normal, half-Cauchy, Uniform, Beta(1, 1) and
Normal-ref into these kernels and nothing else; `demc_logpost` -- where the other kinds were held to the oracle -- reaches none
of them.  prior_term itself is shared and tested there; what is under test HERE is dispatch, selection and the -Inf plumbing:
a kernel that read the wrong entry for a scalar, kept a compiled-in row length's assumptions for a non-Normal segment, ran a
span loop over a non-plain segment, or turned -Inf - (-Inf) into an accepted move would make other decisions than the oracle
(oracle/demc_oracle.c: prior_scalar / prior_loglike, which decide all of this independently).

Every case is a free run of both engines through test_gpu_production.free_run with that helper's bars: particle ids and accept
flags bit for bit, theta bit for bit at beta = 0 and to 1e-10 otherwise, log-posteriors to rtol 1e-9 in every
case.  The instance each case ran is asserted by name; the names were derived by hand from plan_lean / plan_phase / choose_form (csrc/demc_geometry.hpp) and are written into the case list.

The cases, their tables and shapes live in tests/test_prior_tables_host.py (CASES), which shows on the CPU that each of them
is evidence: the prior under test changes decisions, the run accepts, the bounds said to bite do.

The oracle has no truncated Normal.  A table that holds one goes through free_run_split: the engine gets TruncatedNormal(a, b),
the oracle Normal(a, b) with the same bounds; decisions, ids and theta are compared as above and log-posteriors after taking
sum_j log_mass(lo_j, hi_j) off the oracle's values, at the same rtol."""
import numpy as np
import pytest

import test_prior_tables_host as H
from test_gpu_production import free_run

pytestmark = pytest.mark.gpu


def configure_priors_then_bounds(eng, w):
    from demc_amd import workloads as W
    W.configure(eng, w)


def configure_bounds_then_priors(eng, w):
    eng.set_model(w["fam"], w["data"], w["dims"], w["hyper"])
    eng.set_bounds(w["lo"], w["hi"])
    eng.set_priors(w["pk"], w["pa"], w["pb"], w["pref"])
    if w["masks"] is not None:
        eng.set_blocks(w["masks"])


def free_run_split(demc, orc, w, n_it, kernels, G, Np, theta_exact, lp_rtol=1e-9, theta_rtol=1e-10, exact_kernels=None,
                   configure_engine=configure_priors_then_bounds, **cfg):
    """test_gpu_production.free_run with the two engines configured apart: the HIP engine by `configure_engine` from `w`, the
    oracle from H.for_oracle(w) (a truncated Normal as the plain one); the oracle's log-posteriors are lowered by the truncated
    Normals' log mass before they are compared.  Same bars, same order of checks: everything below the two configure calls is
    free_run's body with `+ off` on the oracle's log-posteriors, and the two must be kept in step -- a bar changed there is
    changed here."""
    from demc_amd import workloads as W
    P = G * Np
    base = dict(n_groups=G, Np=Np, D=w["D"], n_rows=n_it, schedule=2, seed=4242, burnin=n_it // 2, trace=0)
    base.update(w["engine"])
    base.update(cfg)
    off = -H.truncnormal_log_mass(w)
    eng = demc.HipEngine(**base)
    o = orc.Oracle(n_threads=8, **{k: v for k, v in base.items() if k in orc.CFG_KEYS})
    configure_engine(eng, w)
    W.configure(o, H.for_oracle(w))
    rng = np.random.default_rng(5)
    n_init = int(base.get("n_initial", 0))
    if n_init:
        rows0 = np.stack([w["init"](P, rng) for _ in range(n_init)])
        eng.set_history_rows(0, rows0)
        o.set_history_rows(0, rows0)
    th0 = w["init"](P, rng)
    eng.set_state(th0)
    o.set_state(th0)
    np.testing.assert_allclose(eng.get_state()[1], o.get_state()[1] + off, rtol=lp_rtol)
    n_run = n_it - n_init
    eng.step(1 + n_init, n_run)
    o.step(1 + n_init, n_run)
    ran = eng.last_kernels()
    for name in kernels:
        assert name in ran, f"expected {name}, the engine ran {ran}"
    if exact_kernels is not None:
        assert ran == exact_kernels, f"expected exactly {exact_kernels}, the engine ran {ran}"
    hg, ho = eng.get_history(n_init, n_it), o.get_history(n_init, n_it)
    assert np.array_equal(hg[3], ho[3]), "particle ids per slot differ (migration bookkeeping)"
    n_flip = int((hg[1] != ho[1]).sum())
    assert n_flip == 0, f"{n_flip} accept decisions differ"
    assert hg[1].mean() > 0.02, "nothing was accepted: the comparison would be vacuous"
    if theta_exact:
        assert np.array_equal(hg[0], ho[0]), "theta history is not bit-exact"
    else:
        np.testing.assert_allclose(hg[0], ho[0], rtol=theta_rtol, atol=1e-13)
    np.testing.assert_allclose(hg[2], ho[2] + off, rtol=lp_rtol)
    sg, so = eng.get_state(), o.get_state()
    assert np.array_equal(sg[2], so[2])
    np.testing.assert_allclose(sg[1], so[1] + off, rtol=lp_rtol)
    eng.close()
    o.close()
    return ran


def run_case(demc, orc, c, **split):
    from demc_amd import families as F
    w = c["make"]()
    names = dict(exact_kernels=c["kernel"], kernels=[]) if c["exact"] else dict(kernels=c["kernel"])
    if split or F.PRIOR_TRUNCNORMAL in w["pk"]:
        return free_run_split(demc, orc, w, c["n_it"], G=c["G"], Np=c["Np"], theta_exact=c["theta_exact"], lp_rtol=c["lp_rtol"], **names,
                              **split, **c["cfg"])
    return free_run(demc, orc, w, c["n_it"], G=c["G"], Np=c["Np"], theta_exact=c["theta_exact"], lp_rtol=c["lp_rtol"], **names, **c["cfg"])


def cases(prefix):
    sel = [c for c in H.CASES if c["id"].startswith(prefix)]
    assert sel
    return pytest.mark.parametrize("c", sel, ids=[c["id"] for c in sel])


def case_by_id(id):
    return next(c for c in H.CASES if c["id"] == id)


@cases("a-")
def test_res_mvn_suffstat_instances_under_every_prior_kind(demc, orc, c):
    """k_res_mvn, SUFFSTAT, two_colour: 24 observations around 0.5, 4 x 16 particles, 12 iterations across burn-in, migrations on.
    D = 8 and D = 32 with a ONE-segment table of each kind (the instances with the row length compiled in: plan_lean picks them on
    "one segment" whatever its kind; entry 0 in registers, the LDS entry to the out-of-line call; Flat: the arm that adds
    nothing); D = 12 and D = 7 with segments that straddle the lanes' four-scalar blocks and bounds of their own (the nibble
    decode: a wrong nibble is another KIND here, not another Normal); 130 particles a group (512 threads); a Gamma prior under
    open bounds with the data at 0.1, where proposals -- and a fifth of the starting rows -- leave the support while in bounds
    (-Inf from the prior, not from the bounds: a current weight of -Inf meets proposals of -Inf in the accept step)."""
    run_case(demc, orc, c)


def test_res_mvn_takes_the_table_that_arrives_last(demc, orc):
    """set_model, set_priors (all Normal: one segment but for the bounds), set_bounds, then set_priors AGAIN with the mixed D = 12
    table before set_state: demc_set_priors takes the lean plan again after every change, and the run must be the one of an
    oracle configured once"""
    c = case_by_id("a-d12-mixed-beta0.1")

    def twice(eng, w):
        eng.set_model(w["fam"], w["data"], w["dims"], w["hyper"])
        eng.set_priors([1] * w["D"], [0.0] * w["D"], [1.0] * w["D"], [0] * w["D"])
        eng.set_bounds(w["lo"], w["hi"])
        eng.set_priors(w["pk"], w["pa"], w["pb"], w["pref"])
    run_case(demc, orc, c, configure_engine=twice)


@pytest.mark.parametrize("id", ["a-d8-truncnormal-beta0.1", "a-d32-truncnormal-beta0"])
def test_truncated_normal_with_the_bounds_set_first(demc, orc, id):
    """DEMC_PRIOR_TRUNCNORMAL is folded into a Normal entry whose constant holds the mass between the bounds: the cases above set
    the priors first (demc_set_bounds re-forms the constant), these set the bounds first (demc_set_priors forms it) -- the
    same run, the same log-posteriors"""
    run_case(demc, orc, case_by_id(id), configure_engine=configure_bounds_then_priors)


@cases("b-")
def test_res_mvn_other_forms_under_non_normal_priors(demc, orc, c):
    """the other forms of k_res_mvn, one non-Normal table each.  STREAMING <256,true,8> and DIRECT <512,true,8,direct> at the shape
    of their production tests (BASELINE cfg2's data, 1030 observations, 32 x 64, 6 iterations) under Cauchy(0, 0.5), and under
    Gamma(2.5, 0.2) with the data moved to 3.  The DE-MC_Z lean body (history partners, synchronous, SUFFSTAT; HIST = 2 inside
    burn-in, 1 past it, 3 with theta_snooker = 0.1) at D = 8 with one Gamma segment and at D = 12 with the mixed table.  The ISO
    instances: MvNormal(mu, sigma^2 I) with d = 5 and sigma ~ Gamma / LogNormal / Exponential (the general row length: sigma's
    entry through the nibble decode), and workloads.mvn30 with the 30 means Cauchy(0, 1) and sigma ~ LogNormal(0, 0.5) in place
    of the reference's Cauchy+: that table is still [one entry for the 30 means | one for sigma] (n_seg = 2, the second segment
    starting at scalar 30), which is all compiled_row_length asks before it takes the D = 31 instance -- the kinds of the two
    entries are not part of the rule -- so the instance with the fixed sigma slot runs a non-Normal entry for the means through
    the one-segment arm and a LogNormal through the slot."""
    run_case(demc, orc, c)


@cases("c-")
def test_res_obs_under_every_prior_kind(demc, orc, c):
    """k_res_obs<256> at the shapes of test_lean_resident_kernel_of_the_per_observation_families, 24 iterations: Gaussian
    (4 x 10, 50 observations) with mu ~ Cauchy(0, 1) or Flat and sigma ~ Gamma(2, 0.5), Exponential(1), LogNormal(0, 0.5),
    TruncatedNormal(1, 0.5) on [0.2, 3], half-Cauchy(0, 0.5); Binomial (5 observations) with theta ~ Beta(2, 5), Beta(0.5, 0.5) -- both logarithms, one
    with a negative factor -- and Uniform(0.1, 0.9) inside the bounds [0, 1] (a tenth of the starting rows at -Inf); LNR with 3
    and 8 accumulators, nu ~ Cauchy(0, 2), tau ~ Gamma(2, 0.1), Exponential(0.2), Beta(8, 2) on [0, min_rt]."""
    run_case(demc, orc, c)


@cases("d-")
def test_propose_kernel_under_every_prior_kind(demc, orc, c):
    """k_propose's own look-up (demc_kernels.hpp: the DimTab entry per scalar).  The resident general form on MvNormal-iso, d = 5,
    SUFFSTAT, two_colour -- LEAN 1 and, with theta_snooker = 0.1, LEAN 2 -- under [Cauchy x2, Flat, Normal x2, Gamma] and under a
    second table that holds the remaining kinds (half-Cauchy, Uniform narrower than its bounds, Beta(2, 5), Exponential,
    TruncatedNormal, LogNormal).  The per-phase chain (fuse = 2, MvNormal-full d = 5, STREAMING: K1 -> k_cross_mfma -> K3), where K3
    has to carry K1's prior sum -- a -Inf included: every scalar's support is narrower than its open bounds -- into the decision.
    The resident TAIL_OBS form on the hierarchical Binomial with 40 subjects: sd_b0 ~ Gamma / LogNormal, subject segments
    [Normal-ref x15, Cauchy x10, Normal(0, 1.5) x10, Flat x5]."""
    run_case(demc, orc, c)


@cases("e-")
def test_long_row_kernels_under_non_plain_segments(demc, orc, c):
    """k_longrow<512> / <256> and k_frozen_sweep<256> / <256,big> on the hierarchical Binomial with S = 2600 subjects (the
    shortest row on which the suite reaches the span loops): sd_b0 ~ Gamma(2, 0.5), LogNormal(0, 0.5), Exponential(1), proposed by
    a single lane; subject segments [Normal-ref x1000, Cauchy(0, 1) x600, Normal(0, 1.5) x500, Flat x500] -- every border inside a
    round of 256 scalars, a non-plain segment between plain ones, so that a span region mis-gated by seg_plain, or seg_fast's
    raw-sum form taken for the Cauchy piece, shows.  Blocks [hyper ; subjects] in both orders (demc_last_kernels names the LAST
    sweep's instance), theta_snooker = 0.2, beta = 0.2, three iterations inside burn-in and three past it.  k_longrow<512>: 16 x 16
    particles; <256>: the same with geometry_groups = 512 -- with kappa = 0.9, which the row-streaming kernel has no form for (the
    general per-pair body), and on an unblocked row at kappa = 1 (the span loops of the 256-thread instance);
    k_frozen_sweep: 40 x 32, the population rule of test_row_streaming_kernel_at_the_benchmarked_row_length (640 moving particles
    per colour phase) -- it is reached at this row length, so no longer row is needed.  DE-MC_Z on both kernels (k_longrow<512> with burn-in ending
    inside the run, k_frozen_sweep<256,big> past it).  S = 2601: an odd
    row, which takes the general body throughout (k_longrow) and keeps the subject sweep away from k_frozen_sweep<256,big>."""
    run_case(demc, orc, c)
