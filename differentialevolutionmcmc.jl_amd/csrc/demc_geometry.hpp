// demc_geometry.hpp -- every launch-geometry decision of the runtime: the arithmetic that turns (configuration, model shape, facts
// about the device) into kernel instance, grid, workgroup size, LDS bytes, chunk counts and fuse flags.  Pure functions of plain
// values, host only: plain C++17, no device header, no handle, no device pointer -- the runtime gathers the inputs, asks the
// device what only it knows (occupancies), calls these, and does what the plan says.  tests/geometry_host.cpp runs them on the
// CPU under the sanitizers.
//
// The planners run on every launch: plans are stack records, nothing here allocates, and a refusal's text is a literal that is
// turned into a message only where one occurs.
#pragma once
#include "../../include/demc.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "demc_constants.hpp"  // Family, Mode, K1Tail, kFrozenMax, kMaxDynLds
#include "demc_prep.hpp"       // ModelShape, Refusal, pow2_ceil

namespace demc {

// ---- the inputs ---------------------------------------------------------------------------------------------------------------

// K1 LDS carve-up (must match k_propose): group tile (if it fits) | Np prefix sums | A^-1 [d][d] | xbar | theta' scratch
struct K1Lds {
    int ainv_lds = 1;       // A^-1 is staged in LDS (d <= 71: beside the tile; wider data read A^-1 from L2)
    bool hier_scr = false;  // hierarchical family whose theta' scratch fits in LDS: the subjects can be summed in K1
    int tile_in_lds = 0;
    size_t tile_bytes = 0, cdf_bytes = 0, ainv_bytes = 0, xbar_bytes = 0, scr_bytes = 0;
    size_t total = 0;       // the sum of the five
};

// What the rules read that does not change from one launch of an update to the next: the configuration, the model's shape, the
// prior table's run-length facts, the device, the sizing done at create / set-model time, and what is known when a step is asked
// for (a replay, an update of a subset of the groups).
struct Setup {
    const demc_config* c = nullptr;
    const ModelShape* m = nullptr;
    int family = -1;
    bool user_row = false;        // FAM_USER: the whole-row plug-in (one workgroup per proposal)
    int n_seg = 0;                // segments of the prior table (0: more than its run-length form holds)
    const int* seg_start = nullptr;
    bool normal_ref = false;      // has_normal_ref of the prior table
    bool has_hist = false;        // a history is kept
    int partial_cap = 64;         // planes of the partial-sum workspace
    int geo_groups = 0;           // groups the lane geometry is sized for (demc_config.geometry_groups, else n_groups)
    int n_cus = 0;
    int lpp = 1;                  // lanes per particle (lanes_per_particle)
    const K1Lds* k1 = nullptr;    // carve_k1_lds
    bool replay = false, subset = false;
};

inline bool is_mvn(int fam) { return fam == FAM_MVN_FULL || fam == FAM_MVN_ISO; }

// the prior table has a Normal(a, theta[ref]) entry (hierarchical scale priors), which the lean kernels do not know
inline bool has_normal_ref(const std::vector<DimTab>& tab) {
    for (const DimTab& t : tab)
        if (t.kind == PR_NORMAL_REF) return true;
    return false;
}

// ---- create-time and model-time sizing ------------------------------------------------------------------------------------------

// lanes per particle: every lane owns dim pairs {2k,2k+1}, k = sl, sl+lpp, ...  Upper end: one pair per lane (or a
// whole workgroup per particle for very long rows).  Several pairs per lane give each lane independent work to
// overlap and fewer cross-lane reduction steps, so take the FEWEST lanes (>= 4) that still (i) fill every lane of
// a pass with a particle and (ii) leave at least two workgroups per CU; small populations keep the widest split
// (measured at D = 32: 256x256 particles -> 4, 128x256 -> 8, 64x128 and below -> 16).
inline int lanes_per_particle(int D, int Np, int schedule, int geo_groups) {
    int lpp = pow2_ceil((D + 1) / 2);
    if (lpp > 64) return (D >= 4096) ? 512 : (D >= 2048) ? 256 : 64;  // a whole workgroup per particle for long rows
    // moving particles per group and launch
    const int n_act = (schedule == DEMC_SCHED_TWO_COLOUR) ? Np / 2 : (schedule == DEMC_SCHED_SEQUENTIAL) ? 1 : Np;
    for (int l = 4; l < lpp; l *= 2) {
        const int ppp = 256 / l;
        if (ppp <= n_act && (long long)geo_groups * ((n_act + ppp - 1) / ppp) >= 512) return l;
    }
    return lpp;
}

// The carve-up for a model and a population; refused when it exceeds what a launch may ask for.
inline Refusal carve_k1_lds(int family, int d, int Np, int D_, int lpp, K1Lds& o) {
    o = K1Lds();
    const size_t D = (size_t)D_;
    o.cdf_bytes = ((size_t)Np + ((size_t)Np + 15) / 16) * sizeof(double);
    o.ainv_bytes = (family == FAM_MVN_FULL) ? (size_t)d * d * sizeof(double) : 0;
    o.ainv_lds = o.ainv_bytes <= 40 * 1024 ? 1 : 0;  // d <= 71: beside the tile; wider data read A^-1 from L2
    if (!o.ainv_lds) o.ainv_bytes = 0;
    o.xbar_bytes = is_mvn(family) ? (size_t)d * sizeof(double) : 0;
    const size_t scr_rows = (size_t)(lpp >= 256 ? 1 : 256 / lpp) * (D + 2) * sizeof(double);
    const bool hier = family == FAM_HIER_BINOMIAL || family == FAM_HIER_GAUSSIAN;
    o.hier_scr = hier && scr_rows <= 96 * 1024;  // theta' of the pass fits in LDS: the subjects can be summed in K1
    const bool scr_fam = is_mvn(family) || family == FAM_GAUSSIAN || family == FAM_BINOMIAL || family == FAM_RASTRIGIN || o.hier_scr;
    o.scr_bytes = scr_fam ? scr_rows : 0;
    const size_t tile = (size_t)Np * D * sizeof(double);
    const size_t rest = o.cdf_bytes + o.ainv_bytes + o.xbar_bytes + o.scr_bytes;
    o.tile_in_lds = (tile + rest <= 96 * 1024) ? 1 : 0;
    o.tile_bytes = o.tile_in_lds ? tile : 0;
    o.total = o.tile_bytes + rest;
    if (o.total > kMaxDynLds) return Refusal{DEMC_EINVAL, "K1 LDS budget exceeded (Np too large for this D)"};
    return {};
}

// ---- tail and lean flags --------------------------------------------------------------------------------------------------------

// which tail K1 carries for this model, mode and schedule
struct TailFlags {
    bool fuse_prep = false;    // K1 computes y = A^-1 theta', a = theta'.y (MvNormal families)
    bool prep_mfma = false;    // ... on the matrix cores
    bool fuse_obs = false;     // K1 sums the per-observation terms itself
    bool fuse_accept = false;  // K1 finishes the update
    bool write_prop = true;    // K1 writes proposals to HBM (needed by K2/K3 or by the trace)
    bool cheap_obs = false;    // the likelihood is cheap enough for K1 (whether or not the phase may fuse it)
    bool pass_sx = false, pass_ainv = false;  // the kernarg carries sx / A^-1
};
inline TailFlags tail_flags(const Setup& s, int lpp, int mode, long long iter) {
    const demc_config& c = *s.c;
    const ModelShape& m = *s.m;
    const int fam = s.family;
    const bool suff = c.loglike_mode == DEMC_LOGLIKE_SUFFSTAT;
    TailFlags t;
    // K1 tails: MvNormal preparation always; the whole update when the likelihood is O(D^2) given data-only
    // statistics and a phase writes only rows that no other workgroup reads (two_colour, or the identity pass)
    t.fuse_prep = is_mvn(fam);
    t.prep_mfma = fam == FAM_MVN_FULL && lpp >= 4 && lpp <= 16 && m.d <= 32;
    t.pass_sx = t.fuse_prep && suff;
    t.pass_ainv = fam == FAM_MVN_FULL;
    // small-N scalar-data families: the sub-group of a particle sums the per-observation terms itself
    // (hierarchical families: one term per subject, i.e. O(D) like the proposal itself; their Gaussian form has p.d
    // observations behind every subject)
    const long long obs_work = (fam == FAM_HIER_GAUSSIAN) ? m.N * (m.d > 0 ? m.d : 1) : m.N;
    t.cheap_obs = ((fam == FAM_GAUSSIAN || fam == FAM_BINOMIAL || fam == FAM_RASTRIGIN) && m.N / lpp <= 512) ||
                  (s.k1->hier_scr && obs_work / lpp <= 4096);
    // nothing a moving particle reads can move in the same launch: two_colour (partners rest), the identity pass, and the
    // sequential schedule (one particle per group and launch, handled by that group's only workgroup)
    // ... and the synchronous schedule when every partner row comes from the HISTORY (resample: rows of earlier iterations,
    // which this launch does not write) and no base particle is read from the current population (random_gamma reads one
    // during burn-in only, crossover.jl:156-164): the reference's own parallel-safe scheme runs as ONE kernel
    const bool hist_private = c.schedule == DEMC_SCHED_SYNCHRONOUS && c.partner_kind == DEMC_PARTNER_HISTORY && mode == MODE_STEP &&
                              !(c.proposal_kind == 0 && iter <= c.burnin);
    const bool phase_private = c.schedule == DEMC_SCHED_TWO_COLOUR || c.schedule == DEMC_SCHED_SEQUENTIAL || mode == MODE_IDENT || hist_private;
    t.fuse_obs = t.cheap_obs && phase_private && c.fuse != 1;
    t.fuse_accept = ((t.fuse_prep && suff) || t.fuse_obs) && c.fuse != 1 && phase_private;
    t.write_prop = !t.fuse_accept || c.trace;
    return t;
}
inline int tail_of(const TailFlags& t) { return t.prep_mfma ? TAIL_PREP_MFMA : t.fuse_prep ? TAIL_PREP : t.fuse_obs ? TAIL_OBS : TAIL_NONE; }

// The default sampler and nothing else, with partners of `partner_kind`: the kernels have instances with every other branch compiled
// out.  1: the default sampler; 2: + snooker updates / block updates, their own lean instance; 0: anything else -- a trace and a
// replay among it -- takes the general instance.
// (DEMC_PARTNER_HISTORY is DE-MC_Z, sample = resample, crossover.jl:113-124: partners are cells of the history, so there is no tile,
// and the lean instances of the no-tile form serve it -- the reference's own DE-MC_Z runs use theta_snooker = 0.1,
// test/multivariate_normal_tests.jl:50-59, Examples/Hierarchical_Example.jl:103-114)
inline int lean_level(const demc_config& c, bool replay, int partner_kind, int mode = MODE_STEP) {
    const bool base = mode == MODE_STEP && c.proposal_kind == 0 && c.partner_kind == partner_kind && c.update_kind == 0 &&
                      c.fitness_kind == 0 && c.kappa == 1.0 && !c.trace && !replay;
    return !base ? 0 : (c.theta_snooker == 0.0 && c.n_blocks == 0) ? 1 : 2;
}

// {scalars inside the block, its longest run} of a block mask in run-length form (MaskRuns / KParams::mrun_*)
struct BlockSpan { int inside = 0, longest = 0; };
inline BlockSpan block_span(int n_run, unsigned in, const int* start, int D) {
    BlockSpan s;
    for (int r = 0; r < n_run; ++r)
        if ((in >> r) & 1u) {
            const int len = (r + 1 < n_run ? start[r + 1] : D) - start[r];
            s.inside += len;
            s.longest = std::max(s.longest, len);
        }
    return s;
}

// Whether this configuration can take the frozen-row sweep (k_frozen_sweep) at all: a blocked hierarchical family with long rows,
// the whole update fused, no trace, no recombination, and enough moving particles -- counted on the geometry's groups, so that a
// shard takes the form of the whole run -- for two workgroups per CU.  plan_phase refines it per sweep (the block's scalars, the
// phase's own particle count and pool); the frozen-order table and the by-product snapshot are prepared nowhere it says no.
inline bool frozen_possible(const Setup& s) {
    const demc_config& c = *s.c;
    const int n_act = c.schedule == DEMC_SCHED_TWO_COLOUR ? c.Np - c.Np / 2 : c.schedule == DEMC_SCHED_SEQUENTIAL ? 1 : c.Np;
    return (s.family == FAM_HIER_BINOMIAL || s.family == FAM_HIER_GAUSSIAN) && s.k1->hier_scr && s.lpp > 64 && c.n_blocks >= 1 &&
           c.fuse == 0 && !c.trace && c.kappa == 1.0 && (long long)s.geo_groups * n_act >= 2LL * s.n_cus;
}

// ---- the per-phase plan: K1 [-> K2 -> K3] of one sweep and colour phase ------------------------------------------------------------

// The phase: which particles move, which are partners, and what the sweeps before it left behind.
struct Phase {
    int n_groups = 0;                // groups of the launch (the subset's count under a subset update)
    int a_lo = 0, n_act = 0, pool_lo = 0, pool_n = 0, mode = MODE_STEP;
    long long iter = 0;
    int sweep = 0;
    int lpp = 1, lpp3 = 1;           // lanes per particle in K1 and in K3
    bool tile_in_lds = false;        // the group tile may be staged (K1Lds::tile_in_lds; the evaluation of given rows turns it off)
    bool live = true;                // the rows that move are the population's own (not a caller's rows under evaluation)
    bool masked = false;             // a block sweep
    int n_mrun = 1;                  // runs of its mask (0: more than kMaxMaskRun), bit r of mrun_in: run r lies inside the block
    unsigned mrun_in = 1u;
    const int* mrun_start = nullptr;
    // the by-product snapshot: allocated, and the (iteration, sweep) whose start it holds
    bool snap2 = false;
    long long snap2_iter = -1;
    int snap2_sweep = -1;
    // the frozen-order table: present, and the iterations it covers
    bool frozen_order = false;
    long long frozen_iter0 = 0;
    int frozen_iters = 0;
};

enum K1Kind { K1_PROPOSE, K1_LONGROW, K1_FROZEN };
// the sweep-start snapshot the base rows are read from: none (the live arrays), a copy of the population and its weights, a copy
// of the weights and of the block's columns only, or the by-product snapshot the sweep before left behind
enum SnapAction { SNAP_NONE, SNAP_WHOLE, SNAP_BLOCK, SNAP_REUSE };

struct PhasePlan {
    TailFlags t;                   // as launched (the snapshot turns an unfused DE-MC_Z sweep inside burn-in into a fused one)
    K1Kind kernel = K1_PROPOSE;
    // the instance: k_propose<wg, tile, tail, false, lean>, k_longrow<wg>, k_frozen_sweep<256, 3, 2, big>
    int wg = 256, tail = TAIL_NONE, lean = 0;
    bool tile = false, big = false;
    long long grid = 0;
    size_t lds = 0;
    int n_split = 1, own_in_pool = 0, tile_rows = 0, plan = 0;
    SnapAction snap = SNAP_NONE;
    bool write_snap2 = false;      // this sweep writes the by-product snapshot, for sweep + 1 of this iteration
    bool frozen_order = false;     // the groups are launched in the frozen-order table's order
    bool chain = false;            // K2 and K3 follow
    long long k3_grid = 0;
};

// `two_longrows_fit(lds)`: whether two 256-thread workgroups of k_longrow with that much dynamic LDS are resident on a CU -- asked
// only where the answer decides (the runtime asks the device once per row size).
template <typename TwoFit>
inline PhasePlan plan_phase(const Setup& s, const Phase& p, TwoFit&& two_longrows_fit) {
    const demc_config& c = *s.c;
    PhasePlan o;
    const long long n_prop = (long long)p.n_groups * p.n_act;
    o.t = tail_flags(s, p.lpp, p.mode, p.iter);
    const int wg = p.lpp > 256 ? 512 : 256;  // K1 workgroup: 512 threads when one particle takes 512 lanes
    const int ppp = wg / p.lpp, ppp3 = 256 / p.lpp3;
    const int max_split = (p.n_act + ppp - 1) / ppp;
    const int target_wgs = 512;
    int n_split = (target_wgs + p.n_groups - 1) / p.n_groups;
    if (n_split > max_split) n_split = max_split;
    if (n_split < 1) n_split = 1;
    o.n_split = n_split;
    const bool tile = p.tile_in_lds && c.partner_kind == DEMC_PARTNER_CURRENT && wg == 256;
    // plan stage (per-particle scalars once per workgroup): 4 doubles + 4 ints per particle of the workgroup's slice
    const size_t per_split = (size_t)(p.n_act + n_split - 1) / n_split;
    const size_t plan_bytes = per_split * (4 * sizeof(double) + 4 * sizeof(int));
    // tile = the partner pool, plus the workgroup's own slice of moving rows when those lie outside the pool
    o.own_in_pool = (p.a_lo >= p.pool_lo && p.a_lo + p.n_act <= p.pool_lo + p.pool_n) ? 1 : 0;
    o.tile_rows = p.pool_n + (o.own_in_pool ? 0 : (int)per_split);
    const size_t lds_no_tile = s.k1->total - s.k1->tile_bytes;
    const size_t lds_tile = lds_no_tile + (size_t)o.tile_rows * c.D * sizeof(double);  // <= K1Lds::total
    o.plan = (tile && p.mode == MODE_STEP && p.lpp >= 4 && p.lpp <= 64 && lds_tile + plan_bytes <= kMaxDynLds && !s.replay) ? 1 : 0;
    // long rows of a hierarchical family, whole update fused: the dedicated one-pass kernel (demc_longrow.hpp)
    const size_t cdf_doubles = p.pool_n > 256 ? (size_t)p.pool_n + ((size_t)p.pool_n + 15) / 16 : 0;
    const size_t lr_lds = ((((size_t)c.D + 1) & ~(size_t)1) + cdf_doubles) * sizeof(double);
    const bool lr_shape = p.lpp > 64 && s.k1->hier_scr && p.mode == MODE_STEP && !s.replay && c.fuse != 2 && s.n_seg > 0 && lr_lds <= kMaxDynLds;
    // DE-MC_Z INSIDE burn-in (Examples/Hierarchical_Example.jl:103-114 spends half its run there): random_gamma's base particle
    // (crossover.jl:156-164) is a row of the current population, which another workgroup of this synchronous launch may be writing,
    // so tail_flags left the sweep unfused (K1 -> k_hier_loglike -> K3 through the proposal buffer: 2.3x the time).  The rows
    // and weights of the sweep's START are what the synchronous schedule reads anyway: two device-to-device copies (into the
    // proposal buffers, which a fused sweep does not use) make them a snapshot nobody writes, and the sweep is ONE k_longrow
    // launch again -- base rows and select_base's weights from the snapshot (KParams::base_theta / base_weight).
    // The same holds for every family whose update fuses into K1 past burn-in (the general kernel's no-tile form reads its base
    // rows through the same two pointers): with the snapshot, DE-MC_Z is one launch per sweep inside burn-in as well as past it.
    const bool suff_mvn = o.t.fuse_prep && c.loglike_mode == DEMC_LOGLIKE_SUFFSTAT;
    bool snapshot = false, have_snap2 = false;
    if (!o.t.fuse_accept && p.mode == MODE_STEP && c.schedule == DEMC_SCHED_SYNCHRONOUS && c.partner_kind == DEMC_PARTNER_HISTORY &&
        c.proposal_kind == 0 && p.iter <= c.burnin && (o.t.cheap_obs || suff_mvn) && c.fuse == 0 && !c.trace && !s.replay && p.live) {
        // (the copies follow the choice of the kernel: a frozen sweep reads its base row at the block's scalars only)
        snapshot = true;
        o.t.fuse_obs = o.t.cheap_obs; o.t.fuse_accept = true; o.t.write_prop = false;
        // ... and when the sweep before this one was a frozen sweep over the whole population, it left this snapshot behind
        // (used once: by the sweep it was written for, in the step call that wrote it)
        if (p.snap2 && p.snap2_iter == p.iter && p.snap2_sweep == p.sweep && !s.subset) {
            snapshot = false;
            have_snap2 = true;
        }
    }
    o.snap = have_snap2 ? SNAP_REUSE : snapshot ? SNAP_WHOLE : SNAP_NONE;
    // A block sweep that FREEZES the row (the block holds a few hyper-parameters): the sweep reduced to what it is -- one pass
    // over the particle's own row, partner rows read at the block's scalars only (whole only by the one particle in ten whose
    // snooker coin fired: its projections run over the row), no LDS row, four workgroups per CU (<256>: 120 registers; three for
    // <256,big>: 155; demc_frozen.hpp) -- instead of
    // the subject-sweep machinery of k_longrow at eight waves per CU.  Partners from the population or from the history, the
    // base row from the sweep-start snapshot when there is one.
    if (frozen_possible(s) && lr_shape && o.t.fuse_obs && o.t.fuse_accept && p.masked && p.n_mrun > 0 && p.pool_n <= 256) {
        const BlockSpan blk = block_span(p.n_mrun, p.mrun_in, p.mrun_start, c.D);
        // (enough moving particles for several workgroups per CU, counted on the geometry's groups so that a shard takes the form
        // of the whole run: with one particle per CU the launch is that particle's dependent prologue whatever follows it --
        // measured on cfg4's share: no form of this kernel beats k_longrow<512> there, profiles/r05/NOTES.md)
        // (a long run inside the block -- the subject block -- takes the BIG instance: proposals formed on the fly, four scalars
        // per thread and round behind 16-byte loads, which the hierarchical Binomial family's even rows allow)
        const bool big = blk.longest > 256;
        const bool on = blk.inside >= 1 && (long long)s.geo_groups * p.n_act >= 2LL * s.n_cus &&
                        (big ? s.family == FAM_HIER_BINOMIAL && (c.D & 1) == 0 : blk.inside <= kFrozenMax);
        if (on) {
            if (snapshot) o.snap = SNAP_BLOCK;
            o.frozen_order = !s.subset && p.frozen_order && p.iter >= p.frozen_iter0 && p.iter < p.frozen_iter0 + p.frozen_iters &&
                             p.sweep < c.n_blocks;
            // the next sweep of this iteration will want a snapshot of its start as well: this sweep writes it on its way (every
            // row passes through the kernel once) -- when it moves the whole population and does not itself read the buffer
            // (allocated when the model and the blocks are known, never inside an enqueued step)
            const int n_sweeps = c.n_blocks > 0 ? c.n_blocks : 1;
            o.write_snap2 = !big && snapshot && !have_snap2 && p.sweep + 1 < n_sweeps && !s.subset && p.a_lo == 0 && p.n_act == c.Np &&
                            p.n_groups == c.n_groups && p.snap2;
            o.kernel = K1_FROZEN; o.wg = 256; o.big = big; o.grid = n_prop; o.lds = 0;
            return o;
        }
    }
    if (lr_shape && o.t.fuse_obs && o.t.fuse_accept) {
        // Enough moving particles for two workgroups per CU (counted on the geometry's groups, so that a shard takes the
        // same form as the whole run): 256 threads each -- one wave per SIMD per workgroup, two particles per CU out of
        // step, one's prologue and row moves under the other's pass -- when two rows fit in the CU's LDS.
        const bool two_per_cu = (long long)s.geo_groups * p.n_act >= 2LL * s.n_cus && two_longrows_fit(lr_lds);
        const int wg_lr = two_per_cu ? 256 : 512;
        // persistent: as many workgroups as are resident at once, each takes particles blockIdx.x, + gridDim.x, ... (the
        // row moves of one particle then run inside the span loops of the next: demc_longrow.hpp).  A multiple of 8 keeps
        // a workgroup's particles on its own XCD (the kernel's blockIdx -> group mapping).
        long long grid_lr = (long long)(wg_lr == 512 ? 1 : 2) * s.n_cus;
        if (grid_lr > n_prop || grid_lr < 1) grid_lr = n_prop;
        if ((p.n_groups & 7) == 0 && grid_lr >= 8) grid_lr &= ~7LL;
        o.kernel = K1_LONGROW; o.wg = wg_lr; o.grid = grid_lr; o.lds = lr_lds;
        return o;
    }
    // LEAN: the general instance (0), the default sampler (1), + snooker / block updates (2) -- without a tile for partners from the
    // history (DE-MC_Z); a 512-thread workgroup per particle (very long rows, no tile) has the general instance only
    o.kernel = K1_PROPOSE; o.wg = wg; o.tile = tile; o.tail = tail_of(o.t);
    o.lean = wg == 256 ? lean_level(c, s.replay, tile ? DEMC_PARTNER_CURRENT : DEMC_PARTNER_HISTORY, p.mode) : 0;
    o.grid = (long long)p.n_groups * n_split;
    o.lds = tile ? lds_tile + (o.plan ? plan_bytes : 0) : lds_no_tile;
    o.chain = !o.t.fuse_accept;
    o.k3_grid = (n_prop + ppp3 - 1) / ppp3;
    return o;
}

// ---- the K2 plan ----------------------------------------------------------------------------------------------------------------

// Number of observation chunks for a K2 kernel that is one long uniform loop per workgroup: such a launch takes
// ceil(workgroups / resident workgroups) rounds of equal length, so among the admissible counts (1..cap) the one that fills
// the last round best wins; ties go to the larger count while the launch stays within four rounds.
inline int chunks_filling_rounds(long long blocks, long long cap, double resident_wgs) {
    long long best = 1;
    double best_fill = 0.0;
    for (long long nc = 1; nc <= cap; ++nc) {
        const double wgs = (double)blocks * (double)nc;
        const double fill = wgs / (std::ceil(wgs / resident_wgs) * resident_wgs);
        if (fill > best_fill + 1e-9 || (fill > best_fill - 1e-9 && wgs <= 4.0 * resident_wgs)) { best = nc; best_fill = fill; }
    }
    return (int)best;
}

// the likelihood kernel behind K1 (none: fused into K1, or MvNormal SUFFSTAT, whose statistic K1 formed).  K2_SIM and K2_ODE have
// nothing to plan -- one workgroup per proposal, one thread per proposal -- and are launched by the runtime on its own.
enum K2Kind { K2_NONE, K2_CROSS_MFMA, K2_DIRECT_MVN, K2_OBS, K2_LBA_WAVE, K2_HIER, K2_USER, K2_USER_ROW, K2_SIM, K2_ODE };

// resident 256-thread workgroups per CU of k_direct_mvn<DP>, k_obs_loglike and k_lba_wave<3>: only the one the kind reads need be set
// (direct4: of k_direct_mvn_x4<DP>, 0 where the library has no such instance for the row length)
struct Occupancy { int direct = 0, obs = 0, lba_wave = 0, direct4 = 0; };

struct LoglikePlan {
    K2Kind kind = K2_NONE;
    int key[2] = {0, 0};        // the instance: k_direct_mvn<key[0]> (key[1] = 4: k_direct_mvn_x4), k_cross_mfma<key[0], key[1]>, k_lba_wave<key[0]>
    unsigned grid_x = 0, grid_y = 1;
    int n_chunks = 1, n_partials = 1;
    int n_kpass = 1, k0_stride = 0, part0_stride = 0;  // k_cross_mfma: pass kp starts at dimension kp * k0_stride, partial plane kp * part0_stride
    int refused = DEMC_OK;      // ... with this text
    const char* why = nullptr;
};

inline K2Kind k2_kind(const Setup& s) {
    switch (s.family) {
        case FAM_MVN_FULL:
        case FAM_MVN_ISO:
            return s.c->loglike_mode == DEMC_LOGLIKE_DIRECT ? K2_DIRECT_MVN : s.c->loglike_mode == DEMC_LOGLIKE_SUFFSTAT ? K2_NONE : K2_CROSS_MFMA;
        case FAM_GAUSSIAN:
        case FAM_BINOMIAL:
        case FAM_LNR:
        case FAM_RASTRIGIN: return K2_OBS;
        case FAM_LBA: return K2_LBA_WAVE;
        case FAM_USER: return s.user_row ? K2_USER_ROW : K2_USER;
        case FAM_HIER_BINOMIAL:
        case FAM_HIER_GAUSSIAN: return K2_HIER;
        default: return K2_NONE;
    }
}

// K2 for n_prop > 0 proposals of a family in the switch above (any other: refused)
inline LoglikePlan plan_loglike(const Setup& s, long long n_prop, const Occupancy& occ) {
    const ModelShape& m = *s.m;
    LoglikePlan o;
    o.kind = k2_kind(s);
    switch (o.kind) {
        case K2_DIRECT_MVN: {
            // proposal blocks of 256 x observation chunks: enough workgroups for 8 waves per SIMD, chunks no shorter
            // than 64 observations, at most the partial-sum workspace
            const long long blocks = (n_prop + 255) / 256;
            long long cap = m.N / 64;
            if (cap > s.partial_cap) cap = s.partial_cap;
            if (cap < 1) cap = 1;
            // The kernel is one long uniform loop per workgroup: the launch takes ceil(workgroups / resident workgroups)
            // rounds of equal length, so the chunk count is chosen to fill the last round (cfg3: 128 blocks x 48 chunks =
            // 4 full rounds of 1536 resident workgroups; 32 chunks would leave a third of the device idle in round 3).
            o.key[0] = m.dp_direct;
            o.n_chunks = chunks_filling_rounds(blocks, cap, (double)occ.direct * s.n_cus);
            o.grid_x = (unsigned)blocks; o.grid_y = (unsigned)o.n_chunks;
            o.n_partials = o.n_chunks;
            // The body is chosen AFTER the chunks, which alone fix the sums: four proposals per lane (blocks of 512, occ.direct4
            // resident workgroups per CU) where half as many workgroups still give every CU its resident count; an under-filled
            // device keeps the thinner ones.  (cfg3: 64 blocks x 48 chunks = 4 x 768.)
            const long long blocks4 = (n_prop + 511) / 512;
            if (m.dp_direct == 32 && occ.direct4 > 0 && blocks4 * o.n_chunks >= (long long)occ.direct4 * s.n_cus) {
                o.key[1] = 4;
                o.grid_x = (unsigned)blocks4;
            }
        } break;
        case K2_CROSS_MFMA: {
            // (k-steps per pass: the next instance up, the model's preparation keeps them a power of two <= 16)
            o.key[0] = m.ks_t <= 1 ? 1 : m.ks_t <= 2 ? 2 : m.ks_t <= 4 ? 4 : m.ks_t <= 8 ? 8 : 16;
            o.key[1] = 4;
            // particle tiles of 256 (4 waves x MT=4 x 16) x observation chunks; chunks in multiples of 8 so that
            // blockIdx % 8 (the XCD a block lands on) selects the chunk it streams
            const long long n_ptiles = (n_prop + 255) / 256;
            int n_chunks = 8;
            while (n_ptiles * n_chunks < 1024 && n_chunks * 2 <= 32 && m.n_tiles / (n_chunks * 2) >= 16) n_chunks *= 2;
            if (m.n_tiles < n_chunks) n_chunks = (int)(m.n_tiles > 0 ? m.n_tiles : 1);
            if (n_chunks * m.n_kpass > s.partial_cap) n_chunks = s.partial_cap / m.n_kpass;
            if (n_chunks < 1) {
                o.refused = DEMC_EINVAL; o.why = "data dimension too large for the partial-sum workspace";
                return o;
            }
            o.n_chunks = n_chunks; o.n_kpass = m.n_kpass;
            o.grid_x = (unsigned)(int)(n_ptiles * n_chunks);
            o.k0_stride = 4 * m.ks_t; o.part0_stride = n_chunks;
            o.n_partials = n_chunks * m.n_kpass;
        } break;
        case K2_OBS: {
            long long cap = m.N / 32;
            if (cap > s.partial_cap) cap = s.partial_cap;
            if (cap < 1 || s.family == FAM_RASTRIGIN) cap = 1;
            o.n_chunks = chunks_filling_rounds((n_prop + 255) / 256, cap, (double)occ.obs * s.n_cus);
            o.grid_x = (unsigned)((n_prop + 255) / 256); o.grid_y = (unsigned)o.n_chunks;
            o.n_partials = o.n_chunks;
        } break;
        case K2_LBA_WAVE: {
            // a wave per proposal, lanes across the (sorted) trials: k_lba_wave.  Chunks of whole batches (512 trials), at least two a chunk.
            // (the occupancy that sizes the chunks is the three-accumulator instance's, whichever runs)
            o.key[0] = m.n_acc == 3 ? 3 : m.n_acc == 2 ? 2 : 0;
            long long capw = m.N / 1024;
            if (capw > s.partial_cap) capw = s.partial_cap;
            if (capw < 1) capw = 1;
            o.n_chunks = chunks_filling_rounds((n_prop + 3) / 4, capw, (double)occ.lba_wave * s.n_cus);
            o.grid_x = (unsigned)((n_prop + 3) / 4); o.grid_y = (unsigned)o.n_chunks;
            o.n_partials = o.n_chunks;
        } break;
        case K2_USER:
        case K2_USER_ROW: {
            // thread per proposal x observation chunks, enough of them for 262144 threads; the whole-row plug-in: a workgroup per proposal
            long long want = (262144 + n_prop - 1) / n_prop;
            long long cap = m.N / 32;
            if (cap < 1) cap = 1;
            if (want > cap) want = cap;
            if (want > s.partial_cap) want = s.partial_cap;
            if (s.user_row) want = 1;
            o.n_chunks = (int)want;
            o.grid_x = s.user_row ? (unsigned)n_prop : (unsigned)((n_prop + 255) / 256);
            o.grid_y = (unsigned)want;
            o.n_partials = (int)want;
        } break;
        case K2_HIER: o.grid_x = (unsigned)n_prop; break;
        default:
            if (!is_mvn(s.family)) { o.refused = DEMC_EUNSUPPORTED; o.why = "model family not set or not registered"; }
            break;
    }
    return o;
}

// ---- the whole-update forms -------------------------------------------------------------------------------------------------------

// The kernel forms that can carry an update.  FORM_PHASE -- a K1 [-> K2 -> K3] chain per sweep and colour phase, k_longrow and
// k_frozen_sweep beneath it -- serves every configuration and is planned per launch (plan_phase).  The others run whole updates
// in one launch: planned once per model (plan_resident, plan_stream, plan_lean), chosen per step (choose_form).
enum Form {
    FORM_PHASE,
    FORM_RESIDENT,        // k_propose<..., RES>: the group in LDS, both colour phases of several iterations
    FORM_STREAM,          // k_propose<..., RES, LEAN, STREAM>: ... with the MvNormal observation stream inside
    FORM_LEAN_SUFFSTAT,   // k_res_mvn<WG, false, DT>: the default sampler on MvNormal-full (demc_resmvn.hpp)
    FORM_LEAN_STREAMING,  // k_res_mvn<WG, true, DT>
    FORM_LEAN_DIRECT,     // k_res_mvn<WG, true, DT, direct>
    FORM_LEAN_OBS,        // k_res_obs: the default sampler on the per-observation families (demc_resobs.hpp)
    FORM_LEAN_Z,          // k_res_mvn<WG, false, DT, HIST>: DE-MC_Z, one iteration per launch
    N_FORMS
};
// a group's observations in chunks, a workgroup each, which spin on each other's progress: the whole grid must be resident at once
constexpr bool spin_waiting(Form f) { return f == FORM_STREAM || f == FORM_LEAN_STREAMING || f == FORM_LEAN_DIRECT; }

struct FormGeo {
    bool ok = false;               // the form serves this model and configuration
    int wg = 0;                    // workgroup size
    size_t lds = 0;                // dynamic LDS bytes
    int lpp = 0, scr_doubles = 0;  // k_propose forms: lanes per particle, doubles of the theta' scratch
    int tail = TAIL_NONE;          // ... and the tail of their instances
};

// Geometry of the observation stream inside a resident kernel (plan_stream), shared by the spin-waiting forms: a handle runs in one
// likelihood mode, so at most one of FORM_STREAM / FORM_LEAN_STREAMING (STREAMING) and FORM_LEAN_DIRECT (DIRECT) reads it.
struct StreamDims {
    bool ok = false;
    int C = 0, nact_max = 0, rows = 0, x_lds = 0, chunk_tiles = 0;  // chunks per group, moving particles, scratch rows, X chunk in LDS, tiles per chunk
};

// lanes per particle of a resident k_propose: as many as let the moving half fill one pass of `budget` threads -- from 4 up to one
// lane per pair of scalars (fewer than 4 only where the row has fewer pairs)
inline int resident_lpp(int n_act, int lpp_max, int budget) {
    int lpp = 4;
    while (lpp * 2 <= lpp_max && n_act * lpp * 2 <= budget) lpp *= 2;
    return lpp > lpp_max ? lpp_max : lpp;
}

// k_res_mvn's DT: the row length where an instance has it compiled in, else 0.  MvNormal-full: 32 and 8 (cfg3, cfg2) when the prior
// table is one segment; MvNormal-iso: the row of the reference's own test -- 30 means and sigma -- whose instance reads the table
// as [one entry for the 30 means | one for sigma]: any other table takes the general row length
inline int compiled_row_length(int family, int D, int n_seg, const int* seg_start) {
    if (family == FAM_MVN_ISO) return (D == 31 && n_seg == 2 && seg_start[1] == 30) ? 31 : 0;
    return (n_seg == 1 && (D == 32 || D == 8)) ? D : 0;
}

// FORM_RESIDENT: one workgroup per group, both colour phases of several iterations in one launch.  It needs the fused accept tail
// (the whole update inside K1), the two_colour schedule (a phase writes only rows nobody reads), partners from the current
// population, and the whole group + its scratch in LDS.
inline FormGeo plan_resident(const Setup& s) {
    const demc_config& c = *s.c;
    FormGeo f;
    if (c.fuse != 0 || c.schedule != DEMC_SCHED_TWO_COLOUR || c.partner_kind != DEMC_PARTNER_CURRENT || c.Np < 4) return f;
    const int lpp_max = pow2_ceil((c.D + 1) / 2);
    if (lpp_max > 64) return f;
    const int n_act = c.Np - c.Np / 2;
    const size_t D = (size_t)c.D, Np = (size_t)c.Np, d = (size_t)s.m->d;
    const bool mvn = is_mvn(s.family);
    // geometry for a thread budget: lanes per particle, workgroup size, LDS bytes; false when the update cannot be fused or the
    // group does not fit
    auto geometry = [&](int budget) -> bool {
        f.lpp = resident_lpp(n_act, lpp_max, budget);
        f.wg = (n_act * f.lpp > 256 && budget > 256) ? 512 : 256;
        const TailFlags t = tail_flags(s, f.lpp, MODE_STEP, 0);
        if (!t.fuse_accept) return false;
        f.tail = tail_of(t);
        const size_t scr_doubles = (t.fuse_prep || t.fuse_obs) ? (size_t)(f.wg / f.lpp) * (D + 2) : 0;
        f.scr_doubles = (int)scr_doubles;
        const size_t doubles =
            Np * D + Np + (Np + (Np + 15) / 16) + ((s.family == FAM_MVN_FULL && s.k1->ainv_lds) ? d * d : 0) + (mvn ? d : 0) + scr_doubles;
        f.lds = doubles * sizeof(double) + (size_t)n_act * (4 * sizeof(double) + 4 * sizeof(int));
        return f.lds <= kMaxDynLds;
    };
    // More groups than CUs: two 256-thread workgroups per CU keep twice as many groups in flight as one of 512 -- when
    // two of them fit in a CU's LDS (measured at 1024 groups x 64: 0.082 -> see DESIGN.md section 6).
    const bool two_per_cu = s.geo_groups > 256 && geometry(256) && f.lds <= 75 * 1024;
    f.ok = two_per_cu || geometry(512);
    return f;
}

// The observation stream inside a resident kernel: the geometry and FORM_STREAM, the general kernel around it.
// 256-thread form: one wave per SIMD, i.e. the whole register file (512 per lane, AGPRs included) behind each wave -- what does
// not fit the 256 architectural VGPRs spills to AGPRs instead of scratch memory; 512 threads when a colour needs the lanes.
// It is for populations too small to fill the device with one K1 -> K2 -> K3 chain per colour phase (launch- and latency-bound):
// MvNormal family, STREAMING likelihood, two_colour, current-population partners, at most one group per CU, the group and its
// per-particle scratch in LDS, and a colour phase whose matrix work is in the launch-overhead range.  Large populations keep the
// per-phase chain, whose k_cross_mfma runs at the matrix peak.
// (DIRECT: the same geometry -- chunks of the observations per workgroup, hand-over granules -- serves FORM_LEAN_DIRECT only,
// plan_lean; the general kernel has no such form.)  Nothing is allocated here: the runtime's buffers follow.
struct StreamPlan { StreamDims dims; FormGeo form; };
inline StreamPlan plan_stream(const Setup& s) {
    const demc_config& c = *s.c;
    const ModelShape& m = *s.m;
    StreamPlan o;
    const bool direct = c.loglike_mode == DEMC_LOGLIKE_DIRECT;
    if (!is_mvn(s.family) || (c.loglike_mode != DEMC_LOGLIKE_STREAMING && !direct) || c.fuse != 0 || c.schedule != DEMC_SCHED_TWO_COLOUR ||
        c.partner_kind != DEMC_PARTNER_CURRENT || c.Np < 4 || s.n_cus < 1 || s.geo_groups > s.n_cus || c.n_groups > s.n_cus ||
        m.dpad > 64 || m.n_kpass != 1)
        return o;
    // Whether the form applies and into how many chunks C a group's observation tiles are cut is decided from the groups of
    // the WHOLE population (geometry_groups), not from this shard's: C fixes the summation order of the cross terms, and a
    // shard must make the choices of the unsharded run to reproduce it bit for bit (demc_create_multi, demc.h).
    const int gg = s.geo_groups > c.n_groups ? s.geo_groups : c.n_groups;
    const int nact_max = c.Np - c.Np / 2;
    if (nact_max > 512) return o;
    const double phase_flop = 2.0 * (double)nact_max * gg * (double)m.N * m.dpad;
    if (phase_flop / 78.6e12 > 300e-6) return o;
    const int lpp_max = pow2_ceil((c.D + 1) / 2);
    if (lpp_max > 64) return o;
    const int lpp = resident_lpp(nact_max, lpp_max, 512);
    const int wg = nact_max * lpp <= 256 ? 256 : 512, ppp = wg / lpp;
    const int rows = ((nact_max + ppp - 1) / ppp) * ppp;
    int C = 1;
    while (2 * C * gg <= s.n_cus && m.n_tiles / (2 * C) >= 8 && 2 * C <= 32) C *= 2;
    const int chunk = (m.n_tiles + C - 1) / C;
    const size_t D = (size_t)c.D, Np = (size_t)c.Np, d = (size_t)m.d;
    const size_t scr_doubles = (size_t)rows * (D + 6);
    const size_t doubles = Np * D + Np + (Np + (Np + 15) / 16) + ((s.family == FAM_MVN_FULL && s.k1->ainv_lds) ? d * d : 0) + d + scr_doubles +
                           (size_t)rows * m.dpad + (size_t)(wg / 64) * nact_max;
    size_t bytes = doubles * sizeof(double) + (size_t)nact_max * (4 * sizeof(double) + 4 * sizeof(int)) +
                   2 * sizeof(unsigned) * (size_t)C * nact_max + 16;
    if (bytes > kMaxDynLds) return o;
    const size_t xbytes = (size_t)(chunk + 1) * (m.dpad / 4) * 64 * sizeof(double);  // + the all-zero tail tile
    const int x_lds = (bytes + xbytes <= kMaxDynLds) ? 1 : 0;
    if (x_lds) bytes += xbytes;
    if (!direct) {  // (k_propose's streaming form has the two tails an MvNormal model can take: PREP_MFMA, else PREP)
        FormGeo& f = o.form;
        f.tail = tail_of(tail_flags(s, lpp, MODE_STEP, 0)) == TAIL_PREP_MFMA ? TAIL_PREP_MFMA : TAIL_PREP;
        f.ok = true; f.wg = wg; f.lds = bytes; f.lpp = lpp; f.scr_doubles = (int)scr_doubles;
    }
    StreamDims& g = o.dims;
    g.ok = true; g.C = C; g.nact_max = nact_max; g.rows = rows; g.x_lds = x_lds; g.chunk_tiles = chunk;
    return o;
}

// The lean resident kernels of the default sampler -- whether the SAMPLER is the default one is asked per step (choose_form).  They
// read the prior table in its run-length form and know no Normal(a, theta[ref]) prior, so this plan follows the table; it reads
// plan_resident's and plan_stream's results (`resident_ok`, `g`: the stream geometry with its buffers in place).
// The instances: k_res_obs<256>; FORM_LEAN_Z k_res_mvn<wg, false, dt, HIST, 1, iso> for HIST = 1, 2, 3; FORM_LEAN_SUFFSTAT
// k_res_mvn<wg, false, dt, 0, 1>; the streaming pair k_res_mvn<wg, true, dt, 0, 1, false, direct>.
struct LeanPlan {
    FormGeo form[N_FORMS];  // the five FORM_LEAN_* entries
    int dt = 0;             // k_res_mvn's DT
    bool iso = false;
};
inline LeanPlan plan_lean(const Setup& s, bool resident_ok, const StreamDims& g, size_t lnr_table_doubles) {
    const demc_config& c = *s.c;
    const ModelShape& m = *s.m;
    LeanPlan o;
    if (s.n_seg < 1 || s.normal_ref) return o;  // (the table must fit its run-length form; hierarchical scale priors: the general kernel)
    const int dt = o.dt = compiled_row_length(s.family, c.D, s.n_seg, s.seg_start);
    const int nact_max = c.Np - c.Np / 2;
    // FORM_LEAN_OBS (demc_resobs.hpp): Gaussian, Binomial and the LNR with a handful of parameters (a lane per scalar of a
    // sixteen-lane particle) and few enough observations for sixteen lanes to walk them; the group, its scratch rows and -- LNR --
    // the log Phi(-z) table in LDS
    if ((s.family == FAM_GAUSSIAN || s.family == FAM_BINOMIAL || s.family == FAM_LNR) && c.D <= 16 && c.fuse == 0 &&
        c.schedule == DEMC_SCHED_TWO_COLOUR && c.partner_kind == DEMC_PARTNER_CURRENT && c.Np >= 4 && c.Np <= 512 && m.N / 16 <= 512) {
        const size_t doubles = (size_t)c.Np * c.D + (size_t)c.Np + (size_t)nact_max + (size_t)(256 / 16) * c.D +
                               (s.family == FAM_LNR ? lnr_table_doubles : 0);
        if (doubles * sizeof(double) <= kMaxDynLds) {
            FormGeo& f = o.form[FORM_LEAN_OBS];
            f.ok = true; f.wg = 256; f.lds = doubles * sizeof(double);
        }
    }
    // FORM_LEAN_Z: DE-MC_Z (history partners, the synchronous schedule) on MvNormal-full in SUFFSTAT mode: the lean body with
    // partner rows from the history, one launch per iteration -- all it needs in LDS are select_base's cumulative weights and the
    // centred rows (... and on MvNormal(mu, sigma^2 I) with sigma a parameter, D = d + 1: the ISO instances of the same body)
    const bool iso = o.iso = s.family == FAM_MVN_ISO;
    if (((s.family == FAM_MVN_FULL && c.D == m.d) || (iso && c.D == m.d + 1)) && c.D <= 32 && c.fuse == 0 &&
        c.schedule == DEMC_SCHED_SYNCHRONOUS && c.partner_kind == DEMC_PARTNER_HISTORY && c.loglike_mode == DEMC_LOGLIKE_SUFFSTAT &&
        c.Np >= 4 && nact_max * 4 <= 512 && s.has_hist) {
        FormGeo& f = o.form[FORM_LEAN_Z];
        f.wg = nact_max * 4 > 256 ? 512 : 256;
        // cdf | chunk offsets | centred rows | A^-1 fragments [2][8][64] | the first half's held-back rows [wg][8] (+ alignment slack;
        // the snooker instance parks them) | ISO: xbar and sum_i x~_i [2][32]: demc_resmvn.hpp, pend_l / iso_l
        f.lds = ((size_t)c.Np + 16 + (size_t)(f.wg / 4) * ((size_t)c.D + 2) + 16 * 64 + 2 + (size_t)f.wg * 8 + 64) * sizeof(double);
        // HIST: 1 past burn-in, 2 inside it (random_gamma reads a base particle, crossover.jl:164: the instance that loads its
        // row), 3 with snooker updates
        f.ok = true;
        return o;
    }
    // the two_colour forms (demc_resmvn.hpp): MvNormal full Sigma, D = d <= 32, one pass per phase
    if (s.family != FAM_MVN_FULL || c.D != m.d || m.d > 32 || c.fuse != 0 || c.schedule != DEMC_SCHED_TWO_COLOUR ||
        c.partner_kind != DEMC_PARTNER_CURRENT || c.Np < 4 || nact_max * 4 > 512)
        return o;
    // (DIRECT at D = 8: 512 threads whatever the group's size -- two waves per SIMD for the residual loop, which one wave per SIMD runs
    // at half the vector pipe's rate: nothing else hides its LDS reads and dependent FP64 pairs)
    const bool dir = c.loglike_mode == DEMC_LOGLIKE_DIRECT;
    const bool dir8 = dir && c.D == 8 && nact_max * 4 <= 256;
    const int wg = (nact_max * 4 > 256 || dir8) ? 512 : 256;
    const size_t D = (size_t)c.D, Np = (size_t)c.Np;
    const size_t base = (Np * D + Np + (size_t)nact_max + 16 + (size_t)(wg / 4) * (D + 2)) * sizeof(double);
    if (c.loglike_mode == DEMC_LOGLIKE_SUFFSTAT) {
        if (base > kMaxDynLds || !resident_ok) return o;
        FormGeo& f = o.form[FORM_LEAN_SUFFSTAT];
        f.ok = true; f.wg = wg; f.lds = base;
        return o;
    }
    // STREAMING / DIRECT: only where the observation stream applies (plan_stream: small populations), and only with one wave per
    // SIMD (256 threads: what the observation stage needs beyond 256 VGPRs then lives in AGPRs, not scratch)
    if (!g.ok || (wg != 256 && !dir8)) return o;
    // (DIRECT: the instances with the row length compiled in, the chunk of whitened rows in LDS)
    if (dir && !(dt != 0 && m.dp_direct == c.D && m.dpad == c.D && g.x_lds)) return o;
    size_t bytes = base + ((size_t)(wg / 4) * m.dpad + (size_t)(dir ? wg / 16 : wg / 64) * nact_max) * sizeof(double) + 16;  // (DIRECT: a partial sum per 16-lane row)
    if (bytes > kMaxDynLds) return o;
    // (the X chunk rides in LDS exactly when plan_stream found room for it; this kernel's other buffers are no larger)
    if (g.x_lds) bytes += (size_t)(g.chunk_tiles + 1) * (m.dpad / 4) * 64 * sizeof(double);
    if (bytes > kMaxDynLds) return o;
    FormGeo& f = o.form[dir ? FORM_LEAN_DIRECT : FORM_LEAN_STREAMING];  // (DIRECT: <512, 8> and <256, 32>, what the tests above leave)
    f.ok = true; f.wg = wg; f.lds = bytes;
    return o;
}

// ---- choosing a form ------------------------------------------------------------------------------------------------------------

// Which form carries the updates of a step call: the ONE place where the plans (`ok[form]`) meet what is known only when a step is
// asked for -- a replay, an update of a subset of the groups, and the sampler around the kernels (lean_level: a trace, snooker
// updates, blocks).  None of it changes inside a call, and no rule depends on the iteration: inside burn-in FORM_LEAN_Z takes
// another instance, not another form.  First match wins.
inline Form choose_form(const bool (&ok)[N_FORMS], const demc_config& c, bool replay, bool subset) {
    // a replay hands over the caller's draws, which only the per-phase kernels read: no multi-iteration form, no lean DE-MC_Z body
    if (replay) return FORM_PHASE;
    const bool whole = !subset;  // a subset of the groups never takes a spin_waiting form; it may take the others
    const bool plain = lean_level(c, replay, DEMC_PARTNER_CURRENT) == 1;  // the lean two_colour kernels: no trace, snooker updates or blocks
    if (ok[FORM_LEAN_DIRECT] && plain && whole) return FORM_LEAN_DIRECT;  // DIRECT: the one whole-update form it has
    // STREAMING: the observation stream inside the resident kernel, the lean one where it serves
    if (ok[FORM_STREAM] && whole) return (plain && ok[FORM_LEAN_STREAMING]) ? FORM_LEAN_STREAMING : FORM_STREAM;
    // SUFFSTAT on MvNormal-full, then the per-observation families: their lean kernel before the general resident one
    if (ok[FORM_LEAN_SUFFSTAT] && plain) return FORM_LEAN_SUFFSTAT;
    if (ok[FORM_LEAN_OBS] && plain) return FORM_LEAN_OBS;
    if (ok[FORM_RESIDENT]) return FORM_RESIDENT;
    // DE-MC_Z: the lean body has a snooker instance but no block sweeps -- snooker with blocks goes to the per-phase chain
    const int lean_z = ok[FORM_LEAN_Z] ? lean_level(c, replay, DEMC_PARTNER_HISTORY) : 0;
    if (lean_z == 1 || (lean_z == 2 && c.n_blocks == 0)) return FORM_LEAN_Z;
    return FORM_PHASE;
}

// Iterations one launch carries at most: it stays in the millisecond range whatever the caller asks for, shorter where the grid
// spins.  (FORM_LEAN_Z: cells of history row t - 1 come from every group, so a launch cannot span iterations.)
inline int iterations_per_launch(Form f) { return (f == FORM_PHASE || f == FORM_LEAN_Z) ? 1 : spin_waiting(f) ? 64 : 1024; }

}  // namespace demc
