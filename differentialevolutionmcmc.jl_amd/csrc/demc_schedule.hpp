// demc_schedule.hpp -- what a demc_step call does, iteration by iteration: the alpha coin and select_groups as the host re-draws
// them, every refusal of a step call, the segments a call falls into (how many iterations go into one launch, and which kind of
// migration opens it), the sweeps and colour phases of one per-phase iteration, the overlapped exchange's partition of the groups,
// the launch order of the frozen sweeps, and when the by-product snapshot exists.  Pure functions of plain values, host only:
// plain C++17, no device header, no handle, nothing allocated -- lists go into memory the caller provides.  The runtime gathers
// the inputs and carries the answers out; tests/schedule_host.cpp runs these on the CPU under the sanitizers.
// (DESIGN.md "The schedule of a step call" states the segment rules.)
#pragma once
#include "../../include/demc.h"

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#include "demc_geometry.hpp"  // Setup, Form, frozen_possible, block_span, MaskRuns
#include "demc_hostbase.hpp"  // Refusal
#include "demc_philox.hpp"    // draw_block, u53, mulhi32: the text the kernels draw with

namespace demc {

// ---- the two public coins -------------------------------------------------------------------------------------------------------

inline int groups_total(const demc_config& c) { return c.n_groups_total > 0 ? c.n_groups_total : c.n_groups; }
// one group in total never migrates (structs.jl:102-105)
inline double alpha_of(const demc_config& c) { return groups_total(c) == 1 ? 0.0 : c.alpha; }

// the alpha coin of iteration `iter` (main.jl:85): a pure function of (seed, iter)
inline bool migration_due(const demc_config& c, int64_t iter) {
    const U4 r = draw_block(c.seed, S_STEP, 0, (uint64_t)iter, 0, 0);
    return u53(r.x, r.y) <= alpha_of(c);
}
// ... as a handle sees it: the replayed uniform while one is set
inline bool migration_due(const demc_config& c, int64_t iter, bool replayed, double u_step) {
    return replayed ? u_step <= alpha_of(c) : migration_due(c, iter);
}

// select_groups (migration.jl:31-35) exactly as k_mig_apply draws it: N = rand(2:n_groups), ordered sample without replacement by
// a partial Fisher-Yates shuffle, words from the STEP stream.  `perm`: scratch of groups_total ints; the count is returned, the
// GLOBAL group indices go to sel (none with fewer than two groups).
inline int select_groups(const demc_config& c, int64_t iter, int* perm, int32_t* sel) {
    const int ng = groups_total(c);
    if (ng < 2) return 0;
    for (int i = 0; i < ng; ++i) perm[i] = i;
    const U4 r0 = draw_block(c.seed, S_STEP, 0, (uint64_t)iter, 0, 0);
    const int ns = 2 + (int)mulhi32(r0.z, (uint32_t)(ng - 1));
    U4 r = r0;
    for (int i = 0; i < ns; ++i) {
        if ((i & 3) == 0) r = draw_block(c.seed, S_STEP, 0, (uint64_t)iter, 0, 1 + (uint32_t)(i >> 2));
        const uint32_t w = (i & 3) == 0 ? r.x : (i & 3) == 1 ? r.y : (i & 3) == 2 ? r.z : r.w;
        const int j = i + (int)mulhi32(w, (uint32_t)(ng - i));
        const int t = perm[i];
        perm[i] = perm[j];
        perm[j] = t;
    }
    for (int i = 0; i < ns; ++i) sel[i] = perm[i];
    return ns;
}

// ---- the refusals of a step call ------------------------------------------------------------------------------------------------

// whatever evaluates the model (a step, demc_logpost); `model_set`: demc_set_model (or one of its kin) has succeeded
inline Refusal refuse_without_model(bool model_set) {
    if (!model_set) return Refusal{DEMC_EINVAL, "demc_set_model has not been called"};
    return {};
}
// every step, update and subset-update call
inline Refusal refuse_step(const demc_config& c, bool model_set, int64_t iter0, int32_t n_iters) {
    if (Refusal r = refuse_without_model(model_set)) return r;
    if (iter0 < 1 || n_iters < 0) return Refusal{DEMC_EINVAL, "iter0 is 1-based (de.iter, main.jl:34)"};
    if (c.partner_kind == DEMC_PARTNER_HISTORY && iter0 < 2)
        return Refusal{DEMC_EINVAL, "history partners need at least one stored row (n_initial > 0)"};
    // resample draws cells of rows 1:(iter-1) (crossover.jl:116-118): every one of them must lie inside the history buffer
    if (c.partner_kind == DEMC_PARTNER_HISTORY && n_iters > 0 && iter0 + (int64_t)n_iters - 2 > c.n_rows)
        return Refusal{DEMC_EINVAL, "history partners: iteration t reads history rows 1:(t-1), the history holds n_rows rows "
                                    "(the reference sizes it n_iter + n_initial, utilities.jl:34)"};
    return {};
}
// what a caller's subset update adds
inline Refusal refuse_subset_call(const demc_config& c, int32_t n_iters) {
    if (c.partner_kind == DEMC_PARTNER_HISTORY && n_iters > 1)
        return Refusal{DEMC_EINVAL, "history partners: a subset of the groups advances one iteration at a time (the cells of a history "
                                    "row come from every group: update the other groups before the next iteration)"};
    return {};
}
// ... and every subset update, the overlapped exchange's own among them; `replayed_subgroup`: a replay with a migration sub-group
inline Refusal refuse_subset(const demc_config& c, bool replayed_subgroup, const int32_t* groups, int32_t n) {
    if (replayed_subgroup)
        return Refusal{DEMC_EINVAL, "subset updates follow demc_migration_groups, which does not see a replayed migration sub-group"};
    for (int i = 0; i < n; ++i)
        if (groups[i] < 0 || groups[i] >= c.n_groups) return Refusal{DEMC_EINVAL, "group index outside this handle"};
    return {};
}
// a due migration of a sharded handle; `in_set`: it is a shard of a multi-GPU set, `has_comm`: it has a communicator
inline Refusal refuse_exchange(bool in_set, bool has_comm) {
    if (in_set) return Refusal{DEMC_EINVAL, "shard of a multi-GPU set: step the set with demc_multi_step"};
    if (!has_comm)
        return Refusal{DEMC_EINVAL, "sharded handle without a communicator: demc_comm_init, or drive the exchange with "
                                    "demc_migration_pack/apply + demc_update"};
    return {};
}

// ---- the segments of a call -----------------------------------------------------------------------------------------------------

// A call [iter0, end) falls into segments: `run` iterations that go out together, opened by one migration or by none.
enum Migrate { MIG_NONE, MIG_LOCAL, MIG_EXCHANGE, MIG_OVERLAPPED };
struct Segment {
    int run = 0;
    Migrate migrate = MIG_NONE;
};

constexpr int kUncapped = INT_MAX;  // StepCall::cap of a segment no form limits

struct StepCall {
    const demc_config* c = nullptr;
    int64_t end = 0;             // one past the call's last iteration
    bool with_migration = false; // demc_step (demc_update and the subset updates migrate nothing; the multi-GPU set: more than one shard)
    bool per_phase = false;      // FORM_PHASE: one iteration at a time
    int cap = 1;                 // iterations_per_launch(form); kUncapped in the multi-GPU set, whose shards cap their own launches
    bool sharded = false;        // n_groups_total != n_groups, or the handle owns a communicator (one of a single rank takes the same path)
    bool overlap = false;        // demc_comm_set_overlap
    bool replay = false;         // a replay is active ...
    bool replayed_step = false;  // ... and it carries the alpha coin's uniform,
    double u_step = 0.0;         //     this one
    bool due(int64_t iter) const { return with_migration && migration_due(*c, iter, replay && replayed_step, u_step); }
};

// The call of a multi-GPU set of n_shards, from a shard's: the coins count only between shards (a single shard keeps its on-device
// migration inside its own call), the rows change hands by the set's exchange, and the segments are uncapped.
inline StepCall set_call(StepCall s, int n_shards) {
    s.with_migration = n_shards > 1;
    s.per_phase = false; s.cap = kUncapped;
    s.sharded = true; s.overlap = false;
    return s;
}

// iterations from `iter` on up to `limit`, the next due coin or the end, whichever comes first (`iter` itself is not asked)
inline int run_length(const StepCall& s, int64_t iter, int limit) {
    int run = 1;
    while (run < limit && iter + run < s.end && !s.due(iter + run)) ++run;
    return run;
}

// What comes next at iteration `iter` of the call (iter < end).  The ONE statement of the run rule.
inline Segment next_segment(const StepCall& s, int64_t iter) {
    Segment g;
    if (s.due(iter)) {
        // (history partners: the cells of row t - 1 come from EVERY group, so no subset of the groups may run ahead of the others by
        // an iteration -- the overlapped form, which lets the unselected groups do exactly that, is not taken)
        const bool overlapped = s.sharded && s.overlap && !s.replay && s.c->partner_kind != DEMC_PARTNER_HISTORY;
        g.migrate = !s.sharded ? MIG_LOCAL : overlapped ? MIG_OVERLAPPED : MIG_EXCHANGE;
    }
    // an overlapped segment is not capped by the form: the subset updates inside it are calls of their own and cap themselves
    g.run = g.migrate == MIG_OVERLAPPED ? run_length(s, iter, kUncapped) : s.per_phase ? 1 : run_length(s, iter, s.cap);
    return g;
}

// ---- the sweeps and colour phases of one per-phase iteration ----------------------------------------------------------------------

inline int n_sweeps(const demc_config& c) { return c.n_blocks > 0 ? c.n_blocks : 1; }  // block_update! main.jl:174-179

// the history row sweep `b` of iteration `iter` stores (store_samples!): row iter - 1, in the last sweep, while the history holds it
inline long long stored_row(const demc_config& c, bool has_hist, int64_t iter, int b) {
    const long long row = iter - 1;
    return (b == n_sweeps(c) - 1 && has_hist && row < c.n_rows) ? row : -1;
}

// Which particles of every group move in a launch, and which are their partners.
struct ColourPhase {
    int a_lo, n_act, pool_lo, pool_n, exclude_self;
};
inline int n_colour_phases(const demc_config& c) {
    return c.schedule == DEMC_SCHED_TWO_COLOUR ? 2 : c.schedule == DEMC_SCHED_SEQUENTIAL ? c.Np : 1;
}
inline ColourPhase colour_phase(const demc_config& c, int i) {
    const int Np = c.Np, half = Np / 2;
    if (c.schedule == DEMC_SCHED_TWO_COLOUR)  // each half moves against the other, which rests
        return i == 0 ? ColourPhase{0, half, half, Np - half, 0} : ColourPhase{half, Np - half, 0, half, 0};
    // crossover.jl:13-15 / mutation.jl:16: particle i of every group moves after 0..i-1 were updated in place; the groups advance
    // side by side (one task per group in p_update!, main.jl:135-148).  Partners come from the whole group minus self (setdiff,
    // crossover.jl:158), snooker's three from the whole group (crossover.jl:241).
    if (c.schedule == DEMC_SCHED_SEQUENTIAL) return ColourPhase{i, 1, 0, Np, 1};
    return ColourPhase{0, Np, 0, Np, 1};  // synchronous: everybody at once, against the whole group minus self
}

// ---- the overlapped exchange's partition ------------------------------------------------------------------------------------------

// The sub-group of an exchange is a pure function of (seed, iter): the local groups it selected wait for the gather (`mine`), the
// others run ahead of it (`rest`), each list in ascending local index.  perm, sel: scratch of groups_total ints each (select_groups);
// mine, rest: room for n_groups entries each.
struct Partition {
    int n_mine = 0, n_rest = 0;
};
inline Partition exchange_partition(const demc_config& c, int64_t iter, int* perm, int32_t* sel, int32_t* mine, int32_t* rest) {
    const int n_sel = select_groups(c, iter, perm, sel);
    Partition p;
    for (int i = 0; i < n_sel; ++i) {
        const int gl = sel[i] - c.group_offset;
        if (gl >= 0 && gl < c.n_groups) mine[p.n_mine++] = gl;
    }
    std::sort(mine, mine + p.n_mine);
    for (int g = 0, m = 0; g < c.n_groups; ++g) {  // whoever is not in the sorted `mine`
        if (m < p.n_mine && mine[m] == g) ++m;
        else rest[p.n_rest++] = g;
    }
    return p;
}

// ---- the frozen-sweep launch order ------------------------------------------------------------------------------------------------

// k_frozen_sweep: launch order of the groups per (iteration, block sweep) of a demc_step call -- groups whose mutation coin fires
// (main.jl:199-207) first: their workgroups move the whole row and take twice as long, and a slow workgroup that starts last ends
// the launch.  A hint only: any order gives the same results.

constexpr size_t kFrozenOrderMax = (size_t)1 << 24;  // entries of the largest table built (64 MiB of pinned and of device memory)

// block sweep `b` can take the frozen form: its mask has a run-length form with a scalar inside
inline bool frozen_block(const MaskRuns* runs, size_t n_runs, int b, int D) {
    return (size_t)b < n_runs && block_span(runs[b].n, runs[b].in, runs[b].start, D).inside >= 1;
}

// Entries of the table of a call of n_iters iterations; 0: none is built -- where the phase plan cannot take the frozen form at
// all (frozen_possible; a pool beyond the kernel's), for a subset of the groups (its own list), without mutation, under a replay,
// where no block is frozen, or past kFrozenOrderMax.
inline size_t frozen_order_entries(const Setup& s, const MaskRuns* runs, size_t n_runs, int32_t n_iters) {
    const demc_config& c = *s.c;
    if (!frozen_possible(s) || c.Np > 512 || s.subset || c.beta <= 0.0 || s.replay || n_iters < 1) return 0;
    bool any = false;
    for (int b = 0; b < c.n_blocks; ++b) any = any || frozen_block(runs, n_runs, b, c.D);
    const size_t need = (size_t)n_iters * c.n_blocks * c.n_groups;
    return any && need <= kFrozenOrderMax ? need : 0;
}

// order[(t * n_blocks + b) * n_groups + .]: in a frozen block the groups whose coin fires, ascending, then the others, ascending;
// in any other block 0, 1, 2, ...  The group's coin is addressed Philox: the host draws what the kernel will draw.
inline void fill_frozen_order(const demc_config& c, const MaskRuns* runs, size_t n_runs, int64_t iter0, int32_t n_iters, int* order) {
    const int G = c.n_groups;
    for (int32_t t = 0; t < n_iters; ++t)
        for (int b = 0; b < c.n_blocks; ++b) {
            int* o = order + ((size_t)t * c.n_blocks + b) * G;
            const bool frozen = frozen_block(runs, n_runs, b, c.D);
            int front = 0, back = G;  // the others are collected from the end, descending, and turned round
            for (int g = 0; g < G; ++g) {
                bool mut = false;
                if (frozen) {
                    const U4 r = draw_block(c.seed, S_GROUP, (uint32_t)b, (uint64_t)(iter0 + t), (uint32_t)(c.group_offset + g), 0u);
                    mut = u53(r.x, r.y) <= c.beta;
                }
                if (mut) o[front++] = g;
                else o[--back] = g;
            }
            for (int i = back, j = G - 1; i < j; ++i, --j) {
                const int x = o[i];
                o[i] = o[j];
                o[j] = x;
            }
        }
}

// ---- the by-product snapshot ------------------------------------------------------------------------------------------------------

// The buffers exist exactly while the configuration can take that path: DE-MC_Z inside burn-in, long hierarchical rows, more than
// one block, enough particles for the row-streaming kernel.
inline bool snap2_wanted(const Setup& s) {
    const demc_config& c = *s.c;
    return frozen_possible(s) && c.n_blocks > 1 && c.schedule == DEMC_SCHED_SYNCHRONOUS && c.partner_kind == DEMC_PARTNER_HISTORY &&
           c.proposal_kind == 0 && c.burnin >= 1;
}

}  // namespace demc
