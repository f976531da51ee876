// schedule_host.cpp -- csrc/demc_schedule.hpp (and under it csrc/demc_philox.hpp) on the CPU: the refusals of a step call with code
// and text held literally, the segments at their edges, the sweeps and colour phases, the overlapped exchange's partition, the
// frozen-order predicate input by input and the shape of its table, the by-product snapshot's predicate.  Built with the address
// and undefined-behaviour sanitizers by tests/test_schedule_host.py; no GPU, no HIP runtime, no ROCm header -- that this compiles
// is the proof that both headers are host-only.
//
// schedule_host --dump reads one request per line from stdin and prints what the header answers, for the references written by
// other means in tests/test_schedule_host.py (the oracle's coins, a numpy Philox, a brute-force loop over the rules):
//   coin seed alpha n_groups_total lo hi                       -> the alpha coin of iterations lo..hi-1
//   groups seed n_groups_total iter                            -> select_groups, in order
//   frozen seed beta n_groups group_offset n_blocks frozen_bits iter0 n_iters   -> the table (bit b of frozen_bits: block b is frozen)
//   seg seed alpha n_groups_total n_groups iter0 n_iters with_migration per_phase cap own_comm overlap replay replayed_step u_step
//       history set_size                                       -> run:migrate of every segment (set_size 0: a handle's own call)
#include "demc_schedule.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {
using namespace demc;

int failures = 0, checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

bool refused_with(const Refusal& r, const char* text) { return r.code == DEMC_EINVAL && r.message == text; }

demc_config config(int n_groups = 4, int Np = 8, int D = 6) {
    demc_config c;
    std::memset(&c, 0, sizeof c);
    c.n_groups = n_groups; c.n_groups_total = n_groups; c.Np = Np; c.D = D;
    c.alpha = 0.1; c.beta = 0.1; c.kappa = 1.0; c.seed = 7; c.n_rows = 100;
    return c;
}

std::vector<Segment> segments(const StepCall& s, int64_t iter0) {
    std::vector<Segment> out;
    for (int64_t it = iter0; it < s.end;) {
        out.push_back(next_segment(s, it));
        CHECK(out.back().run >= 1);
        it += out.back().run;
        CHECK(it <= s.end);
    }
    return out;
}

// ---- every refusal: the code and the exact text, each text once --------------------------------------------------------------------
void refusals() {
    demc_config c = config();
    CHECK(!refuse_step(c, true, 1, 0) && !refuse_step(c, true, 1, 5) && refuse_step(c, true, 3, 2).message.empty());
    CHECK(refused_with(refuse_step(c, false, 1, 1), "demc_set_model has not been called"));
    CHECK(refused_with(refuse_step(c, true, 0, 1), "iter0 is 1-based (de.iter, main.jl:34)"));
    CHECK(refuse_step(c, true, 1, -1).code == DEMC_EINVAL);
    c.partner_kind = DEMC_PARTNER_HISTORY;
    CHECK(refused_with(refuse_step(c, true, 1, 1), "history partners need at least one stored row (n_initial > 0)"));
    CHECK(!refuse_step(c, true, 2, 100) && !refuse_step(c, true, 2, 0) && !refuse_step(c, true, 500, 0));  // rows 1..100: the last iteration reads row 100
    CHECK(refused_with(refuse_step(c, true, 2, 101), "history partners: iteration t reads history rows 1:(t-1), the history holds n_rows rows "
                                                     "(the reference sizes it n_iter + n_initial, utilities.jl:34)"));
    // which one wins: the model, the iteration, the first row, the last row
    CHECK(refuse_step(c, false, 0, 1000).message == "demc_set_model has not been called");
    CHECK(refuse_step(c, true, 0, 1000).message == "iter0 is 1-based (de.iter, main.jl:34)");
    CHECK(refuse_step(c, true, 1, 1000).message == "history partners need at least one stored row (n_initial > 0)");

    CHECK(!refuse_subset_call(c, 1) && !refuse_subset_call(c, 0));
    CHECK(refused_with(refuse_subset_call(c, 2), "history partners: a subset of the groups advances one iteration at a time (the cells of a history "
                                                 "row come from every group: update the other groups before the next iteration)"));
    c.partner_kind = DEMC_PARTNER_CURRENT;
    CHECK(!refuse_subset_call(c, 1000));

    const int32_t in[3] = {0, 3, 1}, low[2] = {1, -1}, high[2] = {4, 0};
    CHECK(!refuse_subset(c, false, in, 3) && !refuse_subset(c, false, nullptr, 0));
    CHECK(refused_with(refuse_subset(c, false, low, 2), "group index outside this handle"));
    CHECK(refuse_subset(c, false, high, 2).message == "group index outside this handle" && !refuse_subset(c, false, high + 1, 1));
    CHECK(refused_with(refuse_subset(c, true, in, 3), "subset updates follow demc_migration_groups, which does not see a replayed migration sub-group"));
    CHECK(refuse_subset(c, true, low, 2).message[0] == 's');  // the replay is seen first

    CHECK(!refuse_exchange(false, true));
    CHECK(refused_with(refuse_exchange(true, true), "shard of a multi-GPU set: step the set with demc_multi_step"));
    CHECK(refuse_exchange(true, false).message[1] == 'h');  // the set is seen first
    CHECK(refused_with(refuse_exchange(false, false), "sharded handle without a communicator: demc_comm_init, or drive the exchange with "
                                                      "demc_migration_pack/apply + demc_update"));
}

// ---- the coins at their ends -----------------------------------------------------------------------------------------------------
void coins() {
    demc_config c = config(1);
    c.alpha = 1.0;
    int perm[64];
    int32_t sel[64];
    for (int64_t it = 1; it <= 200; ++it) {
        CHECK(!migration_due(c, it) && select_groups(c, it, perm, sel) == 0);  // one group: never, nobody
        CHECK(!migration_due(c, it, true, 1e-300));                          // ... nor under a replayed uniform above 0: alpha is 0
    }
    c = config(1);
    c.n_groups_total = 0;  // (not filled in: n_groups stands in)
    CHECK(groups_total(c) == 1 && alpha_of(c) == 0.0);
    c = config(2);
    c.alpha = 1.0;
    for (int64_t it = 1; it <= 200; ++it) {
        CHECK(migration_due(c, it));
        CHECK(select_groups(c, it, perm, sel) == 2 && sel[0] + sel[1] == 1);  // two groups: both, in either order
    }
    CHECK(migration_due(c, 5, true, 1.0) && migration_due(c, 5, false, 2.0) == migration_due(c, 5));  // (no replayed coin: u_step is not read)
    c.alpha = 0.25;
    CHECK(migration_due(c, 5, true, 0.25) && !migration_due(c, 5, true, 0.2500001));
    c = config(64);
    for (int64_t it = 1; it <= 50; ++it) {  // an ordered sample without replacement of 2..64 groups
        const int n = select_groups(c, it, perm, sel);
        CHECK(n >= 2 && n <= 64);
        bool seen[64] = {false};
        for (int i = 0; i < n; ++i) {
            CHECK(sel[i] >= 0 && sel[i] < 64 && !seen[sel[i]]);
            seen[sel[i]] = true;
        }
    }
}
// (a replayed 0.0 with one group fires: the rule is `<=`, as the oracle's)
void one_group_replay() {
    const demc_config c = config(1);
    CHECK(alpha_of(c) == 0.0 && migration_due(c, 1, true, 0.0));
}

// ---- the segments at their edges ---------------------------------------------------------------------------------------------------
void segment_edges() {
    demc_config c = config();
    StepCall s;
    s.c = &c; s.with_migration = true; s.cap = 64;
    // no iteration: no segment
    s.end = 5;
    CHECK(segments(s, 5).empty());
    // no coin at all: a run exactly as long as the cap is one segment, one iteration more is a second, which migrates nothing
    c.alpha = 0.0;
    for (int cap : {1, 64, 1024}) {
        s.cap = cap; s.end = 1 + cap;
        std::vector<Segment> g = segments(s, 1);
        CHECK(g.size() == 1 && g[0].run == cap && g[0].migrate == MIG_NONE);
        s.end = 2 + cap;
        g = segments(s, 1);
        CHECK(g.size() == 2 && g[0].run == cap && g[1].run == 1 && g[1].migrate == MIG_NONE);
        s.per_phase = true;  // one iteration at a time, whatever the cap says
        g = segments(s, 1);
        CHECK((int)g.size() == cap + 1 && g[0].run == 1);
        s.per_phase = false;
    }
    // a coin at the first iteration of the call and at the last: [d1, d2] between two consecutive due iterations
    c.alpha = 0.1; s.cap = 1024;
    int64_t d1 = 1;
    while (!migration_due(c, d1)) ++d1;
    int64_t d2 = d1 + 1;
    while (!migration_due(c, d2)) ++d2;
    s.end = d2 + 1;
    std::vector<Segment> g = segments(s, d1);
    CHECK(g.size() == 2 && g[0].run == d2 - d1 && g[0].migrate == MIG_LOCAL && g[1].run == 1 && g[1].migrate == MIG_LOCAL);
    s.with_migration = false;  // demc_update: the same iterations, no coin
    g = segments(s, d1);
    CHECK(g.size() == 1 && g[0].run == d2 - d1 + 1 && g[0].migrate == MIG_NONE);
    s.with_migration = true;
    // the kinds: sharded, overlapped, and what turns the overlap off
    s.sharded = true;
    CHECK(next_segment(s, d1).migrate == MIG_EXCHANGE);
    s.overlap = true; s.cap = 1;
    g = segments(s, d1);
    CHECK(g.size() == 2 && g[0].migrate == MIG_OVERLAPPED && g[0].run == d2 - d1);  // not capped by the form
    s.replay = true;
    CHECK(next_segment(s, d1).migrate == MIG_EXCHANGE && next_segment(s, d1).run == 1);
    s.replay = false; c.partner_kind = DEMC_PARTNER_HISTORY;
    CHECK(next_segment(s, d1).migrate == MIG_EXCHANGE);
    c.partner_kind = DEMC_PARTNER_CURRENT; s.sharded = false;  // (the switch alone does not make a handle sharded)
    CHECK(next_segment(s, d1).migrate == MIG_LOCAL);
    // a replayed coin: every iteration or none
    s = StepCall();
    s.c = &c; s.with_migration = true; s.cap = 64; s.end = 11; s.replay = true; s.replayed_step = true; s.u_step = 0.05;
    g = segments(s, 1);
    CHECK(g.size() == 10 && g[9].migrate == MIG_LOCAL);
    s.u_step = 0.5;
    g = segments(s, 1);
    CHECK(g.size() == 1 && g[0].run == 10 && g[0].migrate == MIG_NONE);
    // the multi-GPU set: one shard sees no coin and no cap, two see every coin and no cap
    s = StepCall();
    s.c = &c; s.with_migration = true; s.cap = 1; s.per_phase = true; s.overlap = true; s.end = d2 + 1;
    g = segments(set_call(s, 1), 1);
    CHECK(g.size() == 1 && g[0].run == d2 && g[0].migrate == MIG_NONE);
    g = segments(set_call(s, 2), d1);
    CHECK(g.size() == 2 && g[0].run == d2 - d1 && g[0].migrate == MIG_EXCHANGE && g[1].migrate == MIG_EXCHANGE);
}

// ---- sweeps and colour phases ----------------------------------------------------------------------------------------------------
void sweeps_and_phases() {
    demc_config c = config();
    c.n_rows = 10;
    c.n_blocks = 0;
    CHECK(n_sweeps(c) == 1 && stored_row(c, true, 1, 0) == 0 && stored_row(c, true, 10, 0) == 9 && stored_row(c, true, 11, 0) == -1);
    CHECK(stored_row(c, false, 1, 0) == -1);
    c.n_blocks = 3;
    CHECK(n_sweeps(c) == 3);
    for (int64_t it = 1; it <= 12; ++it)
        for (int b = 0; b < 3; ++b) {
            CHECK(stored_row(c, true, it, b) == (b == 2 && it <= 10 ? it - 1 : -1));  // the last sweep only, inside n_rows only
            CHECK(stored_row(c, false, it, b) == -1);
        }
    for (int Np : {2, 3, 8, 9})
        for (int sched : {DEMC_SCHED_SEQUENTIAL, DEMC_SCHED_SYNCHRONOUS, DEMC_SCHED_TWO_COLOUR}) {
            c.Np = Np; c.schedule = sched;
            const int n = n_colour_phases(c);
            CHECK(n == (sched == DEMC_SCHED_TWO_COLOUR ? 2 : sched == DEMC_SCHED_SEQUENTIAL ? Np : 1));
            int next = 0;  // the active ranges partition 0..Np-1, in order
            for (int i = 0; i < n; ++i) {
                const ColourPhase p = colour_phase(c, i);
                CHECK(p.a_lo == next && p.n_act >= 1);
                next = p.a_lo + p.n_act;
                CHECK(p.pool_lo >= 0 && p.pool_n >= 1 && p.pool_lo + p.pool_n <= Np);
                // no pool holds a particle that moves: the pool lies beside the movers, or the mover itself is excluded
                const bool beside = p.pool_lo + p.pool_n <= p.a_lo || p.a_lo + p.n_act <= p.pool_lo;
                CHECK(beside || p.exclude_self == 1);
                if (sched == DEMC_SCHED_TWO_COLOUR) CHECK(beside && p.exclude_self == 0 && p.pool_n == Np - p.n_act);
                else CHECK(p.pool_lo == 0 && p.pool_n == Np && p.exclude_self == 1);
            }
            CHECK(next == Np);
        }
    c.Np = 9; c.schedule = DEMC_SCHED_TWO_COLOUR;  // half = Np / 2
    CHECK(colour_phase(c, 0).n_act == 4 && colour_phase(c, 1).a_lo == 4 && colour_phase(c, 1).n_act == 5);
}

// ---- the partition -------------------------------------------------------------------------------------------------------------
void partitions() {
    for (int world : {1, 2, 4})
        for (int rank = 0; rank < world; ++rank) {  // (world 4, rank 1 and 2: a shard in the middle, group_offset > 0)
            demc_config c = config(5);
            c.n_groups_total = 5 * world; c.group_offset = 5 * rank;
            std::vector<int> perm((size_t)c.n_groups_total);
            std::vector<int32_t> sel((size_t)c.n_groups_total);
            int32_t mine[5], rest[5];
            for (int64_t it = 1; it <= 100; ++it) {
                const Partition p = exchange_partition(c, it, perm.data(), sel.data(), mine, rest);
                CHECK(p.n_mine + p.n_rest == 5);
                bool in_mine[5] = {false}, in_rest[5] = {false};
                for (int i = 0; i < p.n_mine; ++i) { CHECK(mine[i] >= 0 && mine[i] < 5 && (i == 0 || mine[i] > mine[i - 1])); in_mine[mine[i]] = true; }
                for (int i = 0; i < p.n_rest; ++i) { CHECK(rest[i] >= 0 && rest[i] < 5 && (i == 0 || rest[i] > rest[i - 1])); in_rest[rest[i]] = true; }
                const int n = select_groups(c, it, perm.data(), sel.data());
                for (int g = 0; g < 5; ++g) {
                    bool selected = false;
                    for (int i = 0; i < n; ++i) selected = selected || sel[(size_t)i] == c.group_offset + g;
                    CHECK(in_mine[g] == selected && in_rest[g] == !selected);
                }
            }
        }
}

// ---- the frozen order and the by-product snapshot: every input of the predicates flips them on its own ------------------------------
struct FrozenCase {
    demc_config c = config(7, 300, 4200);
    ModelShape m;
    K1Lds k1;
    Setup s;
    MaskRuns runs[3];
    FrozenCase() {
        c.n_blocks = 3; c.beta = 0.1; c.schedule = DEMC_SCHED_SYNCHRONOUS;
        c.partner_kind = DEMC_PARTNER_HISTORY; c.burnin = 10;
        k1.hier_scr = true;
        s.c = &c; s.m = &m; s.k1 = &k1; s.family = FAM_HIER_BINOMIAL; s.lpp = 512; s.geo_groups = 7; s.n_cus = 256;
        for (int b : {0, 2}) { runs[b].n = 2; runs[b].in = 2u; runs[b].start[0] = 0; runs[b].start[1] = 4000; }  // block 1: no run-length form
    }
    size_t entries(int n_iters = 3, size_t n_runs = 3) const { return frozen_order_entries(s, runs, n_runs, n_iters); }
};

void frozen_predicate() {
    {
        FrozenCase f;
        CHECK(frozen_possible(f.s) && f.entries() == 3u * 3u * 7u && snap2_wanted(f.s));
        CHECK(frozen_block(f.runs, 3, 0, f.c.D) && !frozen_block(f.runs, 3, 1, f.c.D) && frozen_block(f.runs, 3, 2, f.c.D) && !frozen_block(f.runs, 2, 2, f.c.D));
        CHECK(f.entries(0) == 0 && f.entries(-1) == 0 && f.entries(1) == 21);
        CHECK(f.entries(3, 0) == 0);  // no mask in run-length form: no frozen block
        CHECK(f.entries(3, 1) == 63);
    }
    { FrozenCase f; f.s.family = FAM_GAUSSIAN; CHECK(!frozen_possible(f.s) && f.entries() == 0 && !snap2_wanted(f.s)); }
    { FrozenCase f; f.c.Np = 513; CHECK(frozen_possible(f.s) && f.entries() == 0); }
    { FrozenCase f; f.c.Np = 512; CHECK(f.entries() == 63); }
    { FrozenCase f; f.s.subset = true; CHECK(f.entries() == 0); }
    { FrozenCase f; f.c.beta = 0.0; CHECK(f.entries() == 0); }
    { FrozenCase f; f.s.replay = true; CHECK(f.entries() == 0); }
    { FrozenCase f; f.runs[0].in = 0u; f.runs[2].n = 0; CHECK(f.entries() == 0); }  // no block with a scalar inside
    {
        FrozenCase f;  // the table's limit: n_iters * n_blocks * n_groups <= kFrozenOrderMax
        static_assert(kFrozenOrderMax == (size_t)1 << 24, "the limit the project states");
        f.c.n_groups = 1 << 12; f.s.geo_groups = 1 << 12;
        CHECK(f.entries(1365) == (size_t)1365 * 3 * 4096 && f.entries(1366) == 0);  // 3 * 4096 * 1365 = 2^24 - 4096
        f.c.n_blocks = 4;
        MaskRuns four[4] = {f.runs[0], f.runs[0], f.runs[0], f.runs[0]};
        CHECK(frozen_order_entries(f.s, four, 4, 1024) == kFrozenOrderMax && frozen_order_entries(f.s, four, 4, 1025) == 0);
    }
    // the by-product snapshot
    { FrozenCase f; f.c.n_blocks = 1; CHECK(frozen_possible(f.s) && !snap2_wanted(f.s)); }
    { FrozenCase f; f.c.schedule = DEMC_SCHED_TWO_COLOUR; CHECK(frozen_possible(f.s) && !snap2_wanted(f.s)); }
    { FrozenCase f; f.c.partner_kind = DEMC_PARTNER_CURRENT; CHECK(!snap2_wanted(f.s)); }
    { FrozenCase f; f.c.proposal_kind = 1; CHECK(!snap2_wanted(f.s)); }
    { FrozenCase f; f.c.burnin = 0; CHECK(!snap2_wanted(f.s)); }
}

void frozen_table_shape() {
    FrozenCase f;
    f.c.beta = 0.5; f.c.group_offset = 5;
    std::vector<int> order(f.entries() + 1, -7);
    fill_frozen_order(f.c, f.runs, 3, 11, 3, order.data());
    CHECK(order.back() == -7);  // nothing past the table
    for (int t = 0; t < 3; ++t)
        for (int b = 0; b < 3; ++b) {
            const int* o = order.data() + (t * 3 + b) * 7;
            std::vector<int> want, others;  // the groups whose coin fires, then the others: each in ascending order
            for (int g = 0; g < 7; ++g) {
                const U4 r = draw_block(f.c.seed, S_GROUP, (uint32_t)b, (uint64_t)(11 + t), (uint32_t)(5 + g), 0u);
                (b != 1 && u53(r.x, r.y) <= 0.5 ? want : others).push_back(g);
            }
            want.insert(want.end(), others.begin(), others.end());
            for (int i = 0; i < 7; ++i) CHECK(o[i] == want[(size_t)i]);
            if (b == 1) for (int i = 0; i < 7; ++i) CHECK(o[i] == i);
        }
}

// ---- --dump ------------------------------------------------------------------------------------------------------------------------
int dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        std::string out = what + " ";
        auto put = [&](long long v, bool first) { out += (first ? "" : ",") + std::to_string(v); };
        demc_config c = config();
        unsigned long long seed = 0;
        if (what == "coin") {
            long long lo, hi;
            in >> seed >> c.alpha >> c.n_groups_total >> lo >> hi;
            c.seed = seed; c.n_groups = c.n_groups_total;
            for (long long it = lo; it < hi; ++it) put(migration_due(c, it), it == lo);
        } else if (what == "groups") {
            long long it;
            in >> seed >> c.n_groups_total >> it;
            c.seed = seed; c.n_groups = c.n_groups_total;
            std::vector<int> perm((size_t)c.n_groups_total);
            std::vector<int32_t> sel((size_t)c.n_groups_total);
            const int n = select_groups(c, it, perm.data(), sel.data());
            for (int i = 0; i < n; ++i) put(sel[(size_t)i], i == 0);
        } else if (what == "frozen") {
            unsigned bits;
            long long iter0;
            int n_iters;
            in >> seed >> c.beta >> c.n_groups >> c.group_offset >> c.n_blocks >> bits >> iter0 >> n_iters;
            c.seed = seed;
            std::vector<MaskRuns> runs((size_t)c.n_blocks);
            for (int b = 0; b < c.n_blocks; ++b)
                if ((bits >> b) & 1u) { runs[(size_t)b].n = 1; runs[(size_t)b].in = 1u; }
            std::vector<int> order((size_t)n_iters * c.n_blocks * c.n_groups);
            fill_frozen_order(c, runs.data(), runs.size(), iter0, n_iters, order.data());
            for (size_t i = 0; i < order.size(); ++i) put(order[i], i == 0);
        } else if (what == "seg") {
            long long iter0;
            int n_iters, with_migration, per_phase, own_comm, overlap, replay, replayed_step, history, set_size;
            StepCall s;
            in >> seed >> c.alpha >> c.n_groups_total >> c.n_groups >> iter0 >> n_iters >> with_migration >> per_phase >> s.cap >> own_comm >> overlap >>
                replay >> replayed_step >> s.u_step >> history >> set_size;
            c.seed = seed; c.partner_kind = history ? DEMC_PARTNER_HISTORY : DEMC_PARTNER_CURRENT;
            s.c = &c; s.end = iter0 + n_iters; s.with_migration = with_migration != 0; s.per_phase = per_phase != 0;
            s.sharded = c.n_groups_total != c.n_groups || own_comm != 0;
            s.overlap = overlap != 0; s.replay = replay != 0; s.replayed_step = replayed_step != 0;
            if (set_size > 0) s = set_call(s, set_size);
            bool first = true;
            for (long long it = iter0; it < s.end;) {
                const Segment g = next_segment(s, it);
                out += (first ? "" : ",") + std::to_string(g.run) + ":" + std::to_string((int)g.migrate);
                first = false;
                it += g.run;
            }
        } else
            return 2;
        if (!in) return 3;
        std::printf("%s\n", out.c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) return dump();
    refusals();
    coins();
    one_group_replay();
    segment_edges();
    sweeps_and_phases();
    partitions();
    frozen_predicate();
    frozen_table_shape();
    if (failures) std::fprintf(stderr, "%d of %d check(s) failed\n", failures, checks);
    else std::printf("schedule ok: %d checks\n", checks);
    return failures ? 1 : 0;
}
