// geometry_host.cpp -- csrc/demc_geometry.hpp on the CPU: the launch-geometry rules of the runtime against the project's own
// statements (the comments of the rules, the docstring of tests/test_gpu_instance_selection.py) and against
// brute force written here by other means (exact integer arithmetic, restated definitions).  Built with the address and
// undefined-behaviour sanitizers by tests/test_geometry_host.py; no GPU, no HIP runtime, no ROCm header.
#include "demc_geometry.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

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

// A configuration, a model shape and the sizing that follows from them, with the Setup that points at them.
struct Case {
    demc_config c{};
    ModelShape m;
    K1Lds k1;
    int seg_start[kMaxDimSeg] = {0};
    Setup s;
    Refusal refused;
    Case(int family, int n_groups, int Np, int D, int schedule, int partner) {
        c.n_groups = n_groups; c.Np = Np; c.D = D; c.schedule = schedule; c.partner_kind = partner;
        c.kappa = 1.0; c.beta = 0.1; c.burnin = 3; c.n_groups_total = n_groups; c.store_history = 1; c.n_initial = 2; c.n_rows = 8;
        s.family = family;
        s.n_seg = 1; s.has_hist = true; s.partial_cap = 64; s.geo_groups = n_groups; s.n_cus = 256;
    }
    // (after the fields above are final)
    Setup& size() {
        s.c = &c; s.m = &m; s.seg_start = seg_start; s.k1 = &k1;
        s.lpp = lanes_per_particle(c.D, c.Np, c.schedule, s.geo_groups);
        refused = carve_k1_lds(s.family, m.d, c.Np, c.D, s.lpp, k1);
        return s;
    }
};

Case mvn_full(int d, int n_groups, int Np, int schedule, int partner, int mode, long long N = 64) {
    Case k(FAM_MVN_FULL, n_groups, Np, d, schedule, partner);
    k.c.loglike_mode = mode;
    k.m.N = N; k.m.d = d; k.m.dpad = d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : 32; k.m.n_tiles = (int)((N + 15) / 16);
    k.m.ks_t = k.m.dpad / 4; k.m.n_kpass = 1; k.m.dp_direct = k.m.dpad < 8 ? 8 : k.m.dpad;
    return k;
}
Case gaussian(int n_groups, int Np, int schedule, int partner, long long N = 64) {
    Case k(FAM_GAUSSIAN, n_groups, Np, 2, schedule, partner);
    k.m.N = N;
    return k;
}
// hierarchical Binomial: two hyper-parameters and S subject effects
Case hier_binomial(int S, int n_groups, int Np, int schedule, int partner) {
    Case k(FAM_HIER_BINOMIAL, n_groups, Np, S + 2, schedule, partner);
    k.m.N = S;
    return k;
}

// ---- chunks_filling_rounds ----------------------------------------------------------------------------------------------------

// fill of a launch of `wgs` workgroups on `res` resident ones, as the fraction wgs / (rounds * res)
struct Frac { long long num, den; };
Frac fill_of(long long wgs, long long res) { return {wgs, ((wgs + res - 1) / res) * res}; }
int cmp(Frac a, Frac b) {  // sign of a - b, exactly
    const long long l = a.num * b.den, r = b.num * a.den;
    return l < r ? -1 : l > r ? 1 : 0;
}

void check_chunks() {
    // cfg3: 128 blocks x 48 chunks = 4 full rounds of 1536 resident workgroups; 32 chunks are admissible and fill less
    CHECK(chunks_filling_rounds(128, 64, 1536.0) == 48);
    CHECK(32 <= 64 && cmp(fill_of(128 * 32, 1536), fill_of(128 * 48, 1536)) < 0);
    CHECK(fill_of(128 * 48, 1536).num == fill_of(128 * 48, 1536).den && 128 * 48 == 4 * 1536);
    const long long residents[] = {1, 7, 256, 1536};
    for (long long res : residents)
        for (long long blocks = 1; blocks <= 40; ++blocks)
            for (long long cap = 1; cap <= 20; ++cap) {
                const int got = chunks_filling_rounds(blocks, cap, (double)res);
                CHECK(got >= 1 && got <= cap);
                if (cap == 1) CHECK(got == 1);
                Frac best = fill_of(blocks, res);
                for (long long nc = 2; nc <= cap; ++nc)
                    if (cmp(fill_of(blocks * nc, res), best) > 0) best = fill_of(blocks * nc, res);
                // (two different fills of this grid are at least 1 / 1536^2 apart: "within 1e-9" is "equal")
                long long want = 0, smallest = 0;
                for (long long nc = 1; nc <= cap; ++nc)
                    if (cmp(fill_of(blocks * nc, res), best) == 0) {
                        if (!smallest) smallest = nc;
                        if ((blocks * nc + res - 1) / res <= 4) want = nc;  // the largest within four rounds
                    }
                if (!want) want = smallest;
                CHECK(cmp(fill_of(blocks * got, res), best) == 0);
                if (got != want) std::fprintf(stderr, "blocks %lld cap %lld resident %lld: %d, expected %lld\n", blocks, cap, res, got, want);
                CHECK(got == want);
            }
}

// ---- lanes per particle, workgroup sizes, compiled row lengths ----------------------------------------------------------------------

void check_lanes() {
    // DESIGN.md section 6, measured at D = 32 (groups x particles per group, two_colour)
    CHECK(lanes_per_particle(32, 256, DEMC_SCHED_TWO_COLOUR, 256) == 4);
    CHECK(lanes_per_particle(32, 256, DEMC_SCHED_TWO_COLOUR, 128) == 8);
    CHECK(lanes_per_particle(32, 128, DEMC_SCHED_TWO_COLOUR, 64) == 16);
    CHECK(lanes_per_particle(32, 16, DEMC_SCHED_TWO_COLOUR, 4) == 16);  // "and below"
    // long rows: a whole workgroup per particle from D = 2048 (256 lanes) and D = 4096 (512), else at most 64
    const int sched[] = {DEMC_SCHED_SEQUENTIAL, DEMC_SCHED_SYNCHRONOUS, DEMC_SCHED_TWO_COLOUR};
    for (int sc : sched)
        for (int groups : {1, 64, 4096}) {
            CHECK(lanes_per_particle(129, 16, sc, groups) == 64);
            CHECK(lanes_per_particle(2047, 16, sc, groups) == 64);
            CHECK(lanes_per_particle(2048, 16, sc, groups) == 256);
            CHECK(lanes_per_particle(4095, 16, sc, groups) == 256);
            CHECK(lanes_per_particle(4096, 16, sc, groups) == 512);
            CHECK(lanes_per_particle(10002, 16, sc, groups) == 512);
        }
    // never more lanes than pairs of scalars (rounded up to a power of two)
    CHECK(lanes_per_particle(1, 8, DEMC_SCHED_TWO_COLOUR, 2) == 1 && lanes_per_particle(5, 8, DEMC_SCHED_TWO_COLOUR, 2) == 4);
}

void check_workgroups() {
    // the lean SUFFSTAT kernel and the general resident kernel: 512 threads when the moving half of a group at four lanes a particle
    // needs more than 256, (Np - Np/2) * 4 > 256: Np = 128 takes 256 threads, Np = 130 takes 512 -- the smallest even such group
    // (of the odd ones, 129 moves 65 particles in its larger colour phase)
    int first512_lean = 0, first512_res = 0;
    for (int Np = 4; Np <= 200; ++Np) {
        Case full = mvn_full(8, 2, Np, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_SUFFSTAT);
        const FormGeo res_full = plan_resident(full.size());
        CHECK(res_full.ok);
        const LeanPlan lean = plan_lean(full.s, res_full.ok, StreamDims(), 3770);
        CHECK(lean.form[FORM_LEAN_SUFFSTAT].ok && lean.dt == 8);
        if (!first512_lean && lean.form[FORM_LEAN_SUFFSTAT].wg == 512) first512_lean = Np;
        CHECK(lean.form[FORM_LEAN_SUFFSTAT].wg == ((Np - Np / 2) * 4 > 256 ? 512 : 256) && res_full.wg == lean.form[FORM_LEAN_SUFFSTAT].wg);
        Case iso(FAM_MVN_ISO, 2, Np, 6, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT);
        iso.c.loglike_mode = DEMC_LOGLIKE_SUFFSTAT;
        iso.m.N = 64; iso.m.d = 5; iso.m.dpad = 8;
        const FormGeo res = plan_resident(iso.size());
        CHECK(res.ok && res.tail == TAIL_PREP && res.lpp == 4);
        if (!first512_res && res.wg == 512) first512_res = Np;
        if (Np == 128) CHECK(res.wg == 256 && lean.form[FORM_LEAN_SUFFSTAT].wg == 256);
        if (Np == 130) CHECK(res.wg == 512 && lean.form[FORM_LEAN_SUFFSTAT].wg == 512);
    }
    CHECK(first512_lean == 129 && first512_res == 129);
    {
        Case full = mvn_full(8, 2, 128, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_SUFFSTAT);
        CHECK(plan_lean(full.size(), true, StreamDims(), 3770).form[FORM_LEAN_SUFFSTAT].wg == 256);
        CHECK(!plan_lean(full.s, false, StreamDims(), 3770).form[FORM_LEAN_SUFFSTAT].ok);  // (only where the general resident form serves)
    }
    // DIRECT at D = 8: 512 threads whatever Np (while the moving half fits 256 lanes at four a particle)
    for (int Np : {4, 8, 64, 128}) {
        Case dir = mvn_full(8, 2, Np, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_DIRECT);
        const StreamPlan st = plan_stream(dir.size());
        CHECK(st.dims.ok && st.dims.x_lds == 1 && !st.form.ok);  // (DIRECT has no general streaming kernel)
        const LeanPlan lean = plan_lean(dir.s, false, st.dims, 3770);
        CHECK(lean.form[FORM_LEAN_DIRECT].ok && lean.form[FORM_LEAN_DIRECT].wg == 512 && !lean.form[FORM_LEAN_STREAMING].ok);
        // ... and STREAMING at the same shape keeps one wave per SIMD
        Case str = mvn_full(8, 2, Np, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_STREAMING);
        const StreamPlan ss = plan_stream(str.size());
        CHECK(ss.dims.ok && ss.form.ok && ss.form.tail == TAIL_PREP_MFMA);
        const LeanPlan ls = plan_lean(str.s, false, ss.dims, 3770);
        CHECK(ls.form[FORM_LEAN_STREAMING].ok && ls.form[FORM_LEAN_STREAMING].wg == 256 && !ls.form[FORM_LEAN_DIRECT].ok);
    }
    // DE-MC_Z: the same 130 rule
    for (int Np : {8, 128, 130}) {
        Case z = mvn_full(5, 2, Np, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY, DEMC_LOGLIKE_SUFFSTAT);
        const LeanPlan lean = plan_lean(z.size(), false, StreamDims(), 3770);
        CHECK(lean.form[FORM_LEAN_Z].ok && lean.form[FORM_LEAN_Z].wg == (Np == 130 ? 512 : 256) && lean.dt == 0 && !lean.iso);
        z.s.has_hist = false;
        CHECK(!plan_lean(z.s, false, StreamDims(), 3770).form[FORM_LEAN_Z].ok);
    }
    // no lean kernel knows a Normal(a, theta[ref]) prior or a table beyond its run-length form
    {
        Case full = mvn_full(8, 2, 8, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_SUFFSTAT);
        full.size().normal_ref = true;
        const LeanPlan a = plan_lean(full.s, true, StreamDims(), 3770);
        full.s.normal_ref = false; full.s.n_seg = 0;
        const LeanPlan b = plan_lean(full.s, true, StreamDims(), 3770);
        for (int f = 0; f < N_FORMS; ++f) CHECK(!a.form[f].ok && !b.form[f].ok);
    }
}

void check_row_length() {
    const int one[kMaxDimSeg] = {0}, two[kMaxDimSeg] = {0, 30}, other[kMaxDimSeg] = {0, 5};
    CHECK(compiled_row_length(FAM_MVN_FULL, 8, 1, one) == 8);
    CHECK(compiled_row_length(FAM_MVN_FULL, 32, 1, one) == 32);
    CHECK(compiled_row_length(FAM_MVN_FULL, 8, 2, other) == 0 && compiled_row_length(FAM_MVN_FULL, 32, 2, two) == 0);
    CHECK(compiled_row_length(FAM_MVN_FULL, 5, 1, one) == 0 && compiled_row_length(FAM_MVN_FULL, 16, 1, one) == 0);
    CHECK(compiled_row_length(FAM_MVN_ISO, 31, 2, two) == 31);
    CHECK(compiled_row_length(FAM_MVN_ISO, 31, 2, other) == 0 && compiled_row_length(FAM_MVN_ISO, 31, 1, one) == 0);
    CHECK(compiled_row_length(FAM_MVN_ISO, 6, 2, other) == 0 && compiled_row_length(FAM_MVN_ISO, 6, 1, one) == 0);
    CHECK(compiled_row_length(FAM_MVN_ISO, 8, 1, one) == 0 && compiled_row_length(FAM_MVN_ISO, 32, 1, one) == 0);
}

// ---- the K1 LDS carve-up --------------------------------------------------------------------------------------------------------

// tile | Np prefix sums (+ one per 16) | A^-1 | xbar | theta' scratch of one pass, in bytes, term by term
void check_carve(int family, int Np, int D, int d, int lpp, int line) {
    const bool mvn = family == FAM_MVN_FULL || family == FAM_MVN_ISO;
    const bool hier = family == FAM_HIER_BINOMIAL || family == FAM_HIER_GAUSSIAN;
    const long long cdf = 8LL * (Np + (Np + 15) / 16);
    long long ainv = family == FAM_MVN_FULL ? 8LL * d * d : 0;
    const bool ainv_in = ainv <= 40 * 1024;
    if (!ainv_in) ainv = 0;
    const long long xbar = mvn ? 8LL * d : 0;
    const long long pass = (lpp >= 256 ? 1 : 256 / lpp) * 8LL * (D + 2);
    const bool hier_scr = hier && pass <= 96 * 1024;
    const long long scratch = (mvn || family == FAM_GAUSSIAN || family == FAM_BINOMIAL || family == FAM_RASTRIGIN || hier_scr) ? pass : 0;
    long long tile = 8LL * Np * D;
    const bool tile_in = tile + cdf + ainv + xbar + scratch <= 96 * 1024;
    if (!tile_in) tile = 0;
    K1Lds k;
    const Refusal r = carve_k1_lds(family, d, Np, D, lpp, k);
    const bool ok = (long long)k.total == tile + cdf + ainv + xbar + scratch && (long long)k.tile_bytes == tile && (long long)k.cdf_bytes == cdf &&
                    (long long)k.ainv_bytes == ainv && (long long)k.xbar_bytes == xbar && (long long)k.scr_bytes == scratch &&
                    k.tile_in_lds == (tile_in ? 1 : 0) && k.ainv_lds == (ainv_in ? 1 : 0) && k.hier_scr == hier_scr;
    if (!ok) std::fprintf(stderr, "carve-up of the case at line %d differs\n", line);
    CHECK(ok);
    if (tile + cdf + ainv + xbar + scratch > 150 * 1024)
        CHECK(r.code == DEMC_EINVAL && r.message == "K1 LDS budget exceeded (Np too large for this D)");
    else
        CHECK(r.code == DEMC_OK && r.message.empty());
}
#define CARVE(family, Np, D, d, lpp) check_carve(family, Np, D, d, lpp, __LINE__)

void check_k1_lds() {
    // the shapes of tests/test_gpu_instance_selection.py (2 groups): MvNormal-full d = 5, 8, 32 and MvNormal-iso d = 5, 30 at
    // Np = 8 and 130, the Gaussian model, the hierarchical Binomial row of 4096 scalars
    for (int Np : {8, 130}) {
        for (int d : {5, 8, 32}) CARVE(FAM_MVN_FULL, Np, d, d, lanes_per_particle(d, Np, DEMC_SCHED_TWO_COLOUR, 2));
        for (int d : {5, 8, 32}) CARVE(FAM_MVN_FULL, Np, d, d, lanes_per_particle(d, Np, DEMC_SCHED_SYNCHRONOUS, 2));
        for (int d : {5, 30}) CARVE(FAM_MVN_ISO, Np, d + 1, d, lanes_per_particle(d + 1, Np, DEMC_SCHED_TWO_COLOUR, 2));
    }
    CARVE(FAM_GAUSSIAN, 8, 2, 0, 1);
    CARVE(FAM_HIER_BINOMIAL, 8, 4096, 0, 512);
    CARVE(FAM_LBA, 16, 7, 0, 4);  // (no scratch)
    // one of them by hand: MvNormal-full d = 8, Np = 8, four lanes a particle:
    // tile 8*8*8 = 512, cdf (8 + 1)*8 = 72, A^-1 8*8*8 = 512, xbar 64, scratch 64 rows * 10 * 8 = 5120
    {
        K1Lds k;
        CHECK(lanes_per_particle(8, 8, DEMC_SCHED_TWO_COLOUR, 2) == 4);
        CHECK(!carve_k1_lds(FAM_MVN_FULL, 8, 8, 8, 4, k) && k.total == 512 + 72 + 512 + 64 + 5120 && k.tile_in_lds == 1);
    }
    // the 96 KB tile limit, Gaussian (D = 2, one lane: 256 scratch rows of 4 doubles = 8192 bytes): 24 Np + 8 ceil(Np / 16) + 8192
    // is 98304 exactly at Np = 3678
    CARVE(FAM_GAUSSIAN, 3678, 2, 0, 1);
    CARVE(FAM_GAUSSIAN, 3679, 2, 0, 1);
    {
        K1Lds a, b;
        CHECK(!carve_k1_lds(FAM_GAUSSIAN, 0, 3678, 2, 1, a) && a.tile_in_lds == 1 && a.total == 96 * 1024);
        CHECK(!carve_k1_lds(FAM_GAUSSIAN, 0, 3679, 2, 1, b) && b.tile_in_lds == 0 && b.tile_bytes == 0 && b.total < a.total);
    }
    // the 40 KB limit of A^-1: d = 71 (40328 bytes) beside the tile, d = 72 (41472) read from L2
    CARVE(FAM_MVN_FULL, 8, 71, 71, 64);
    CARVE(FAM_MVN_FULL, 8, 72, 72, 64);
    {
        K1Lds a, b;
        CHECK(!carve_k1_lds(FAM_MVN_FULL, 71, 8, 71, 64, a) && a.ainv_lds == 1 && a.ainv_bytes == 40328);
        CHECK(!carve_k1_lds(FAM_MVN_FULL, 72, 8, 72, 64, b) && b.ainv_lds == 0 && b.ainv_bytes == 0);
    }
    // past what a launch may ask for: the prefix sums of 20 000 particles alone are 170 000 bytes
    CARVE(FAM_GAUSSIAN, 20000, 2, 0, 1);
    {
        K1Lds k;
        const Refusal r = carve_k1_lds(FAM_GAUSSIAN, 0, 20000, 2, 1, k);
        CHECK(r.code == DEMC_EINVAL && r.message == "K1 LDS budget exceeded (Np too large for this D)" && k.total > kMaxDynLds);
    }
}

// ---- tail flags -------------------------------------------------------------------------------------------------------------------

void check_tail_flags() {
    const int sched[] = {DEMC_SCHED_TWO_COLOUR, DEMC_SCHED_SYNCHRONOUS, DEMC_SCHED_SEQUENTIAL};
    const int partners[] = {DEMC_PARTNER_CURRENT, DEMC_PARTNER_HISTORY};
    for (int model = 0; model < 2; ++model)
        for (int sc : sched)
            for (int pk : partners)
                for (int fuse = 0; fuse <= 2; ++fuse)
                    for (int mode : {(int)MODE_STEP, (int)MODE_IDENT})
                        for (long long iter : {3LL, 4LL})  // burnin = 3: inside, past
                            for (int proposal_kind = 0; proposal_kind <= 1; ++proposal_kind)
                                for (int trace = 0; trace <= 1; ++trace) {
                                    Case k = model == 0 ? gaussian(2, 8, sc, pk) : mvn_full(8, 2, 8, sc, pk, DEMC_LOGLIKE_SUFFSTAT);
                                    k.c.fuse = fuse; k.c.proposal_kind = proposal_kind; k.c.trace = trace;
                                    k.size();
                                    const TailFlags t = tail_flags(k.s, k.s.lpp, mode, iter);
                                    // nothing a moving particle reads can move in the same launch: the four stated conditions
                                    const bool priv = sc == DEMC_SCHED_TWO_COLOUR || sc == DEMC_SCHED_SEQUENTIAL || mode == MODE_IDENT ||
                                                      (sc == DEMC_SCHED_SYNCHRONOUS && pk == DEMC_PARTNER_HISTORY && mode == MODE_STEP &&
                                                       !(proposal_kind == 0 && iter <= 3));
                                    CHECK(!t.fuse_accept || priv);
                                    CHECK(t.write_prop == (!t.fuse_accept || trace != 0));
                                    if (fuse == 1) CHECK(!t.fuse_obs && !t.fuse_accept);
                                    // ... and where they hold and fusing is allowed, these two models do fuse the whole update
                                    if (fuse != 1) CHECK(t.fuse_accept == priv);
                                    CHECK(t.fuse_obs == (model == 0 && priv && fuse != 1));
                                    CHECK(t.cheap_obs == (model == 0));
                                    CHECK(t.fuse_prep == (model == 1) && t.pass_sx == (model == 1) && t.pass_ainv == (model == 1));
                                    CHECK(t.prep_mfma == (model == 1));  // d = 8 at four lanes a particle
                                    CHECK(tail_of(t) == (model == 1 ? TAIL_PREP_MFMA : t.fuse_obs ? TAIL_OBS : TAIL_NONE));
                                }
    // STREAMING: the preparation is fused, the update is not; sx is not passed
    Case st = mvn_full(8, 2, 8, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_STREAMING);
    st.size();
    const TailFlags t = tail_flags(st.s, st.s.lpp, MODE_STEP, 1);
    CHECK(t.fuse_prep && !t.fuse_accept && !t.pass_sx && t.pass_ainv && t.write_prop);
    // lean levels: the default sampler 1, with snooker updates or blocks 2, anything else 0
    demc_config c = st.c;
    CHECK(lean_level(c, false, DEMC_PARTNER_CURRENT) == 1 && lean_level(c, false, DEMC_PARTNER_HISTORY) == 0);
    CHECK(lean_level(c, true, DEMC_PARTNER_CURRENT) == 0 && lean_level(c, false, DEMC_PARTNER_CURRENT, MODE_IDENT) == 0);
    c.theta_snooker = 0.1;
    CHECK(lean_level(c, false, DEMC_PARTNER_CURRENT) == 2);
    c.theta_snooker = 0.0; c.n_blocks = 2;
    CHECK(lean_level(c, false, DEMC_PARTNER_CURRENT) == 2);
    c.trace = 1;
    CHECK(lean_level(c, false, DEMC_PARTNER_CURRENT) == 0);
}

// ---- the per-phase plan -------------------------------------------------------------------------------------------------------------

int fit_asked = 0;
bool fit_yes(size_t) { ++fit_asked; return true; }
bool fit_no(size_t) { ++fit_asked; return false; }
bool fit_never(size_t) {
    CHECK(!"the long-row occupancy is asked only where it decides");
    return false;
}

// the whole group moves, partners from the whole group (the synchronous schedule)
Phase whole_phase(const Case& k, long long iter) {
    Phase p;
    p.n_groups = k.c.n_groups; p.a_lo = 0; p.n_act = k.c.Np; p.pool_lo = 0; p.pool_n = k.c.Np; p.iter = iter;
    p.lpp = k.s.lpp; p.lpp3 = k.s.lpp > 256 ? 256 : k.s.lpp; p.tile_in_lds = k.k1.tile_in_lds != 0;
    return p;
}

void check_snapshot() {
    // DE-MC_Z: synchronous, partners from the history, random_gamma (proposal_kind 0), cheap observations
    Case k = gaussian(2, 8, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY);
    k.size();
    const PhasePlan inside = plan_phase(k.s, whole_phase(k, 3), fit_never);
    CHECK(inside.snap == SNAP_WHOLE && inside.t.fuse_accept && inside.t.fuse_obs && !inside.t.write_prop && !inside.chain);
    CHECK(inside.kernel == K1_PROPOSE && !inside.tile && inside.tail == TAIL_OBS && inside.wg == 256);
    const PhasePlan past = plan_phase(k.s, whole_phase(k, 4), fit_never);
    CHECK(past.snap == SNAP_NONE && past.t.fuse_accept && !past.chain);
    {
        Case tr = gaussian(2, 8, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY);
        tr.c.trace = 1;
        tr.size();
        const PhasePlan p = plan_phase(tr.s, whole_phase(tr, 3), fit_never);
        CHECK(p.snap == SNAP_NONE && !p.t.fuse_accept && p.chain && p.t.write_prop && p.lean == 0);
    }
    {
        k.s.replay = true;
        const PhasePlan p = plan_phase(k.s, whole_phase(k, 3), fit_never);
        CHECK(p.snap == SNAP_NONE && !p.t.fuse_accept && p.chain && p.lean == 0);
        k.s.replay = false;
    }
    // rows under evaluation (not the population's own) take no snapshot; the by-product snapshot serves the sweep it was written for
    Phase p = whole_phase(k, 3);
    p.live = false;
    CHECK(plan_phase(k.s, p, fit_never).snap == SNAP_NONE);
    p.live = true; p.snap2 = true; p.snap2_iter = 3; p.snap2_sweep = 0;
    CHECK(plan_phase(k.s, p, fit_never).snap == SNAP_REUSE);
    p.snap2_sweep = 1;
    CHECK(plan_phase(k.s, p, fit_never).snap == SNAP_WHOLE);
    p.snap2_sweep = 0; k.s.subset = true;
    CHECK(plan_phase(k.s, p, fit_never).snap == SNAP_WHOLE);
    k.s.subset = false;
    // MvNormal in SUFFSTAT mode takes the same snapshot
    Case m = mvn_full(5, 2, 8, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY, DEMC_LOGLIKE_SUFFSTAT);
    m.size();
    const PhasePlan mp = plan_phase(m.s, whole_phase(m, 3), fit_never);
    CHECK(mp.snap == SNAP_WHOLE && mp.t.fuse_accept && !mp.t.fuse_obs && !mp.chain && mp.tail == TAIL_PREP_MFMA);
}

// hierarchical Binomial, 4094 subjects: D = 4096 (even), 512 lanes a particle; DE-MC_Z past burn-in, one block
Case frozen_case(int n_groups, int Np) {
    Case k = hier_binomial(4094, n_groups, Np, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY);
    k.c.n_blocks = 1;
    return k;  // (size() where it has come to rest)
}
Phase block_phase(const Case& k, const int* start, int n_run, unsigned in) {
    Phase p = whole_phase(k, 4);
    p.masked = true; p.n_mrun = n_run; p.mrun_in = in; p.mrun_start = start;
    return p;
}

void check_frozen() {
    const int three[kMaxMaskRun] = {0, 3};                     // scalars [0, 3) inside
    const int nine[kMaxMaskRun] = {0, kFrozenMax + 1};         // one scalar too many
    const int long_run[kMaxMaskRun] = {0, 2, 302};             // [2, 302): 300 scalars in one run
    const int at_limit[kMaxMaskRun] = {0, 2, 258};             // [2, 258): 256 scalars, not "longer than 256"
    Case k = frozen_case(64, 8);  // 512 moving particles = 2 x 256 CUs
    k.size();
    CHECK(k.s.lpp == 512 && k.k1.hier_scr && frozen_possible(k.s));
    {
        const PhasePlan p = plan_phase(k.s, block_phase(k, three, 2, 1u), fit_never);
        CHECK(p.kernel == K1_FROZEN && !p.big && p.wg == 256 && p.grid == 512 && p.lds == 0 && !p.chain && p.snap == SNAP_NONE);
        CHECK(!p.frozen_order && !p.write_snap2);
        const BlockSpan b = block_span(2, 1u, three, 4096);
        CHECK(b.inside == 3 && b.longest == 3);
    }
    {
        const PhasePlan p = plan_phase(k.s, block_phase(k, long_run, 3, 2u), fit_never);
        CHECK(p.kernel == K1_FROZEN && p.big && p.wg == 256 && p.grid == 512);
        const BlockSpan b = block_span(3, 2u, long_run, 4096);
        CHECK(b.inside == 300 && b.longest == 300);
    }
    {   // 256 scalars in a run: not the big instance, and too many for the small one
        fit_asked = 0;
        const PhasePlan p = plan_phase(k.s, block_phase(k, at_limit, 3, 2u), fit_no);
        CHECK(p.kernel == K1_LONGROW && fit_asked == 1);
    }
    {
        const PhasePlan p = plan_phase(k.s, block_phase(k, nine, 2, 1u), fit_yes);
        CHECK(p.kernel == K1_LONGROW && p.wg == 256);
        // ... and the last run of a mask ends at D
        const BlockSpan b = block_span(2, 2u, nine, 4096);
        CHECK(b.inside == 4096 - 9 && b.longest == 4096 - 9);
    }
    {   // the big instance needs even rows of the hierarchical Binomial family
        Case odd = hier_binomial(4095, 64, 8, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY);
        odd.c.n_blocks = 1;
        odd.size();
        CHECK(plan_phase(odd.s, block_phase(odd, long_run, 3, 2u), fit_yes).kernel == K1_LONGROW);
        CHECK(plan_phase(odd.s, block_phase(odd, three, 2, 1u), fit_never).kernel == K1_FROZEN);
    }
    {   // one particle fewer than 2 x CUs: 73 x 7 = 511
        Case few = frozen_case(73, 7);
        few.size();
        CHECK(!frozen_possible(few.s));
        fit_asked = 0;
        const PhasePlan p = plan_phase(few.s, block_phase(few, three, 2, 1u), fit_never);
        CHECK(p.kernel == K1_LONGROW && p.wg == 512 && fit_asked == 0);  // (too few for two a CU: the occupancy is not asked)
    }
    {   // the frozen-order table covers iterations [4, 6) of a whole-population step
        Phase p = block_phase(k, three, 2, 1u);
        p.frozen_order = true; p.frozen_iter0 = 4; p.frozen_iters = 2;
        CHECK(plan_phase(k.s, p, fit_never).frozen_order);
        p.iter = 6;
        CHECK(!plan_phase(k.s, p, fit_never).frozen_order);
        p.iter = 5; k.s.subset = true;
        CHECK(!plan_phase(k.s, p, fit_never).frozen_order);
        k.s.subset = false;
    }
    {   // inside burn-in a frozen sweep copies the block's columns only, and leaves the next sweep's snapshot behind
        Case two = frozen_case(64, 8);
        two.c.n_blocks = 2;
        two.size();
        Phase p = block_phase(two, three, 2, 1u);
        p.iter = 3; p.snap2 = true;
        const PhasePlan a = plan_phase(two.s, p, fit_never);
        CHECK(a.kernel == K1_FROZEN && a.snap == SNAP_BLOCK && a.write_snap2 && a.t.fuse_accept && !a.t.write_prop);
        p.sweep = 1; p.snap2_iter = 3; p.snap2_sweep = 1;  // the last sweep reads it and writes none
        const PhasePlan b = plan_phase(two.s, p, fit_never);
        CHECK(b.kernel == K1_FROZEN && b.snap == SNAP_REUSE && !b.write_snap2);
        p.sweep = 0; p.snap2 = false; p.snap2_iter = -1;
        CHECK(!plan_phase(two.s, p, fit_never).write_snap2);
    }
}

void check_longrow_grid() {
    // no block: the long-row kernel.  lds: the row rounded up to an even count of doubles (no cdf for a pool of at most 256)
    struct G { int n_cus, n_groups, Np; bool fit; int wg; long long grid; };
    const G cases[] = {
        {256, 64, 16, true, 256, 512},   // two a CU
        {256, 64, 16, false, 512, 256},  // one a CU
        {256, 8, 8, true, 512, 64},      // 64 proposals: too few for two a CU, clipped to the proposal count
        {10, 3, 7, true, 256, 20},       // 21 proposals on 10 CUs: 20, n_groups % 8 != 0 keeps it
        {10, 8, 3, true, 256, 16},       // 24 proposals, n_groups % 8 == 0: 20 rounded down to 16
        {10, 8, 3, false, 512, 8},       // ... 10 rounded down to 8
        {10, 1, 7, false, 512, 7},       // clipped to 7 proposals
        {12, 16, 1, true, 512, 8},       // 16 proposals < 24: one a CU, 12 rounded down to 8
        {3, 8, 1, false, 512, 3},        // below 8 nothing is rounded
    };
    for (const G& g : cases) {
        Case k = hier_binomial(4094, g.n_groups, g.Np, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY);
        k.s.n_cus = g.n_cus;
        k.size();
        const PhasePlan p = g.fit ? plan_phase(k.s, whole_phase(k, 4), fit_yes) : plan_phase(k.s, whole_phase(k, 4), fit_no);
        const long long n_prop = (long long)g.n_groups * g.Np;
        long long want = (g.wg == 256 ? 2LL : 1LL) * g.n_cus;
        if (want > n_prop) want = n_prop;
        if (g.n_groups % 8 == 0 && want >= 8) want -= want % 8;
        if (!(p.kernel == K1_LONGROW && p.wg == g.wg && p.grid == g.grid))
            std::fprintf(stderr, "long-row grid: %d CUs, %d x %d: <%d> x %lld\n", g.n_cus, g.n_groups, g.Np, p.wg, p.grid);
        CHECK(p.kernel == K1_LONGROW && p.wg == g.wg && p.grid == g.grid && g.grid == want);
        CHECK(p.lds == 4096 * sizeof(double) && !p.chain && p.t.fuse_obs && p.t.fuse_accept);
    }
    // an odd row rounds up; a pool beyond 256 adds its prefix sums
    Case odd = hier_binomial(4095, 64, 300, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY);
    odd.size();
    const PhasePlan p = plan_phase(odd.s, whole_phase(odd, 4), fit_yes);
    CHECK(p.kernel == K1_LONGROW && p.lds == (4098 + 300 + 19) * sizeof(double));
    // fuse = 2 keeps the per-phase kernel, 512 threads (tests/test_gpu_instance_selection.py)
    Case f2 = hier_binomial(4094, 2, 8, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT);
    f2.c.fuse = 2; f2.c.trace = 1;
    f2.size();
    Phase ph = whole_phase(f2, 1);
    ph.n_act = 4; ph.pool_lo = 4; ph.pool_n = 4;
    const PhasePlan q = plan_phase(f2.s, ph, fit_never);
    CHECK(q.kernel == K1_PROPOSE && q.wg == 512 && !q.tile && q.tail == TAIL_OBS && q.lean == 0 && !q.chain);
}

void check_split() {
    // MvNormal-full d = 32, two_colour, sixteen lanes a particle: 16 particles a workgroup, 128 moving particles -> at most 8 slices
    for (int n_groups : {1, 2, 100, 300, 512, 513}) {
        Case k = mvn_full(32, n_groups, 256, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_STREAMING);
        k.size();
        Phase p = whole_phase(k, 1);
        p.lpp = p.lpp3 = 16;
        p.a_lo = 0; p.n_act = 128; p.pool_lo = 128; p.pool_n = 128;
        const PhasePlan pl = plan_phase(k.s, p, fit_never);
        int want = (512 + n_groups - 1) / n_groups;
        const int most = (128 + 15) / 16;
        if (want > most) want = most;
        if (want < 1) want = 1;
        CHECK(pl.n_split == want && pl.grid == (long long)n_groups * want);
        const int by_hand = n_groups == 1 ? 8 : n_groups == 2 ? 8 : n_groups == 100 ? 6 : n_groups == 300 ? 2 : 1;
        CHECK(pl.n_split == by_hand);
        // the moving half lies outside the pool: the tile holds the pool and the workgroup's own slice
        const int per_split = (128 + want - 1) / want;
        CHECK(pl.kernel == K1_PROPOSE && pl.chain && pl.own_in_pool == 0 && pl.tile_rows == 128 + per_split);
        CHECK(pl.k3_grid == ((long long)n_groups * 128 + 15) / 16);
        if (pl.tile) {
            const size_t tile = (size_t)pl.tile_rows * 32 * 8, rest = k.k1.total - k.k1.tile_bytes;
            const size_t plan = (size_t)per_split * (4 * 8 + 4 * 4);
            CHECK(pl.plan == (tile + rest + plan <= kMaxDynLds ? 1 : 0));
            CHECK(pl.lds == tile + rest + (pl.plan ? plan : 0));
        }
    }
}

// ---- the K2 plan ----------------------------------------------------------------------------------------------------------------

void check_loglike() {
    Occupancy occ;
    occ.direct = 6; occ.obs = 8; occ.lba_wave = 4;
    {   // cfg3 in DIRECT mode: 128 groups x 256 particles at once (synchronous), N = 10000: 128 blocks x 48 chunks
        Case k = mvn_full(32, 128, 256, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_DIRECT, 10000);
        const LoglikePlan p = plan_loglike(k.size(), 128 * 256, occ);
        CHECK(p.kind == K2_DIRECT_MVN && p.key[0] == 32 && p.grid_x == 128 && p.grid_y == 48 && p.n_chunks == 48 && p.n_partials == 48 && !p.refused);
        k.m.N = 100;  // chunks no shorter than 64 observations
        CHECK(plan_loglike(k.s, 128 * 256, occ).n_chunks == 1);
    }
    {   // the cross term on the matrix cores: chunks in multiples of 8, doubled while the grid is small and a chunk keeps 16 tiles
        Case k = mvn_full(32, 128, 256, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_CURRENT, DEMC_LOGLIKE_STREAMING, 10000);
        const LoglikePlan p = plan_loglike(k.size(), 128 * 256, occ);  // 128 particle tiles x 8 = 1024 workgroups: no doubling
        CHECK(p.kind == K2_CROSS_MFMA && p.key[0] == 8 && p.key[1] == 4 && p.n_chunks == 8 && p.grid_x == 1024 && p.grid_y == 1);
        CHECK(p.n_kpass == 1 && p.n_partials == 8 && p.k0_stride == 32 && p.part0_stride == 8);
        const LoglikePlan q = plan_loglike(k.s, 256, occ);  // one particle tile: 8 -> 16 -> 32 (625 tiles / 32 >= 16)
        CHECK(q.n_chunks == 32 && q.grid_x == 32 && q.n_chunks % 8 == 0);
        k.m.n_tiles = 4;  // fewer tiles than chunks: a chunk a tile
        CHECK(plan_loglike(k.s, 256, occ).n_chunks == 4);
        k.m.n_tiles = 625; k.m.n_kpass = 2; k.m.ks_t = 16;  // two passes over wide data share the workspace
        const LoglikePlan w = plan_loglike(k.s, 256, occ);
        CHECK(w.n_chunks == 32 && w.n_kpass == 2 && w.n_partials == 64 && w.k0_stride == 64 && w.part0_stride == 32 && w.key[0] == 16);
        k.m.n_kpass = 65;
        const LoglikePlan r = plan_loglike(k.s, 256, occ);
        CHECK(r.refused == DEMC_EINVAL && std::string(r.why) == "data dimension too large for the partial-sum workspace");
        k.c.loglike_mode = DEMC_LOGLIKE_SUFFSTAT;
        const LoglikePlan n = plan_loglike(k.s, 256, occ);
        CHECK(n.kind == K2_NONE && !n.refused && n.n_partials == 1);
    }
    {   // per-observation families: chunks of at least 32 observations; the Rastrigin function has none
        Case k = gaussian(64, 64, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_CURRENT, 100000);
        k.c.fuse = 1;
        const LoglikePlan p = plan_loglike(k.size(), 4096, occ);
        CHECK(p.kind == K2_OBS && p.grid_x == 16 && p.n_chunks == 64 && p.grid_y == 64 && p.n_partials == 64);  // 16 x nc of 2048 resident: the more chunks, the fuller the one round
        k.m.N = 100;
        CHECK(plan_loglike(k.s, 4096, occ).n_chunks == 3);
        k.s.family = FAM_RASTRIGIN;
        CHECK(plan_loglike(k.s, 4096, occ).n_chunks == 1);
        k.s.family = FAM_LBA; k.m.N = 10000; k.m.n_acc = 3;  // a wave per proposal: chunks of at least 1024 trials
        const LoglikePlan l = plan_loglike(k.s, 4096, occ);
        CHECK(l.kind == K2_LBA_WAVE && l.key[0] == 3 && l.grid_x == 1024 && l.n_chunks >= 1 && l.n_chunks <= 9 && l.grid_y == (unsigned)l.n_chunks);
        CHECK(l.n_chunks == 4);  // 1024 resident: every count fills whole rounds, four of them is the most
        k.m.n_acc = 2;
        CHECK(plan_loglike(k.s, 4096, occ).key[0] == 2);
        k.m.n_acc = 5;
        CHECK(plan_loglike(k.s, 4096, occ).key[0] == 0);
    }
    {   // the user's plug-in: enough chunks for 262144 threads, no shorter than 32 observations, within the workspace
        Case k(FAM_USER, 64, 64, 3, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_CURRENT);
        k.m.N = 100000;
        const LoglikePlan p = plan_loglike(k.size(), 4096, occ);
        CHECK(p.kind == K2_USER && p.n_chunks == 64 && p.grid_x == 16 && p.grid_y == 64 && p.n_partials == 64);
        CHECK(plan_loglike(k.s, 65536, occ).n_chunks == 4 && plan_loglike(k.s, 262144, occ).n_chunks == 1 && plan_loglike(k.s, 300000, occ).n_chunks == 1);
        k.m.N = 100;
        CHECK(plan_loglike(k.s, 4096, occ).n_chunks == 3);
        k.s.user_row = true;
        const LoglikePlan r = plan_loglike(k.s, 4096, occ);
        CHECK(r.kind == K2_USER_ROW && r.n_chunks == 1 && r.grid_x == 4096 && r.grid_y == 1 && r.n_partials == 1);
    }
    {
        Case k = hier_binomial(100, 4, 8, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_CURRENT);
        const LoglikePlan p = plan_loglike(k.size(), 32, occ);
        CHECK(p.kind == K2_HIER && p.grid_x == 32 && p.grid_y == 1 && p.n_partials == 1);
        k.s.family = -1;
        const LoglikePlan r = plan_loglike(k.s, 32, occ);
        CHECK(r.refused == DEMC_EUNSUPPORTED && std::string(r.why) == "model family not set or not registered");
    }
}

// ---- choosing a form --------------------------------------------------------------------------------------------------------------

void check_choose_form() {
    demc_config c{};
    c.kappa = 1.0;
    c.partner_kind = DEMC_PARTNER_CURRENT;
    bool all[N_FORMS], none[N_FORMS] = {};
    for (bool& b : all) b = true;
    // a replay always gives the phase form
    CHECK(choose_form(all, c, true, false) == FORM_PHASE && choose_form(all, c, true, true) == FORM_PHASE);
    CHECK(choose_form(none, c, false, false) == FORM_PHASE);
    // first match, in the order of the rules
    CHECK(choose_form(all, c, false, false) == FORM_LEAN_DIRECT);
    bool ok[N_FORMS];
    auto only = [&](std::initializer_list<Form> fs) {
        for (bool& b : ok) b = false;
        for (Form f : fs) ok[f] = true;
    };
    only({FORM_STREAM, FORM_LEAN_STREAMING, FORM_LEAN_SUFFSTAT, FORM_RESIDENT});
    CHECK(choose_form(ok, c, false, false) == FORM_LEAN_STREAMING);
    only({FORM_STREAM, FORM_RESIDENT});
    CHECK(choose_form(ok, c, false, false) == FORM_STREAM);
    only({FORM_LEAN_SUFFSTAT, FORM_LEAN_OBS, FORM_RESIDENT});
    CHECK(choose_form(ok, c, false, false) == FORM_LEAN_SUFFSTAT);
    only({FORM_LEAN_OBS, FORM_RESIDENT});
    CHECK(choose_form(ok, c, false, false) == FORM_LEAN_OBS);
    only({FORM_RESIDENT, FORM_LEAN_Z});
    CHECK(choose_form(ok, c, false, false) == FORM_RESIDENT);
    // a subset update never gives a spin-waiting form, whatever is planned; it may take the others
    for (int bits = 0; bits < (1 << N_FORMS); ++bits) {
        for (int f = 0; f < N_FORMS; ++f) ok[f] = (bits >> f) & 1;
        for (int variant = 0; variant < 3; ++variant) {
            demc_config v = c;
            if (variant == 1) v.theta_snooker = 0.1;
            if (variant == 2) v.trace = 1;
            const Form sub = choose_form(ok, v, false, true);
            CHECK(!spin_waiting(sub));
            CHECK(sub == FORM_PHASE || ok[sub]);
            const Form whole = choose_form(ok, v, false, false);
            CHECK(whole == FORM_PHASE || ok[whole]);
            if (variant != 0) CHECK(whole != FORM_LEAN_DIRECT && whole != FORM_LEAN_STREAMING && whole != FORM_LEAN_SUFFSTAT && whole != FORM_LEAN_OBS);
        }
    }
    only({FORM_LEAN_DIRECT, FORM_STREAM, FORM_LEAN_STREAMING, FORM_LEAN_SUFFSTAT});
    CHECK(choose_form(ok, c, false, true) == FORM_LEAN_SUFFSTAT);
    // with snooker updates or a trace the general kernels serve: the stream, then the resident one
    c.theta_snooker = 0.1;
    CHECK(choose_form(all, c, false, false) == FORM_STREAM && choose_form(all, c, false, true) == FORM_RESIDENT);
    // DE-MC_Z: the default sampler (level 1) and snooker updates (level 2) take the lean body; level 2 with blocks the phase form
    demc_config z{};
    z.kappa = 1.0;
    z.partner_kind = DEMC_PARTNER_HISTORY;
    only({FORM_LEAN_Z});
    CHECK(choose_form(ok, z, false, false) == FORM_LEAN_Z && choose_form(ok, z, false, true) == FORM_LEAN_Z);
    z.theta_snooker = 0.1;
    CHECK(lean_level(z, false, DEMC_PARTNER_HISTORY) == 2 && choose_form(ok, z, false, false) == FORM_LEAN_Z);
    z.n_blocks = 2;
    CHECK(lean_level(z, false, DEMC_PARTNER_HISTORY) == 2 && choose_form(ok, z, false, false) == FORM_PHASE);
    z.theta_snooker = 0.0;  // (blocks alone are level 2 as well)
    CHECK(choose_form(ok, z, false, false) == FORM_PHASE);
    z.n_blocks = 0; z.trace = 1;
    CHECK(choose_form(ok, z, false, false) == FORM_PHASE);
    // iterations one launch carries
    CHECK(iterations_per_launch(FORM_PHASE) == 1 && iterations_per_launch(FORM_LEAN_Z) == 1);
    CHECK(iterations_per_launch(FORM_STREAM) == 64 && iterations_per_launch(FORM_LEAN_STREAMING) == 64 && iterations_per_launch(FORM_LEAN_DIRECT) == 64);
    CHECK(iterations_per_launch(FORM_RESIDENT) == 1024 && iterations_per_launch(FORM_LEAN_SUFFSTAT) == 1024 && iterations_per_launch(FORM_LEAN_OBS) == 1024);
}

// ---- the pool of the weighted pick ------------------------------------------------------------------------------------------------

// select_base's cumulative weights: k_res_obs, k_res_mvn and k_frozen_sweep keep them in ONE wave's registers (wave_cdf<1 / 2 / 4>:
// 64 lanes x 4) and count the entries below t over sixteen chunks of 16 -- neither has a form for a pool beyond 256 entries.
// Brute force over every group size up to 1024: no plan hands one of them such a pool (two_colour: the larger colour, Np - Np / 2;
// the DE-MC_Z body and a synchronous frozen sweep: the whole group), and each reaches the largest pool its rule admits.
void check_pick_pools() {
    const int three[kMaxMaskRun] = {0, 3}, long_run[kMaxMaskRun] = {0, 2, 302};
    int most_obs = 0, most_two_colour = 0, most_z = 0, most_frozen = 0, first_longrow = 0;
    for (int Np = 4; Np <= 1024; ++Np) {
        const int colour = Np - Np / 2;
        {
            Case k = gaussian(2, Np, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT);
            if (plan_lean(k.size(), true, StreamDims(), 3770).form[FORM_LEAN_OBS].ok) {
                CHECK(colour <= 256);
                most_obs = std::max(most_obs, colour);
            }
        }
        for (int d : {5, 8, 32})
            for (int mode : {DEMC_LOGLIKE_SUFFSTAT, DEMC_LOGLIKE_STREAMING, DEMC_LOGLIKE_DIRECT}) {
                Case k = mvn_full(d, 2, Np, DEMC_SCHED_TWO_COLOUR, DEMC_PARTNER_CURRENT, mode, mode == DEMC_LOGLIKE_SUFFSTAT ? 64 : 4096);
                k.size();
                const LeanPlan lean = plan_lean(k.s, true, plan_stream(k.s).dims, 3770);
                for (int f : {FORM_LEAN_SUFFSTAT, FORM_LEAN_STREAMING, FORM_LEAN_DIRECT})
                    if (lean.form[f].ok) {
                        CHECK(colour <= 256);
                        most_two_colour = std::max(most_two_colour, colour);
                    }
                Case z = mvn_full(d, 2, Np, DEMC_SCHED_SYNCHRONOUS, DEMC_PARTNER_HISTORY, mode);
                if (plan_lean(z.size(), true, StreamDims(), 3770).form[FORM_LEAN_Z].ok) {
                    CHECK(Np <= 256);
                    most_z = std::max(most_z, Np);
                }
            }
        for (int sched : {DEMC_SCHED_SYNCHRONOUS, DEMC_SCHED_TWO_COLOUR}) {
            Case k = hier_binomial(4094, 1024, Np, sched, sched == DEMC_SCHED_SYNCHRONOUS ? DEMC_PARTNER_HISTORY : DEMC_PARTNER_CURRENT);
            k.c.n_blocks = 1;
            k.size();
            for (int ph = 0; ph < (sched == DEMC_SCHED_TWO_COLOUR ? 2 : 1); ++ph)
                for (int big = 0; big < 2; ++big) {
                    Phase p = big ? block_phase(k, long_run, 3, 2u) : block_phase(k, three, 2, 1u);
                    if (sched == DEMC_SCHED_TWO_COLOUR) {
                        p.a_lo = ph ? Np / 2 : 0; p.n_act = ph ? colour : Np / 2;
                        p.pool_lo = ph ? 0 : Np / 2; p.pool_n = ph ? Np / 2 : colour;
                    }
                    const PhasePlan pl = plan_phase(k.s, p, fit_yes);
                    CHECK(pl.kernel == K1_FROZEN || pl.kernel == K1_LONGROW);
                    if (pl.kernel == K1_FROZEN) {
                        CHECK(p.pool_n <= 256 && pl.big == (big != 0));
                        most_frozen = std::max(most_frozen, p.pool_n);
                    } else {
                        CHECK(p.pool_n > 256);  // (nothing else keeps this configuration from the frozen sweep)
                        if (!first_longrow) first_longrow = p.pool_n;
                        CHECK(pl.lds == (4096 + (size_t)p.pool_n + ((size_t)p.pool_n + 15) / 16) * sizeof(double));  // (its LDS form)
                    }
                }
        }
    }
    CHECK(most_obs == 256);         // Np = 511 and 512
    CHECK(most_two_colour == 128);  // four lanes a particle on at most 512 threads
    CHECK(most_z == 256);           // ... of which the DE-MC_Z body's pool is the whole group
    CHECK(most_frozen == 256 && first_longrow == 257);
}

}  // namespace

int main() {
    check_pick_pools();
    check_chunks();
    check_lanes();
    check_workgroups();
    check_row_length();
    check_k1_lds();
    check_tail_flags();
    check_snapshot();
    check_frozen();
    check_longrow_grid();
    check_split();
    check_loglike();
    check_choose_form();
    std::printf("%d checks, %d failures\n", checks, failures);
    if (failures) return 1;
    std::printf("geometry ok\n");
    return 0;
}
