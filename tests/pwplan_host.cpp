// pwplan_host.cpp -- csrc/demc_pwplan.hpp on the CPU: which families the per-observation calls serve, every refusal's code and text
// held literally, the cell cap, and the planner against brute force written here by other means (every observation in exactly one
// tile, every draw in exactly one chunk, counted).  Built with the address and undefined-behaviour sanitizers by
// tests/test_pwplan_host.py; no GPU, no HIP runtime, no ROCm header.
//
// pwplan_host --dump reads one request per line from stdin and prints what the header answers, for the Python restatement of the
// same arithmetic that the GPU tests import (tests/test_pwplan_host.py: geometry()):
//   const | P call family direct N n_acc d dp S D       (call: 0 demc_pointwise_loglik, 1 demc_waic)
#include "demc_pwplan.hpp"

#include <cstdio>
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

bool refused_with(const Refusal& r, int code, const std::string& text) { return r.code == code && r.message == text; }

PwModel model(int family, bool direct, long long N, int n_acc = 0, int d = 0, int dp = 0) {
    PwModel m;
    m.family = family; m.direct = direct; m.N = N; m.n_acc = n_acc; m.d = d; m.dp = dp;
    return m;
}

// ---- families and refusals --------------------------------------------------------------------------------------------------------
void families() {
    PwFamily f;
    const struct { int family; PwFamily want; } served[] = {{DEMC_FAM_GAUSSIAN, PW_GAUSSIAN}, {DEMC_FAM_BINOMIAL, PW_BINOMIAL}, {DEMC_FAM_LNR, PW_LNR}, {DEMC_FAM_LBA, PW_LBA}};
    for (const auto& s : served)
        for (int direct = 0; direct < 2; ++direct)  // any likelihood mode
            for (int call = 0; call < 2; ++call) {
                CHECK(!pw_family((PwCall)call, model(s.family, direct != 0, 10, 3), &f) && f == s.want);
            }
    CHECK(!pw_family(PW_WAIC, model(DEMC_FAM_MVN_ISO, true, 10, 0, 5, 8), &f) && f == PW_MVN_ISO);
    CHECK(!pw_family(PW_WAIC, model(DEMC_FAM_MVN_FULL, true, 10, 0, 5, 8), &f) && f == PW_MVN_FULL);
    const char* who[2] = {"demc_pointwise_loglik", "demc_waic"};
    for (int call = 0; call < 2; ++call) {
        const std::string w = who[call];
        const std::string mvn = w + ": the MvNormal families keep sums over the data in this likelihood mode, not its rows; create the handle with "
                                    "loglike_mode = direct (DEMC_LOGLIKE_DIRECT) for per-observation terms";
        CHECK(refused_with(pw_family((PwCall)call, model(DEMC_FAM_MVN_ISO, false, 10, 0, 5, 8), &f), DEMC_EUNSUPPORTED, mvn) && f == PW_NONE);
        CHECK(refused_with(pw_family((PwCall)call, model(DEMC_FAM_MVN_FULL, false, 10, 0, 5, 8), &f), DEMC_EUNSUPPORTED, mvn));
        CHECK(mvn.find("loglike_mode = direct") != std::string::npos);
        const struct { int family; const char* name; } refused[] = {
            {DEMC_FAM_HIER_BINOMIAL, "DEMC_FAM_HIER_BINOMIAL"}, {DEMC_FAM_HIER_GAUSSIAN, "DEMC_FAM_HIER_GAUSSIAN"}, {DEMC_FAM_RASTRIGIN, "DEMC_FAM_RASTRIGIN"},
            {DEMC_FAM_ODE_LV, "DEMC_FAM_ODE_LV"}, {DEMC_FAM_USER, "DEMC_FAM_USER (a hiprtc plug-in)"}, {kPwFamSim, "a simulation likelihood (demc_set_model_sim)"}};
        for (const auto& r : refused)
            for (int direct = 0; direct < 2; ++direct)
                CHECK(refused_with(pw_family((PwCall)call, model(r.family, direct != 0, 10), &f), DEMC_EUNSUPPORTED,
                                   w + ": " + r.name + " has no per-observation log-density on the device"));
        CHECK(refused_with(pw_family((PwCall)call, model(-1, false, 0), &f), DEMC_EINVAL, w + ": no model is set on this handle"));
        // a served family without an observation (prep_race accepts dims = [0, n_acc]): refused before any plan divides by its tiles
        for (int family : {DEMC_FAM_LBA, DEMC_FAM_LNR, DEMC_FAM_GAUSSIAN, DEMC_FAM_BINOMIAL, DEMC_FAM_MVN_ISO, DEMC_FAM_MVN_FULL})
            for (long long N : {0LL, -1LL}) {
                CHECK(refused_with(pw_family((PwCall)call, model(family, true, N, 3, 4, 8), &f), DEMC_EINVAL, w + ": the model holds no observations (N < 1)") && f == PW_NONE);
                const PwPlan none = plan_pointwise((PwCall)call, model(family, true, N, 3, 4, 8), 12, 6);
                CHECK(refused_with(none.refused, DEMC_EINVAL, w + ": the model holds no observations (N < 1)") && none.tiles == 0 && none.chunks == 0 && none.n_cst == 0);
            }
        CHECK(pw_family((PwCall)call, model(DEMC_FAM_MVN_FULL, false, 0, 0, 4, 8), &f).code == DEMC_EUNSUPPORTED);  // (the mode is what is wrong first)
        CHECK(pw_family((PwCall)call, model(DEMC_FAM_RASTRIGIN, false, 0), &f).code == DEMC_EUNSUPPORTED);
        // the planner carries the refusal and plans nothing
        const PwPlan p = plan_pointwise((PwCall)call, model(DEMC_FAM_RASTRIGIN, false, 1), 10, 2);
        CHECK(p.refused.code == DEMC_EUNSUPPORTED && p.tiles == 0 && p.chunks == 0 && p.n_cst == 0);
    }
}

void window_and_rows() {
    const char* rows = "bad rows: demc_waic needs at least one row of the history";
    const char* sharded = "sharded handle: gather demc_get_history from every rank and evaluate demc_pointwise_loglik on one";
    const Refusal args{DEMC_EUNSUPPORTED, "the model's"};
    CHECK(!check_pw_window(true, 0, 1, 1, false) && !check_pw_window(true, 3, 10, 10, false));
    CHECK(refused_with(check_pw_window(false, 0, 1, 1, false), DEMC_EINVAL, "history is not stored on this handle"));
    CHECK(refused_with(check_pw_window(true, -1, 1, 1, false), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 1, 1, 1, false), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 2, 1, 4, false), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 0, 5, 4, false), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, false, args), DEMC_EUNSUPPORTED, "the model's"));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, true), DEMC_EINVAL, sharded));
    // ... and in the order of check_history_window: no history, rows, the call's own, sharded
    CHECK(refused_with(check_pw_window(false, -1, 1, 1, true, args), DEMC_EINVAL, "history is not stored on this handle"));
    CHECK(refused_with(check_pw_window(true, -1, 1, 1, true, args), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, true, args), DEMC_EUNSUPPORTED, "the model's"));
    CHECK(std::string(kPwNoOutput) == "demc_waic: total_out and pointwise_out are both NULL");
    // the call's own: what it has against the model first, then against its outputs; both rank between the rows and the sharded handle
    CHECK(!pw_waic_args(Refusal(), true) && refused_with(pw_waic_args(Refusal(), false), DEMC_EINVAL, kPwNoOutput));
    CHECK(refused_with(pw_waic_args(args, false), DEMC_EUNSUPPORTED, "the model's"));
    CHECK(refused_with(check_pw_window(true, -1, 1, 1, true, pw_waic_args(Refusal(), false)), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, true, pw_waic_args(Refusal(), false)), DEMC_EINVAL, kPwNoOutput));

    // demc_pointwise_loglik: n < 1, the cell cap
    CHECK(kPwMaxCells == (1LL << 27) && DEMC_PW_MAX_CELLS == 134217728);
    CHECK(refused_with(check_pw_rows(0, 10), DEMC_EINVAL, "demc_pointwise_loglik: n < 1"));
    CHECK(refused_with(check_pw_rows(-3, 10), DEMC_EINVAL, "demc_pointwise_loglik: n < 1"));
    const char* cap = "demc_pointwise_loglik: n N = 134217729 x 1 is above the cap of 134217728 cells (DEMC_PW_MAX_CELLS: the matrix is staged on the device); "
                      "pass fewer rows per call";
    CHECK(!check_pw_rows(1LL << 27, 1) && refused_with(check_pw_rows((1LL << 27) + 1, 1), DEMC_EINVAL, cap));
    for (long long N : {1LL, 7LL, 50000LL, 100000LL, 1LL << 27, (1LL << 27) + 1, 1LL << 40})
        for (long long n : {1LL, 2LL, 1342LL, 1343LL, 2684LL, 2685LL, 1LL << 20, 1LL << 27, 1LL << 45}) {
            const bool over = (__int128)n * N > (__int128)kPwMaxCells;  // the product itself, in arithmetic that cannot wrap
            CHECK((check_pw_rows(n, N).code == DEMC_EINVAL) == over);
        }
    const PwPlan p = plan_pointwise(PW_LOGLIK, model(DEMC_FAM_GAUSSIAN, false, 100000), 1343, 2);
    CHECK(p.refused.code == DEMC_EINVAL && p.refused.message.find("above the cap") != std::string::npos);
    CHECK(!plan_pointwise(PW_LOGLIK, model(DEMC_FAM_GAUSSIAN, false, 100000), 1342, 2).refused);
    CHECK(!plan_pointwise(PW_WAIC, model(DEMC_FAM_GAUSSIAN, false, 100000), 409600, 2).refused);  // the cap is the matrix's, not demc_waic's
    CHECK(refused_with(plan_pointwise(PW_WAIC, model(DEMC_FAM_GAUSSIAN, false, 10), 0, 2).refused, DEMC_EINVAL, "demc_waic: no draws (S < 1)"));
    CHECK(refused_with(plan_pointwise(PW_WAIC, model(DEMC_FAM_GAUSSIAN, false, 10), (1LL << 40) + 1, 2).refused, DEMC_EINVAL, "demc_waic: too many draws"));
    CHECK(!plan_pointwise(PW_WAIC, model(DEMC_FAM_GAUSSIAN, false, 10), 1LL << 40, 2).refused);
}

// ---- the plan against brute force --------------------------------------------------------------------------------------------------
void constants_per_draw() {
    CHECK(pw_constants(PW_GAUSSIAN, 0, 0) == 4 && pw_constants(PW_BINOMIAL, 0, 0) == 3 && pw_constants(PW_LNR, 3, 0) == 5);
    CHECK(pw_constants(PW_LBA, 3, 0) == 13 && pw_constants(PW_LBA, 8, 0) == 23 && pw_constants(PW_MVN_ISO, 0, 32) == 35 && pw_constants(PW_MVN_FULL, 0, 8) == 9);
}

void plan_brute_force() {
    const long long Ns[] = {1, 63, 64, 65, 130, 255, 256, 257, 511, 513, 50000, 100000, 524288, 524289, 3000000};
    const long long Ss[] = {1, 3, 63, 64, 65, 127, 128, 129, 130, 192, 193, 1000, 4095, 65536, 65537, 409600, 1 << 20};
    for (long long N : Ns)
        for (long long S : Ss)
            for (int call = 0; call < 2; ++call) {
                if (call == PW_LOGLIK && (__int128)S * N > kPwMaxCells) continue;
                const PwPlan p = plan_pointwise((PwCall)call, model(DEMC_FAM_LBA, false, N, 3), S, 6);
                CHECK(!p.refused && p.fam == PW_LBA && p.K == 13 && p.S == S);
                // tiles: every observation in exactly one -- the kernel's own indexing, i = tile kPwWG + lane, counted
                long long seen = 0, first_uncovered = 0;
                for (int t = 0; t < p.tiles; ++t) {
                    const long long lo = (long long)t * kPwWG, hi = std::min<long long>(lo + kPwWG, N);
                    CHECK(lo == first_uncovered && hi > lo);
                    seen += hi - lo;
                    first_uncovered = hi;
                }
                CHECK(seen == N && first_uncovered == N);
                // chunks: every draw in exactly one, none empty, none longer than chunk_len; only the last one ragged
                long long draws = 0, next = 0;
                for (int c = 0; c < p.chunks; ++c) {
                    const long long s0 = (long long)c * p.chunk_len, s1 = std::min<long long>(s0 + p.chunk_len, S);
                    CHECK(s0 == next && s1 > s0 && (c == p.chunks - 1 || s1 - s0 == p.chunk_len));
                    draws += s1 - s0;
                    next = s1;
                }
                CHECK(draws == S && next == S);
                CHECK(p.chunks >= 1 && p.chunks <= kPwMaxChunks);
                // no chunk count below this one would have done: a launch reaches kPwTargetWG workgroups, or has no draws left to
                // split (chunks of at least kPwMinChunk), or is at the cap
                const bool full = (long long)p.tiles * p.chunks >= kPwTargetWG - p.tiles || p.chunks == kPwMaxChunks;
                CHECK(full || p.chunk_len < 2 * kPwMinChunk || p.tiles > kPwTargetWG);
                CHECK(p.chunks == 1 || p.chunk_len >= kPwMinChunk / 2);
                CHECK(p.prep_blocks >= 1 && (long long)p.prep_blocks * kPwPrepWG >= std::min<long long>(S, (long long)kPwPrepWG << 20));
                CHECK(p.final_blocks == p.tiles && p.n_cst == (size_t)S * 13);
                if (call == PW_WAIC)
                    CHECK(p.n_part == (size_t)p.chunks * 5 * (size_t)N && p.n_point == (size_t)N * 4 && p.n_total == 8 && p.n_matrix == 0 && p.n_theta == 0);
                else
                    CHECK(p.n_matrix == (size_t)S * (size_t)N && p.n_theta == (size_t)S * 6 && p.n_part == 0 && p.n_point == 0 && p.n_total == 0);
            }
    // the shapes the documents name: cfg5's share and the Gaussian of tools/waic_bench.py
    const PwPlan lba = plan_pointwise(PW_WAIC, model(DEMC_FAM_LBA, false, 50000, 3), 409600, 6);
    CHECK(lba.tiles == 196 && lba.chunks == 10 && lba.chunk_len == 40960);
    const PwPlan g = plan_pointwise(PW_WAIC, model(DEMC_FAM_GAUSSIAN, false, 100000), 409600, 2);
    CHECK(g.tiles == 391 && g.chunks == 5 && g.chunk_len == 81920);
    // a small model: the draws alone fill the chip
    const PwPlan s = plan_pointwise(PW_WAIC, model(DEMC_FAM_GAUSSIAN, false, 65), 130, 2);
    CHECK(s.tiles == 1 && s.chunks == 3 && s.chunk_len == 44);
}

// ---- --dump -----------------------------------------------------------------------------------------------------------------------
int dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "const") {
            std::printf("const kPwWG=%d kPwMinChunk=%d kPwTargetWG=%d kPwMaxChunks=%d kPwPartial=%d kPwPrepWG=%d kPwTotalsWG=%d kPwMaxCells=%lld DEMC_WAIC_NTOTAL=%d "
                        "DEMC_WAIC_NPOINT=%d\n", kPwWG, kPwMinChunk, kPwTargetWG, kPwMaxChunks, kPwPartial, kPwPrepWG, kPwTotalsWG, kPwMaxCells, DEMC_WAIC_NTOTAL,
                        DEMC_WAIC_NPOINT);
        } else if (kind == "P") {
            int call, family, direct, n_acc, d, dp, D;
            long long N, S;
            if (!(in >> call >> family >> direct >> N >> n_acc >> d >> dp >> S >> D)) return 2;
            const PwPlan p = plan_pointwise((PwCall)call, model(family, direct != 0, N, n_acc, d, dp), S, D);
            if (p.refused) {
                std::printf("P refused=%d message=%s\n", p.refused.code, p.refused.message.c_str());
                continue;
            }
            std::printf("P refused=0 fam=%d K=%d S=%lld tiles=%d chunks=%d chunk_len=%lld prep_blocks=%d final_blocks=%d n_cst=%zu n_part=%zu n_point=%zu n_total=%zu "
                        "n_matrix=%zu n_theta=%zu\n", (int)p.fam, p.K, p.S, p.tiles, p.chunks, p.chunk_len, p.prep_blocks, p.final_blocks, p.n_cst, p.n_part, p.n_point,
                        p.n_total, p.n_matrix, p.n_theta);
        } else
            return 2;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) return dump();
    families();
    window_and_rows();
    constants_per_draw();
    plan_brute_force();
    if (failures) std::fprintf(stderr, "%d of %d checks failed\n", failures, checks);
    else std::printf("pwplan ok: %d checks\n", checks);
    return failures ? 1 : 0;
}
