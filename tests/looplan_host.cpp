// looplan_host.cpp -- csrc/demc_looplan.hpp on the CPU: the tail length M(S), the cap on the draws, every refusal of demc_loo with
// its code and text held literally, and the planner against brute force written here by other means (every observation in exactly
// one block and one tile, every draw in exactly one chunk, counted).  Built with the address and undefined-behaviour sanitizers by
// tests/test_loo_host.py; no GPU, no HIP runtime, no ROCm header.
//
// looplan_host --dump reads one request per line from stdin and prints what the header answers, for the Python restatement of the
// same arithmetic that the GPU tests import (tests/loo_cases.py: plan()):
//   const | P family direct N n_acc d dp S
#include "demc_looplan.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
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

bool refused_with(const Refusal& r, int code, const std::string& text) { return r.code == code && r.message == text; }

PwModel model(int family, bool direct, long long N, int n_acc = 0, int d = 0, int dp = 0) {
    PwModel m;
    m.family = family; m.direct = direct; m.N = N; m.n_acc = n_acc; m.d = d; m.dp = dp;
    return m;
}

// M(S) in integers: the smallest M with M >= S / 5 or M * M >= 9 S, whichever bound is the smaller
long long tail_by_integers(long long S) {
    long long a = (S + 4) / 5, b = 0;
    while (b * b < 9 * S) ++b;
    return std::min(a, b);
}

void tail_and_cap() {
    CHECK(loo_tail_len(1) == 1 && loo_tail_len(20) == 4 && loo_tail_len(21) == 5 && loo_tail_len(26) == 6 && loo_tail_len(130) == 26);
    CHECK(loo_tail_len(2000) == 135 && loo_tail_len(65536) == 768 && loo_tail_len(409600) == 1920 && loo_tail_len(kLooMaxDraws) == kLooMaxTail);
    for (long long S = 1; S <= 70000; ++S) CHECK(loo_tail_len(S) == tail_by_integers(S));
    for (long long S : {100000LL, 409600LL, 1LL << 20, (1LL << 22) - 1, 1LL << 22}) CHECK(loo_tail_len(S) == tail_by_integers(S) && loo_tail_len(S) <= kLooMaxTail);
    CHECK(kLooMaxDraws == 4194304 && DEMC_LOO_NTOTAL == 8 && DEMC_LOO_NPOINT == 6 && kLooCap > kLooMaxTail);
    CHECK(30 + (int)std::floor(std::sqrt((double)kLooMaxTail)) <= kLooFitMax);
    CHECK(!check_loo_draws(1) && !check_loo_draws(kLooMaxDraws));
    CHECK(refused_with(check_loo_draws(kLooMaxDraws + 1), DEMC_EINVAL,
                       "demc_loo: S = 4194305 draws are above the cap of 4194304 (DEMC_LOO_MAX_DRAWS: the tail of an observation is sorted in LDS); "
                       "pass a narrower window"));
    const LooPlan over = plan_loo(model(DEMC_FAM_GAUSSIAN, false, 10), kLooMaxDraws + 1);
    CHECK(over.refused.code == DEMC_EINVAL && !over.model && over.blocks == 0 && over.n_terms == 0);
    CHECK(over.refused.message.find("4194305") != std::string::npos && over.refused.message.find("narrower window") != std::string::npos);
    CHECK(refused_with(plan_loo(model(DEMC_FAM_GAUSSIAN, false, 10), 0).refused, DEMC_EINVAL, "demc_loo: no draws (S < 1)"));
}

void refusals() {
    PwFamily f;
    const std::string w = "demc_loo";
    for (int family : {DEMC_FAM_GAUSSIAN, DEMC_FAM_BINOMIAL, DEMC_FAM_LNR, DEMC_FAM_LBA})
        for (int direct = 0; direct < 2; ++direct) CHECK(!pw_family(PW_LOO, model(family, direct != 0, 10, 3), &f) && f != PW_NONE);
    CHECK(!pw_family(PW_LOO, model(DEMC_FAM_MVN_ISO, true, 10, 0, 5, 8), &f) && f == PW_MVN_ISO);
    CHECK(!pw_family(PW_LOO, model(DEMC_FAM_MVN_FULL, true, 10, 0, 5, 8), &f) && f == PW_MVN_FULL);
    const std::string mvn = w + ": the MvNormal families keep sums over the data in this likelihood mode, not its rows; create the handle with "
                                "loglike_mode = direct (DEMC_LOGLIKE_DIRECT) for per-observation terms";
    CHECK(refused_with(plan_loo(model(DEMC_FAM_MVN_FULL, false, 10, 0, 5, 8), 100).refused, DEMC_EUNSUPPORTED, mvn));
    CHECK(refused_with(plan_loo(model(DEMC_FAM_MVN_ISO, false, 10, 0, 5, 8), 100).model, DEMC_EUNSUPPORTED, mvn));
    const struct { int family; const char* name; } unserved[] = {
        {DEMC_FAM_HIER_BINOMIAL, "DEMC_FAM_HIER_BINOMIAL"}, {DEMC_FAM_HIER_GAUSSIAN, "DEMC_FAM_HIER_GAUSSIAN"}, {DEMC_FAM_RASTRIGIN, "DEMC_FAM_RASTRIGIN"},
        {DEMC_FAM_ODE_LV, "DEMC_FAM_ODE_LV"}, {DEMC_FAM_USER, "DEMC_FAM_USER (a hiprtc plug-in)"}, {kPwFamSim, "a simulation likelihood (demc_set_model_sim)"}};
    for (const auto& r : unserved) {
        const LooPlan p = plan_loo(model(r.family, false, 10), 100);
        CHECK(refused_with(p.refused, DEMC_EUNSUPPORTED, w + ": " + r.name + " has no per-observation log-density on the device") && p.blocks == 0 && p.n_cst == 0);
        CHECK(p.model.code == DEMC_EUNSUPPORTED);
    }
    CHECK(refused_with(plan_loo(model(-1, false, 0), 100).refused, DEMC_EINVAL, w + ": no model is set on this handle"));
    CHECK(refused_with(plan_loo(model(DEMC_FAM_LBA, false, 0, 3), 100).refused, DEMC_EINVAL, w + ": the model holds no observations (N < 1)"));
    // the window, under the call's own texts and in demc_waic's order: no history, rows, the model, the outputs, a sharded handle
    const char* rows = "bad rows: demc_loo needs at least one row of the history";
    const char* sharded = "sharded handle: demc_loo reads the whole history of one handle";
    const char* outputs = "demc_loo: total_out and pointwise_out are both NULL";
    const Refusal args{DEMC_EUNSUPPORTED, "the model's"};
    CHECK(std::string(kLooBadRows) == rows && std::string(kLooSharded) == sharded && std::string(kLooNoOutput) == outputs);
    CHECK(!check_pw_window(true, 0, 1, 1, false, loo_args(Refusal(), true), kLooBadRows, kLooSharded));
    CHECK(refused_with(check_pw_window(false, -1, 1, 1, true, loo_args(args, false), kLooBadRows, kLooSharded), DEMC_EINVAL, "history is not stored on this handle"));
    CHECK(refused_with(check_pw_window(true, -1, 1, 1, true, loo_args(args, false), kLooBadRows, kLooSharded), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 2, 2, 4, true, loo_args(args, false), kLooBadRows, kLooSharded), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 0, 5, 4, true, loo_args(args, false), kLooBadRows, kLooSharded), DEMC_EINVAL, rows));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, true, loo_args(args, false), kLooBadRows, kLooSharded), DEMC_EUNSUPPORTED, "the model's"));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, true, loo_args(Refusal(), false), kLooBadRows, kLooSharded), DEMC_EINVAL, outputs));
    CHECK(refused_with(check_pw_window(true, 0, 1, 1, true, loo_args(Refusal(), true), kLooBadRows, kLooSharded), DEMC_EINVAL, sharded));
    // demc_waic's own window texts are untouched by the borrowed check
    CHECK(refused_with(check_pw_window(true, -1, 1, 1, false), DEMC_EINVAL, "bad rows: demc_waic needs at least one row of the history"));
}

void plan_brute_force() {
    const long long Ns[] = {1, 5, 63, 64, 65, 257, 2048, 2049, 50000, 100000};
    const long long Ss[] = {1, 15, 16, 17, 20, 21, 26, 130, 2000, 65536, 65537, 409600, 1 << 22};
    for (long long N : Ns)
        for (long long S : Ss) {
            const LooPlan p = plan_loo(model(DEMC_FAM_LBA, false, N, 3), S);
            CHECK(!p.refused && !p.model && p.fam == PW_LBA && p.K == 13 && p.S == S);
            CHECK(p.M == (S <= 20 ? 0 : (int)tail_by_integers(S)) && p.M < kLooCap);
            // blocks: every observation in exactly one, none empty, each within the staging budget; only the last one ragged
            CHECK(p.Nb >= 1 && p.Nb <= N && (__int128)p.Nb * S <= kLooMaxCells && ((__int128)(p.Nb + 1) * S > kLooMaxCells || p.Nb == N));
            long long seen = 0;
            for (int b = 0; b < p.blocks; ++b) {
                const long long lo = (long long)b * p.Nb, nb = std::min<long long>(p.Nb, N - lo);
                CHECK(lo == seen && nb >= 1 && (b == p.blocks - 1 || nb == p.Nb));
                CHECK((nb + kLooObs - 1) / kLooObs <= p.tiles);  // the grid of a block never exceeds the full block's
                seen += nb;
            }
            CHECK(seen == N);
            CHECK((long long)p.tiles * kLooObs >= p.Nb && (long long)(p.tiles - 1) * kLooObs < p.Nb);
            // chunks: whole tiles of draws, every draw in exactly one, none empty
            CHECK(p.chunk_len % kLooTile == 0 && p.chunks >= 1 && p.chunks <= 65535);
            long long draws = 0;
            for (int c = 0; c < p.chunks; ++c) {
                const long long s0 = (long long)c * p.chunk_len, s1 = std::min<long long>(s0 + p.chunk_len, S);
                CHECK(s0 == draws && s1 > s0);
                draws = s1;
            }
            CHECK(draws == S);
            CHECK(p.prep_blocks >= 1 && p.lds_bytes == kLooLdsBytes && p.lds_bytes <= 160 * 1024);
            CHECK(p.n_cst == (size_t)S * 13 && p.n_terms == (size_t)p.Nb * (size_t)S && p.n_point == (size_t)N * 6 && p.n_total == 8);
        }
    // the shapes the tests and the documents name
    const LooPlan two = plan_loo(model(DEMC_FAM_GAUSSIAN, false, 2049), 65536);
    CHECK(two.Nb == 2048 && two.blocks == 2 && two.M == 768);
    const LooPlan cfg5 = plan_loo(model(DEMC_FAM_LBA, false, 50000, 3), 409600);
    CHECK(cfg5.Nb == 327 && cfg5.blocks == 153 && cfg5.M == 1920);
}

int dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "const") {
            std::printf("const kLooObs=%d kLooTile=%d kLooTargetWG=%d kLooWG=%d kLooCap=%d kLooMaxTail=%d kLooBits=%d kLooMaxDraws=%lld kLooMaxCells=%lld "
                        "kLooLdsBytes=%zu DEMC_LOO_NTOTAL=%d DEMC_LOO_NPOINT=%d\n", kLooObs, kLooTile, kLooTargetWG, kLooWG, kLooCap, kLooMaxTail, kLooBits,
                        kLooMaxDraws, kLooMaxCells, kLooLdsBytes, DEMC_LOO_NTOTAL, DEMC_LOO_NPOINT);
        } else if (kind == "P") {
            int family, direct, n_acc, d, dp;
            long long N, S;
            if (!(in >> family >> direct >> N >> n_acc >> d >> dp >> S)) return 2;
            const LooPlan p = plan_loo(model(family, direct != 0, N, n_acc, d, dp), S);
            if (p.refused) {
                std::printf("P refused=%d message=%s\n", p.refused.code, p.refused.message.c_str());
                continue;
            }
            std::printf("P refused=0 fam=%d K=%d S=%lld M=%d Nb=%lld blocks=%d tiles=%d chunks=%d chunk_len=%lld prep_blocks=%d n_cst=%zu n_terms=%zu n_point=%zu "
                        "n_total=%zu\n", (int)p.fam, p.K, p.S, p.M, p.Nb, p.blocks, p.tiles, p.chunks, p.chunk_len, p.prep_blocks, p.n_cst, p.n_terms, p.n_point, p.n_total);
        } else
            return 2;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) return dump();
    tail_and_cap();
    refusals();
    plan_brute_force();
    if (failures) std::fprintf(stderr, "%d of %d checks failed\n", failures, checks);
    else std::printf("looplan ok: %d checks\n", checks);
    return failures ? 1 : 0;
}
