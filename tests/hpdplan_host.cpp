// hpdplan_host.cpp -- csrc/demc_hpdplan.hpp on the CPU: every refusal of demc_hpd with its code and text held literally, the number
// of candidates against integer arithmetic where alpha N is exact, and the planner against brute force written here by other means
// (every candidate of every alpha in exactly one (workgroup, thread, trip) of the window kernel, every series in exactly one batch,
// the batch within the budget, the sort of one series as csrc/demc_rankplan.hpp plans it).  Built with the address and
// undefined-behaviour sanitizers by tests/test_hpd_host.py, with -ffp-contract=off as the library is; no GPU, no HIP runtime, no ROCm
// header.
//
// hpdplan_host --dump reads one request per line from stdin and prints what the header answers, for the Python restatement of the
// same arithmetic (tests/test_hpd_host.py: geometry()):
//   const | H n P series alpha [alpha ...] (C99 hex floats)
#include "demc_hpdplan.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
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

void refusals() {
    const Refusal none;
    const double ok[3] = {0.05, 0.5, 0.999};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    CHECK(!hpd_args(true, ok, 1) && !hpd_args(true, ok, 3));
    CHECK(refused_with(hpd_args(false, ok, 3), DEMC_EINVAL, "demc_hpd: out is NULL"));
    CHECK(refused_with(hpd_args(false, nullptr, 0), DEMC_EINVAL, "demc_hpd: out is NULL"));
    CHECK(refused_with(hpd_args(true, nullptr, 3), DEMC_EINVAL, "demc_hpd: alphas is NULL"));
    std::vector<double> many(17, 0.5);
    for (int n : {0, -1, 17}) CHECK(refused_with(hpd_args(true, many.data(), n), DEMC_EINVAL, "demc_hpd: n_alphas must be between 1 and 16"));
    CHECK(!hpd_args(true, many.data(), 16));
    for (double bad : {0.0, 1.0, -0.0, -0.05, 1.5, inf, -inf, nan}) {
        const double a[2] = {0.5, bad};
        CHECK(refused_with(hpd_args(true, a, 2), DEMC_EINVAL, "demc_hpd: every alpha must be finite and strictly inside (0, 1)"));
        CHECK(!hpd_args(true, a, 1));
    }
    const double edge[2] = {std::nextafter(0.0, 1.0), std::nextafter(1.0, 0.0)};
    CHECK(!hpd_args(true, edge, 2));
    // the window, in the order of the other posterior-statistics calls: history, rows, arguments, sharded, then the cap
    const Refusal arg = hpd_args(false, ok, 3);
    CHECK(refused_with(check_hpd_window(false, -1, 0, 10, true, 8, arg), DEMC_EINVAL, "demc_hpd: history is not stored on this handle"));
    for (auto rows : {std::pair<long long, long long>{-1, 5}, {0, 11}, {5, 5}, {6, 5}})
        CHECK(refused_with(check_hpd_window(true, rows.first, rows.second, 10, true, 8, arg), DEMC_EINVAL,
                           "bad rows: demc_hpd needs at least one row of the history"));
    CHECK(refused_with(check_hpd_window(true, 0, 10, 10, true, 8, arg), DEMC_EINVAL, "demc_hpd: out is NULL"));
    CHECK(refused_with(check_hpd_window(true, 0, 10, 10, true, 8, none), DEMC_EINVAL,
                       "sharded handle: gather demc_get_history from every rank and take the intervals of the pool on the host"));
    CHECK(!check_hpd_window(true, 0, 10, 10, false, 8, none) && !check_hpd_window(true, 9, 10, 10, false, 1, none));
    const char* too_many = "demc_hpd: N = n P is 2^31 or more, positions in the pool are 32-bit; pass a narrower window";
    CHECK(refused_with(check_hpd_window(true, 0, 1LL << 21, 1LL << 21, false, 1024, none), DEMC_EUNSUPPORTED, too_many));
    CHECK(!check_hpd_window(true, 0, (1LL << 21) - 1, 1LL << 21, false, 1024, none));
    // the planner is total: what the sort's plan refuses, a bad count, a bad alpha
    CHECK(refused_with(plan_hpd(plan_rank(1LL << 21, 1024, 1), 4, ok, 3).refused, DEMC_EUNSUPPORTED, too_many));
    CHECK(refused_with(plan_hpd(plan_rank(0, 4, 1), 4, ok, 3).refused, DEMC_EINVAL, "bad rows: demc_hpd needs at least one row of the history"));
    CHECK(refused_with(plan_hpd(plan_rank(4, 4, 1), 0, ok, 3).refused, DEMC_EINVAL, "bad rows: demc_hpd needs at least one row of the history"));
    CHECK(refused_with(plan_hpd(plan_rank(4, 4, 1), 4, ok, 0).refused, DEMC_EINVAL, "demc_hpd: n_alphas must be between 1 and 16"));
    CHECK(refused_with(plan_hpd(plan_rank(4, 4, 1), 4, nullptr, 1).refused, DEMC_EINVAL, "demc_hpd: alphas is NULL"));
    CHECK(!plan_hpd(plan_rank((1LL << 31) - 1, 1, 1), 1, ok, 3).refused);
}

void candidates() {
    // alpha = a / 2^k: alpha N is exact in a double while N a stays below 2^53, so m = max(1, ceil(N a / 2^k)) in integers
    const long long sizes[] = {1, 2, 3, 100, 2047, 2048, 2049, (1LL << 31) - 1};
    for (long long N : sizes)
        for (int k : {1, 2, 3, 4, 10, 20, 31})
            for (long long a : {1LL, 3LL, 5LL, (1LL << k) - 1}) {
                if (a >= (1LL << k) || N * a >= (1LL << 53)) continue;  // (beyond 53 bits the product is rounded)
                const double alpha = std::ldexp((double)a, -k);
                const long long want = std::max<long long>(1, (N * a + (1LL << k) - 1) >> k);
                CHECK(hpd_candidates(N, alpha) == want);
                CHECK(want >= 1 && want <= N);
            }
    for (long long N : sizes) {  // the ends of (0, 1): one candidate; every position (N below 2^53: N (1 - 2^-53) is not an integer, except N = 1)
        CHECK(hpd_candidates(N, std::nextafter(0.0, 1.0)) == 1 && hpd_candidates(N, 1e-300) == 1);
        CHECK(hpd_candidates(N, std::nextafter(1.0, 0.0)) == N);
    }
    // rounded products: 0.05 x 100 rounds to 5.0 exactly although 0.05 is above 1 / 20; 0.999 x 2048 = 2045.95...
    CHECK(hpd_candidates(100, 0.05) == 5 && hpd_candidates(2048, 0.999) == 2046 && hpd_candidates(8, 0.999) == 8 && hpd_candidates(8, 1e-9) == 1);
    CHECK(hpd_candidates(2049, 0.5) == 1025 && hpd_candidates(2048, 0.5) == 1024 && hpd_candidates(3, 0.5) == 2);
}

void plans() {
    CHECK(DEMC_HPD_COLS == 4 && DEMC_HPD_MAX_ALPHAS == 16 && kHpdWG == 256 && kHpdWG % 64 == 0 && kHpdFinalWG == 64 && kHpdBytesPerValue == 24);
    const double alphas[4] = {1e-9, 0.05, 0.5, 0.999};
    for (long long n : {1LL, 2LL, 3LL, 7LL, 64LL, 129LL, 256LL, 1000LL, 2051LL, 24577LL})
        for (long long P : {1LL, 3LL, 8LL, 16LL, 24LL, 2048LL})
            for (int series : {1, 3, 4, 16, 17, 34, 66})
                for (int K : {1, 4}) {
                    const RankPlan sort = plan_rank(n, P, 1);
                    const HpdPlan p = plan_hpd(sort, series, alphas, K);
                    CHECK(!p.refused && p.N == n * P && p.n == n && p.P == P && p.series == series);
                    CHECK(p.tiles == sort.tiles && p.blocks == sort.blocks && p.scan_chunk == sort.scan_chunk && p.passes == sort.passes && p.passes == 8);
                    // every series in exactly one batch, none empty, none above the cap; the budget holds whenever more than one is taken
                    CHECK(p.batch >= 1 && p.batch <= kRankMaxBatch && p.batch <= series && p.last_batch >= 1 && p.last_batch <= p.batch);
                    CHECK((p.batches - 1) * p.batch + p.last_batch == series);
                    CHECK(p.bytes_per_series == (size_t)p.N * 24 + (size_t)p.tiles * 1024);
                    CHECK(p.batch == 1 || (size_t)p.batch * p.bytes_per_series <= kRankBudget);
                    CHECK(p.batch == std::min(series, kRankMaxBatch) || (size_t)(p.batch + 1) * p.bytes_per_series > kRankBudget);
                    CHECK(p.batch >= plan_rank(n, P, series).batch);  // the smaller scratch never fits fewer series than the rank call's
                    // the grid of the window kernel
                    const HpdGrid& g = p.grid;
                    CHECK(g.n_alphas == K && g.slots >= 1 && g.slots <= kHpdMaxBlocks);
                    int widest = 1;
                    for (int k = 0; k < DEMC_HPD_MAX_ALPHAS; ++k) {
                        if (k >= K) { CHECK(g.m[k] == 0 && g.wgs[k] == 0); continue; }
                        CHECK(g.m[k] == hpd_candidates(p.N, alphas[k]) && g.m[k] >= 1 && g.m[k] <= p.N);
                        CHECK(g.wgs[k] >= 1 && g.wgs[k] <= kHpdMaxBlocks && ((long long)g.wgs[k] * kHpdWG >= g.m[k] || g.wgs[k] == kHpdMaxBlocks));
                        CHECK((long long)(g.wgs[k] - 1) * kHpdWG < g.m[k]);  // no workgroup without a candidate
                        widest = std::max(widest, g.wgs[k]);
                        if (series != 4 || p.N > 200000) continue;
                        // every candidate in exactly one (workgroup, thread, trip); the upper end stays inside the pool
                        std::vector<unsigned char> seen((size_t)g.m[k], 0);
                        const long long stride = (long long)g.wgs[k] * kHpdWG;
                        for (int x = 0; x < g.wgs[k]; ++x)
                            for (int t = 0; t < kHpdWG; ++t)
                                for (long long i = (long long)x * kHpdWG + t; i < g.m[k]; i += stride) {
                                    CHECK(p.N - g.m[k] + i < p.N && p.N - g.m[k] + i >= i);
                                    ++seen[(size_t)i];
                                }
                        bool once = true;
                        for (unsigned char c : seen) once = once && c == 1;
                        CHECK(once);
                    }
                    CHECK(g.slots == widest);
                    const size_t B = (size_t)p.batch, N = (size_t)p.N;
                    CHECK(p.n_keys == 2 * B * N && p.n_pos == 2 * B * N && p.n_hist == B * 256 * (size_t)p.tiles && p.n_word == 3 * B && p.n_flag == B);
                    CHECK(p.n_part == B * (size_t)K * (size_t)g.slots && p.n_out == (size_t)series * (size_t)K * 4);
                }
    // the stride path starts where one (series, alpha) has more candidates than kHpdMaxBlocks workgroups hold
    const double top[1] = {0.999};
    const long long full = (long long)kHpdMaxBlocks * kHpdWG;
    CHECK(plan_hpd(plan_rank(2050, 8, 1), 4, top, 1).grid.m[0] == full && plan_hpd(plan_rank(2050, 8, 1), 4, top, 1).grid.wgs[0] == kHpdMaxBlocks);
    CHECK(plan_hpd(plan_rank(2051, 8, 1), 4, top, 1).grid.m[0] > full && plan_hpd(plan_rank(2051, 8, 1), 4, top, 1).grid.wgs[0] == kHpdMaxBlocks);
    const double a05[1] = {0.05};
    const HpdPlan big = plan_hpd(plan_rank(1000, 65536, 1), 34, a05, 1);  // 65.5 M values a series: 1.6 GB of pairs, two series side by side
    CHECK(!big.refused && big.batch == 2 && big.batches == 17 && big.tiles == 32000 && big.grid.wgs[0] == kHpdMaxBlocks);
    const HpdPlan mid = plan_hpd(plan_rank(1000, 4096, 1), 34, a05, 1);  // the larger size of DESIGN.md 5.5's table
    CHECK(mid.batch == 16 && mid.batches == 3 && mid.last_batch == 2 && mid.grid.m[0] == 204800);
}

void dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "const") {
            std::printf("const kHpdWG=%d kHpdMaxBlocks=%d kHpdFinalWG=%d kHpdBytesPerValue=%zu DEMC_HPD_COLS=%d DEMC_HPD_MAX_ALPHAS=%d\n", kHpdWG,
                        kHpdMaxBlocks, kHpdFinalWG, kHpdBytesPerValue, DEMC_HPD_COLS, DEMC_HPD_MAX_ALPHAS);
        } else if (what == "H") {
            long long n = 0, P = 0;
            int series = 0;
            in >> n >> P >> series;
            std::vector<double> alphas;
            alphas.reserve(DEMC_HPD_MAX_ALPHAS + 1);  // (so that data() is not null when the request names none)
            std::string hex;
            while (in >> hex) alphas.push_back(std::strtod(hex.c_str(), nullptr));
            const HpdPlan p = plan_hpd(plan_rank(n, P, 1), series, alphas.data(), (int)alphas.size());
            if (p.refused) { std::printf("H refused=%d message=%s\n", p.refused.code, p.refused.message.c_str()); continue; }
            std::printf("H N=%lld tiles=%d blocks=%d batch=%d batches=%d last_batch=%d scan_chunk=%lld passes=%d slots=%d m=", p.N, p.tiles, p.blocks,
                        p.batch, p.batches, p.last_batch, p.scan_chunk, p.passes, p.grid.slots);
            for (int k = 0; k < p.grid.n_alphas; ++k) std::printf("%s%lld", k ? "," : "", p.grid.m[k]);
            std::printf(" wgs=");
            for (int k = 0; k < p.grid.n_alphas; ++k) std::printf("%s%d", k ? "," : "", p.grid.wgs[k]);
            std::printf("\n");
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) { dump(); return 0; }
    refusals();
    candidates();
    plans();
    std::printf("%d checks, %d failures\n", checks, failures);
    if (failures == 0) std::printf("hpdplan ok\n");
    return failures == 0 ? 0 : 1;
}
