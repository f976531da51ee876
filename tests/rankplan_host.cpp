// rankplan_host.cpp -- csrc/demc_rankplan.hpp and csrc/demc_ppnd.hpp on the CPU: every refusal of demc_rankstats and
// demc_rank_series with its code and text held literally, the planner against brute force written here by other means (every pool
// position in exactly one tile, every (digit, tile) count in exactly one thread's chunk, every series in exactly one batch, the
// batch within the budget), the three quantile targets against integers, and the edge values of ppnd16.  Built with the address
// and undefined-behaviour sanitizers by tests/test_rank_host.py, with -ffp-contract=off as the library is; no GPU, no HIP runtime,
// no ROCm header.
//
// rankplan_host --dump reads one request per line from stdin and prints what the headers answer, for the Python restatements of
// the same arithmetic (tests/test_rank_host.py: geometry(), and the accuracy test of the inverse normal):
//   const | P n P series | Z p (a C99 hex float: prints ppnd16(p) the same way)
#include "demc_ppnd.hpp"
#include "demc_rankplan.hpp"

#include <cmath>
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

bool refused_with(const Refusal& r, int code, const std::string& text) { return r.code == code && r.message == text; }

void refusals() {
    const Refusal none;
    CHECK(!rank_args(true, 0, false, -1, -1, 3) && !rank_args(true, 7, true, 4, 2, 3) && !rank_args(true, 0, true, 0, 0, 3));
    CHECK(refused_with(rank_args(false, 0, false, -1, -1, 3), DEMC_EINVAL, "demc_rankstats: out is NULL"));
    CHECK(refused_with(rank_args(true, -1, false, -1, -1, 3), DEMC_EINVAL, "demc_rankstats: max_lag is negative"));
    CHECK(refused_with(rank_args(true, 0, true, 5, 0, 3), DEMC_EINVAL, "demc_rank_series: series is outside [0, D + 2)"));
    CHECK(refused_with(rank_args(true, 0, true, -1, 0, 3), DEMC_EINVAL, "demc_rank_series: series is outside [0, D + 2)"));
    CHECK(refused_with(rank_args(true, 0, true, 0, 3, 3), DEMC_EINVAL, "demc_rank_series: kind must be 0 (ranks), 1 (normal scores) or 2 (ranks of |x - med|)"));
    CHECK(refused_with(rank_args(true, 0, true, 0, -1, 3), DEMC_EINVAL, "demc_rank_series: kind must be 0 (ranks), 1 (normal scores) or 2 (ranks of |x - med|)"));
    // the window, in the order of the other posterior-statistics calls: history, rows, arguments, sharded, then the cap
    const Refusal arg = rank_args(false, 0, false, -1, -1, 3);
    CHECK(refused_with(check_rank_window(false, -1, 0, 10, true, 8, arg), DEMC_EINVAL, "demc_rankstats: history is not stored on this handle"));
    for (auto rows : {std::pair<long long, long long>{-1, 5}, {0, 11}, {5, 5}, {6, 5}})
        CHECK(refused_with(check_rank_window(true, rows.first, rows.second, 10, true, 8, arg), DEMC_EINVAL,
                           "bad rows: demc_rankstats needs at least one row of the history"));
    CHECK(refused_with(check_rank_window(true, 0, 10, 10, true, 8, arg), DEMC_EINVAL, "demc_rankstats: out is NULL"));
    CHECK(refused_with(check_rank_window(true, 0, 10, 10, true, 8, none), DEMC_EINVAL,
                       "sharded handle: gather demc_get_history from every rank and rank the pool on the host"));
    CHECK(!check_rank_window(true, 0, 10, 10, false, 8, none) && !check_rank_window(true, 9, 10, 10, false, 1, none));
    const char* many = "demc_rankstats: N = n P is 2^31 or more, positions in the pool are 32-bit; pass a narrower window";
    CHECK(refused_with(check_rank_window(true, 0, 1LL << 21, 1LL << 21, false, 1024, none), DEMC_EUNSUPPORTED, many));
    CHECK(!check_rank_window(true, 0, (1LL << 21) - 1, 1LL << 21, false, 1024, none));
    CHECK(refused_with(plan_rank(1LL << 21, 1024, 3).refused, DEMC_EUNSUPPORTED, many));
    CHECK(!plan_rank((1LL << 31) - 1, 1, 1).refused && plan_rank((1LL << 31) - 1, 1, 1).N == kRankMaxN);
    CHECK(refused_with(plan_rank(1LL << 31, 1, 1).refused, DEMC_EUNSUPPORTED, many));
    CHECK(plan_rank(0, 4, 3).refused.code == DEMC_EINVAL && plan_rank(4, 0, 3).refused.code == DEMC_EINVAL && plan_rank(4, 4, 0).refused.code == DEMC_EINVAL);
}

void targets() {
    // N p + (1 - p) in integers for the three probs: p = a / 20 -> (N a + 20 - a) / 20
    const int num[3] = {10, 1, 19};
    for (long long N : {1LL, 2LL, 3LL, 4LL, 7LL, 19LL, 20LL, 21LL, 39LL, 40LL, 41LL, 1000LL, 12288LL, 196608LL}) {
        const RankTargets t = rank_targets(N);
        for (int k = 0; k < 3; ++k) {
            if (N == 1) { CHECK(t.j[k] == 1 && t.gamma[k] == 0.0); continue; }
            const long long top = N * num[k] + 20 - num[k];
            long long j = std::max<long long>(1, std::min<long long>(top / 20, N - 1));
            // the rounded product may sit one ulp beside the exact one; trunc can then differ only where top is a multiple of 20
            CHECK(t.j[k] == j || (top % 20 == 0 && t.j[k] == j - 1) );
            CHECK(t.gamma[k] >= 0.0 && t.gamma[k] <= 1.0 && t.j[k] >= 1 && t.j[k] <= N - 1);
            CHECK(std::fabs((double)t.j[k] + t.gamma[k] - (double)top / 20.0) <= 1e-9 * (double)N || t.gamma[k] == 0.0 || t.gamma[k] == 1.0);
        }
    }
    const RankTargets t4 = rank_targets(4);  // med of four values: between x_(2) and x_(3), half way
    CHECK(t4.j[0] == 2 && t4.gamma[0] == 0.5);
}

void plans() {
    CHECK(DEMC_RANK_COLS == 8 && kRankPasses == 8 && kRankTile % kRankWave == 0 && kRankBytesPerValue == 64);
    for (long long n : {1LL, 2LL, 3LL, 7LL, 64LL, 129LL, 256LL, 1000LL, 24577LL})
        for (long long P : {1LL, 3LL, 8LL, 16LL, 24LL, 2048LL})
            for (int series : {1, 3, 4, 16, 17, 34, 66}) {
                const RankPlan p = plan_rank(n, P, series);
                CHECK(!p.refused && p.N == n * P && p.series == series);
                // every position in exactly one tile; the last tile is not empty
                CHECK((long long)p.tiles * kRankTile >= p.N && (long long)(p.tiles - 1) * kRankTile < p.N);
                // every (digit, tile) count in exactly one chunk
                const long long entries = 256LL * p.tiles;
                CHECK(p.scan_chunk * kRankScanWG >= entries && (p.scan_chunk - 1) * kRankScanWG < entries);
                CHECK(p.blocks >= 1 && p.blocks <= kRankMaxBlocks && ((long long)p.blocks * kRankWG >= p.N || p.blocks == kRankMaxBlocks));
                // every series in exactly one batch, none empty, none above the cap; the budget holds whenever more than one is taken
                CHECK(p.batch >= 1 && p.batch <= kRankMaxBatch && p.batch <= series && p.last_batch >= 1 && p.last_batch <= p.batch);
                CHECK((p.batches - 1) * p.batch + p.last_batch == series);
                CHECK(p.batch == 1 || (size_t)p.batch * p.bytes_per_series <= kRankBudget);
                CHECK(p.batch == std::min(series, kRankMaxBatch) || (size_t)(p.batch + 1) * p.bytes_per_series > kRankBudget);
                const size_t B = (size_t)p.batch, N = (size_t)p.N;
                CHECK(p.n_keys == 2 * B * N && p.n_pos == 2 * B * N && p.n_rk == B * N && p.n_der == 4 * B * N && p.n_hist == B * 256 * (size_t)p.tiles);
                CHECK(p.n_zero == N && p.n_word == 6 * B && p.n_flag == 2 * B && p.n_q == 3 * B && p.n_out == (size_t)series * 8);
            }
    const RankPlan big = plan_rank(1000, 65536, 34);  // 65.5 M values a series: one series is 4.2 GB, above the budget, and still runs
    CHECK(!big.refused && big.batch == 1 && big.batches == 34 && big.tiles == 32000);
    const RankPlan mid = plan_rank(1000, 4096, 34);  // the larger size of DESIGN.md 5.5's table: 16 series side by side, three batches
    CHECK(mid.batch == 16 && mid.batches == 3 && mid.last_batch == 2 && mid.tiles == 2000);
}

void scores() {
    CHECK(ppnd16(0.5) == 0.0 && ppnd16(0.0) == -HUGE_VAL && ppnd16(1.0) == HUGE_VAL);
    CHECK(std::isnan(ppnd16(-0.25)) && std::isnan(ppnd16(1.5)) && std::isnan(ppnd16(std::nan(""))) && std::isnan(ppnd16(HUGE_VAL)));
    CHECK(std::fabs(ppnd16(0.975) - 1.959963984540054) <= 1e-15 && std::fabs(ppnd16(0.025) + 1.959963984540054) <= 1e-15);
    CHECK(std::fabs(ppnd16(0.001) + 3.090232306167813) <= 4e-15 && std::fabs(ppnd16(1e-20) + 9.262340089798408) <= 2e-14);
    CHECK(ppnd16(0.075) == -ppnd16(0.925) || std::fabs(ppnd16(0.075) + ppnd16(0.925)) <= 1e-15);  // (1 - 0.925 is not 0.075 to the bit)
    for (double p = 0.001; p < 0.5; p += 0.001) CHECK(ppnd16(p) < ppnd16(p + 0.001) && ppnd16(p) < 0.0);
    CHECK(ppnd16((1.0 - 0.375) / (1.0 + 0.25)) == 0.0);  // N = 1: r = 1, z = 0
}

void dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "const") {
            std::printf("const kRankBits=%d kRankPasses=%d kRankWave=%d kRankTile=%d kRankScanWG=%d kRankWG=%d kRankMaxBlocks=%d kRankMaxBatch=%d "
                        "kRankDerived=%d kRankBudget=%zu kRankMaxN=%lld kRankBytesPerValue=%zu DEMC_RANK_COLS=%d\n",
                        kRankBits, kRankPasses, kRankWave, kRankTile, kRankScanWG, kRankWG, kRankMaxBlocks, kRankMaxBatch, kRankDerived, kRankBudget,
                        kRankMaxN, kRankBytesPerValue, DEMC_RANK_COLS);
        } else if (what == "P") {
            long long n = 0, P = 0;
            int series = 0;
            in >> n >> P >> series;
            const RankPlan p = plan_rank(n, P, series);
            if (p.refused) { std::printf("P refused=%d message=%s\n", p.refused.code, p.refused.message.c_str()); continue; }
            std::printf("P N=%lld tiles=%d blocks=%d batch=%d batches=%d last_batch=%d scan_chunk=%lld passes=%d j=%lld,%lld,%lld gamma=%a,%a,%a\n", p.N,
                        p.tiles, p.blocks, p.batch, p.batches, p.last_batch, p.scan_chunk, p.passes, p.tg.j[0], p.tg.j[1], p.tg.j[2], p.tg.gamma[0],
                        p.tg.gamma[1], p.tg.gamma[2]);
        } else if (what == "Z") {
            std::string hex;
            in >> hex;
            std::printf("Z z=%a\n", ppnd16(std::strtod(hex.c_str(), nullptr)));
        }
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) { dump(); return 0; }
    refusals();
    targets();
    plans();
    scores();
    std::printf("%d checks, %d failures\n", checks, failures);
    if (failures == 0) std::printf("rankplan ok\n");
    return failures == 0 ? 0 : 1;
}
