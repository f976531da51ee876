// postplan_host.cpp -- csrc/demc_postplan.hpp on the CPU: the history window, the two small history rules and the planners of
// demc_summarize, demc_quantiles and demc_covariance against the project's own statements (the comments of the
// kernel headers) as literal numbers, against brute force written here by other means (searches and counting loops where the
// header divides, exact integer arithmetic where it rounds), and every refusal's code and text held literally.  Built with the
// address and undefined-behaviour sanitizers by tests/test_postplan_host.py; no GPU, no HIP runtime, no ROCm header.
//
// postplan_host --dump reads one request per line from stdin and prints what the header answers, for the Python restatements of
// the same arithmetic that the GPU tests import (tests/test_postplan_host.py):
//   const | L D partner_kind | S n P D max_lag rho_len wants_rho | Q N D ld prob... | C N D col... (no col: cols == NULL, D + 2)
#include "demc_postplan.hpp"

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

long long ceil_div(long long a, long long b) { return a / b + (a % b != 0); }

// ---- the history rules and the window -------------------------------------------------------------------------------------------
void history_rules() {
    CHECK(history_cell_stride(9, DEMC_PARTNER_HISTORY) == 16 && history_cell_stride(17, DEMC_PARTNER_HISTORY) == 32);
    CHECK(history_cell_stride(63, DEMC_PARTNER_HISTORY) == 64 && history_cell_stride(9, DEMC_PARTNER_CURRENT) == 9);
    for (int D = 1; D <= 200; ++D) {
        int want = D;  // the smallest power of two (cells of up to 16) or multiple of 16 (up to 64) that holds D
        if (D <= 16) for (want = 1; want < D; want *= 2) {}
        else if (D <= 64) for (want = 16; want < D; want += 16) {}
        CHECK(history_cell_stride((size_t)D, DEMC_PARTNER_HISTORY) == want);
        CHECK(history_cell_stride((size_t)D, DEMC_PARTNER_CURRENT) == D);
    }
    const size_t budget = (size_t)64 << 20;
    CHECK(history_stage_rows(8, 9) == 116508 && history_stage_rows(4096, 63) == 32 && history_stage_rows(1 << 20, 64) == 1);
    for (size_t P : {1, 3, 8, 24, 4096, 65536, 1 << 22})
        for (size_t D : {1, 2, 9, 17, 31, 63, 64}) {
            const size_t r = history_stage_rows(P, D), row = P * D * 8;
            CHECK(r >= 1 && (r == 1 || r * row <= budget) && (r + 1) * row > budget);
        }
}

void window_checks() {
    const char* rows[3] = {"bad rows: demc_summarize needs at least one row of the history", "bad rows: demc_quantiles needs at least one row of the history",
                           "bad rows: demc_covariance needs at least one row of the history"};
    const char* sharded[3] = {"sharded handle: gather demc_get_history from every rank and summarise on the host",
                              "sharded handle: gather demc_get_history from every rank and take the quantiles on the host",
                              "sharded handle: gather demc_get_history from every rank and take the covariance on the host"};
    const Refusal args{DEMC_EINVAL, "the call's own"};
    for (int c = 0; c < 3; ++c) {
        const PostCall call = (PostCall)c;
        CHECK(!check_history_window(call, true, 0, 1, 1, false) && !check_history_window(call, true, 3, 10, 10, false));
        CHECK(check_history_window(call, true, 0, 1, 1, false).code == DEMC_OK && check_history_window(call, true, 0, 1, 1, false).message.empty());
        // each condition alone ...
        CHECK(refused_with(check_history_window(call, false, 0, 1, 1, false), "history is not stored on this handle"));
        CHECK(refused_with(check_history_window(call, true, -1, 1, 1, false), rows[c]));
        CHECK(refused_with(check_history_window(call, true, 1, 1, 1, false), rows[c]));   // no row
        CHECK(refused_with(check_history_window(call, true, 2, 1, 4, false), rows[c]));   // fewer than none
        CHECK(refused_with(check_history_window(call, true, 0, 5, 4, false), rows[c]));   // past the end
        CHECK(refused_with(check_history_window(call, true, 0, 1, 1, false, args), "the call's own"));
        CHECK(refused_with(check_history_window(call, true, 0, 1, 1, true), sharded[c]));
        // ... and which one wins: no history, the rows, the call's own arguments, the sharded handle
        CHECK(refused_with(check_history_window(call, false, -1, 9, 1, true, args), "history is not stored on this handle"));
        CHECK(refused_with(check_history_window(call, true, -1, 9, 1, true, args), rows[c]));
        CHECK(refused_with(check_history_window(call, true, 0, 1, 1, true, args), "the call's own"));
    }
}

// ---- demc_summarize -------------------------------------------------------------------------------------------------------------
void summary_statements() {
    // DESIGN.md 5.5 and the comments of demc_summary.hpp: the modes on each side of both LDS limits
    const long long ns[4] = {8064, 8065, 18304, 18305};
    const bool lds[4] = {true, true, true, false};
    const size_t bytes[4] = {65536, 8193 * 8, 147456, 1024};
    for (int i = 0; i < 4; ++i) {
        const SummaryPlan s = plan_summary(ns[i], 4, 1, 0, 0, false);
        CHECK(!s.refused && s.lds == lds[i] && s.JT == 1 && s.tiles == 3 && s.lds_bytes == bytes[i] && s.workers == 4);
        CHECK((s.n_xg != 0) == !lds[i]);
    }
    SummaryPlan s = plan_summary(1000, 4096, 32, 0, 0, false);  // JT = 7: tiles of 7, 7, 7, 7, 6 series
    CHECK(s.JT == 7 && s.tiles == 5 && s.workers == 1024 && s.lds && s.lds_bytes == 7 * 1128 * 8 && s.h == 500 && s.L == 499 && s.lag_blocks == 8);
    s = plan_summary(200, 8, 2, 0, 0, false);
    CHECK(s.JT == 4 && s.tiles == 1 && s.workers == 8 && s.lag_blocks == 2);
    s = plan_summary(18305, 64, 6, 0, 0, false);  // a global tile of 8 x 18305 doubles per worker: 57 of them in 64 MiB
    CHECK(!s.lds && s.workers == 57 && s.JT == 1 && s.tiles == 8 && s.n_xg == (size_t)57 * 8 * 18305);
    CHECK(plan_summary(1, 3, 1, 0, 0, false).lag_blocks == 0 && plan_summary(130, 3, 1, 0, 0, false).lag_blocks == 2 && plan_summary(128, 3, 1, 0, 0, false).lag_blocks == 1);
    CHECK(plan_summary(1, 3, 1, 0, 5, true).L == -1 && plan_summary(1, 3, 1, 0, 5, true).rho_cols == 0 && plan_summary(3, 3, 1, 0, 5, true).L == -1);
    CHECK(plan_summary(1000, 16, 2, 64, 70, true).rho_cols == 65 && plan_summary(1000, 16, 2, 64, 70, true).lag_blocks == 2);
    // the refusal: h - 1 lags must fit twice in an int
    const long long hmax = (long long)std::numeric_limits<int>::max() / 2 + 1;
    CHECK(!plan_summary(2 * hmax + 1, 1, 1, 0, 0, false).refused);
    CHECK(refused_with(plan_summary(2 * hmax + 2, 1, 1, 0, 0, false).refused, "demc_summarize: too many rows"));
}

void summary_brute_force() {
    const long long ns[] = {1, 2, 3, 4, 5, 8, 127, 128, 129, 130, 131, 200, 1000, 3900, 3968, 3969, 8064, 8065, 18304, 18305, 20000, 1000000};
    const long long Ps[] = {1, 3, 8, 57, 64, 1023, 1024, 1025, 4096};
    const int Ds[] = {1, 2, 5, 6, 7, 30, 32, 62, 70};
    const int lags[] = {0, 1, 63, 64, 65, 127, 128, 1000000};
    const long long rls[] = {0, 1, 70, 1000};
    for (long long n : ns) for (long long P : Ps) for (int D : Ds) for (int max_lag : lags) for (long long rho_len : rls) for (int wants = 0; wants < 2; ++wants) {
        const SummaryPlan s = plan_summary(n, P, D, max_lag, rho_len, wants != 0);
        const long long D2 = D + 2, h = n / 2;
        CHECK(!s.refused && s.h == h);
        long long L = -1;
        if (h >= 2) L = max_lag > 0 && max_lag < h - 1 ? max_lag : h - 1;
        CHECK(s.L == L);
        int blocks = 0;  // blocks of 64 lags that hold a lag <= L
        for (long long t0 = 0; t0 <= L; t0 += 64) ++blocks;
        CHECK(s.lag_blocks == blocks);
        const long long series_bytes = 8 * (n + 128);  // the rows and two rows of 64 accumulators
        long long JT = 1, workers = P < 1024 ? P : 1024;
        bool lds = true;
        if (series_bytes <= 64 * 1024) { for (JT = 1; JT + 1 <= D2 && JT + 1 <= 8 && (JT + 1) * series_bytes <= 64 * 1024; ++JT) {} }
        else if (series_bytes > 144 * 1024) {
            lds = false;
            while (workers > 1 && workers * n * D2 * 8 > (64LL << 20)) --workers;
        }
        CHECK(s.lds == lds && s.JT == JT && s.workers == workers);
        int tiles = 0;
        for (long long j0 = 0; j0 < D2; j0 += JT) ++tiles;
        CHECK(s.tiles == tiles);
        CHECK(s.lds_bytes == (size_t)(lds ? JT * series_bytes : 1024) && s.lds_bytes <= 144 * 1024);
        long long rho_cols = 0;
        if (wants) { rho_cols = rho_len < L + 1 ? rho_len : L + 1; if (rho_cols < 0) rho_cols = 0; }
        CHECK(s.rho_cols == rho_cols);
        CHECK(s.n_inv == (size_t)(n * P) && s.n_mu == (size_t)(D2 * 2 * P) && s.n_part == (size_t)(workers * D2) && s.n_part_g == (size_t)(workers * D2 * 64));
        CHECK(s.n_small == (size_t)(12 * D2) && s.n_flags == (size_t)(2 * D2) && s.n_xg == (size_t)(lds ? 0 : workers * D2 * n) && s.n_rho == (size_t)(D2 * rho_cols));
    }
}

// ---- demc_quantiles -------------------------------------------------------------------------------------------------------------
const double kDefault[5] = {0.025, 0.25, 0.5, 0.75, 0.975};

void quantile_statements() {
    QuantilePlan q = plan_quantiles(1000LL * 4096, 32, 32, kDefault, 5);
    CHECK(!q.refused && q.cpi == 16 && q.W == 512 && q.chunks == 500 * 512 && q.T == 10 && q.slots[0] == 64 && q.slots[1] == 64 && q.slots[7] == 64);
    CHECK(q.lds_max == 65792 && q.lds_bytes[0] == 65792 && q.n_cells == 340 && q.n_table == 340 * 256 && q.n_series == 34 && q.n_out == 170);
    q = plan_quantiles(1000LL * 24, 2, 2, kDefault, 5);
    CHECK(q.cpi == 256 && q.slots[0] == 4 && q.slots[1] == 64 && q.lds_bytes[0] == 4 * 257 * 4);
    q = plan_quantiles(16 * 8, 62, 62, kDefault, 5);
    CHECK(q.slots[0] == 64 && q.cpi == 8 && q.chunks == 16 && q.W == 16);
    q = plan_quantiles(16, 70, 70, kDefault, 5);  // 72 series: eight find no table in the first pass
    CHECK(q.slots[0] == 64 && q.n_series == 72);
    q = plan_quantiles(64, 9, 16, kDefault, 5);  // padded cells
    CHECK(q.cpi == 32 && q.chunks == 2);
    q = plan_quantiles(10, 600, 600, kDefault, 5);  // cells wider than a workgroup
    CHECK(q.cpi == 1 && q.chunks == 10);
    const double half = 0.5, ends[2] = {0.0, 1.0};
    q = plan_quantiles(4, 1, 1, &half, 1);
    CHECK(q.T == 2 && q.tg.rank[0] == 1 && q.tg.rank[1] == 2 && q.tg.gamma[0] == 0.5 && q.tg.ia[0] == 0 && q.tg.ib[0] == 1);
    q = plan_quantiles(4, 1, 1, ends, 2);
    CHECK(q.T == 4 && q.tg.rank[0] == 0 && q.tg.rank[3] == 3 && q.tg.gamma[0] == 0.0 && q.tg.gamma[1] == 1.0 && q.tg.ia[1] == 2 && q.tg.ib[1] == 3);
    q = plan_quantiles(1, 3, 3, kDefault, 5);  // a pool of one value
    CHECK(!q.refused && q.T == 1 && q.tg.rank[0] == 0 && q.tg.n_probs == 5);
    for (int k = 0; k < 5; ++k) CHECK(q.tg.gamma[k] == 0.0 && q.tg.ia[k] == 0 && q.tg.ib[k] == 0);
    // N = 21, p = 0.9: aleph = 18.900000000000002 + 0.09999999999999998 (the order of the operations is the result)
    const double p9 = 0.9;
    q = plan_quantiles(21, 1, 1, &p9, 1);
    CHECK(q.tg.rank[0] == 18 && q.tg.rank[1] == 19 && q.tg.gamma[0] == (21.0 * 0.9 + (1.0 - 0.9)) - 19.0);
}

void quantile_refusals() {
    double probs[17];
    for (int k = 0; k < 17; ++k) probs[k] = k / 16.0;
    const char* count = "demc_quantiles: n_probs must be in 1 .. 16";
    const char* range = "demc_quantiles: a prob is outside [0, 1]";
    CHECK(refused_with(plan_quantiles(100, 2, 2, probs, 0).refused, count) && refused_with(plan_quantiles(100, 2, 2, probs, -3).refused, count));
    CHECK(refused_with(plan_quantiles(100, 2, 2, probs, 17).refused, count) && !plan_quantiles(100, 2, 2, probs, 16).refused);
    CHECK(refused_with(check_probs(probs, 17), count) && !check_probs(probs, 16) && !check_probs(probs, 1));
    CHECK(plan_quantiles(100, 2, 2, probs, 16).T == 32);
    for (double bad : {-1e-300, 1.0000000000000002, std::nan(""), HUGE_VAL, -HUGE_VAL}) {
        probs[3] = bad;
        CHECK(refused_with(plan_quantiles(100, 2, 2, probs, 4).refused, range) && refused_with(check_probs(probs, 16), range));
        CHECK(!plan_quantiles(100, 2, 2, probs, 3).refused);
        CHECK(refused_with(plan_quantiles(100, 2, 2, probs, 17).refused, count));  // the count is looked at first
    }
    probs[3] = 3 / 16.0;
    // 2^22 chunks a workgroup: cells wider than a workgroup are a chunk each, and 512 workgroups share them
    const char* many = "demc_quantiles: too many rows for the 32-bit counts of a workgroup";
    const long long most = 512LL << 22;
    CHECK(!plan_quantiles(most, 600, 600, probs, 2).refused && refused_with(plan_quantiles(most + 1, 600, 600, probs, 2).refused, many));
    CHECK(!plan_quantiles(most * 16, 32, 32, probs, 2).refused && refused_with(plan_quantiles(most * 16 + 1, 32, 32, probs, 2).refused, many));
    probs[1] = 2.0;
    CHECK(refused_with(plan_quantiles(most + 1, 600, 600, probs, 2).refused, range));  // the arguments before the size
}

void quantile_brute_force() {
    // geometry: chunks, workgroups and the slots of every pass
    const int lds[] = {1, 2, 3, 4, 7, 8, 9, 16, 31, 32, 33, 62, 64, 70, 255, 256, 257, 511, 512, 513, 600, 4096};
    const long long Ns[] = {1, 2, 3, 7, 8, 9, 127, 128, 129, 4095, 4096, 4097, 24000, 131071, 4096000, (1LL << 32) + 5};
    const double probs[16] = {0.0, 1.0, 0.5, 0.25, 0.75, 0.125, 0.375, 0.625, 0.875, 0.0625, 0.1875, 0.3125, 0.4375, 0.5625, 0.6875, 0.8125};
    for (int ld : lds) for (long long N : Ns) for (int n_probs : {1, 2, 3, 5, 8, 16}) for (int D : {1, 2, 6, 30, 62, 63, 70}) {
        if (D > ld) continue;
        const QuantilePlan q = plan_quantiles(N, D, ld, probs, n_probs);
        int cpi = 1;  // the most whole cells whose lanes fit a workgroup
        while ((cpi + 1) * (ld < 512 ? ld : 512) <= 512) ++cpi;
        if (ceil_div(ceil_div(N, cpi), 512) > 1LL << 22) {  // more than 2^22 chunks for a workgroup: its 32-bit counts are refused the risk
            CHECK(refused_with(q.refused, "demc_quantiles: too many rows for the 32-bit counts of a workgroup"));
            continue;
        }
        CHECK(!q.refused);
        CHECK(q.cpi == cpi && q.chunks == ceil_div(N, cpi) && q.W == (q.chunks < 512 ? q.chunks : 512) && q.W >= 1);
        CHECK(ceil_div(q.chunks, q.W) * 512 <= 1LL << 32);
        for (int i = 0; i < 8; ++i) {
            const long long groups = i == 0 ? D + 2 : (long long)(D + 2) * q.T;
            int slots = 64;  // the smallest power of two that holds the groups, 64 at the most
            for (int s = 32; s >= 1; s /= 2) if (s >= groups) slots = s;
            CHECK(q.slots[i] == slots && q.lds_bytes[i] == (size_t)slots * (256 + 1) * 4 && q.lds_bytes[i] <= q.lds_max);
        }
        CHECK(q.lds_max == 64 * 257 * 4);
        CHECK(q.n_cells == (size_t)(D + 2) * q.T && q.n_table == 256 * q.n_cells && q.n_series == (size_t)(D + 2) && q.n_out == (size_t)(D + 2) * n_probs);
        // the targets of dyadic probs a / 16: 16 aleph = N a + 16 - a exactly (N a < 2^53)
        CHECK(q.tg.n_probs == n_probs && q.T >= 1 && q.T <= 2 * n_probs);
        for (int t = 1; t < q.T; ++t) CHECK(q.tg.rank[t - 1] < q.tg.rank[t]);
        bool used[kQMaxTargets] = {};
        for (int k = 0; k < n_probs; ++k) {
            const long long a = (long long)(probs[k] * 16);
            const long long num = N * a + 16 - a;
            long long j = num / 16;
            j = j < 1 ? 1 : j;
            j = j > N - 1 ? N - 1 : j;
            if (N == 1) j = 1;
            double gamma = (double)(num - 16 * j) / 16.0;
            gamma = N == 1 ? 0.0 : gamma < 0.0 ? 0.0 : gamma > 1.0 ? 1.0 : gamma;
            const int ia = q.tg.ia[k], ib = q.tg.ib[k];
            CHECK(ia >= 0 && ia < q.T && ib >= 0 && ib < q.T);
            CHECK(q.tg.rank[ia] == (unsigned long long)(j - 1) && q.tg.rank[ib] == (unsigned long long)(N == 1 ? 0 : j) && q.tg.gamma[k] == gamma);
            used[ia] = used[ib] = true;
        }
        for (int t = 0; t < q.T; ++t) CHECK(used[t]);
    }
}

// ---- demc_covariance ------------------------------------------------------------------------------------------------------------
void cov_statements() {
    int32_t cols[64];
    for (int k = 0; k < 64; ++k) cols[k] = k;
    CovPlan c = plan_cov(1000LL * 4096, 32, nullptr, 34);
    CHECK(!c.refused && c.K == 34 && c.NB == 3 && cov_tiles(c.NB) == 6 && c.chunks == 8000 && c.W == 512 && ceil_div(c.chunks, c.W) == 16);
    CHECK(cov_partial(c.NB) == 1584 && c.n_part2 == 512 * 1584 && c.n_part1 == 512 * 64 && c.n_mean == 34 && c.n_mat == 34 * 34 && c.n_cols == 64 && c.n_mhat == 64);
    CHECK(8 * (c.n_part1 + c.n_mhat + c.n_part2 + c.n_mean + 2 * c.n_mat) + 4 * c.n_cols < (size_t)8 << 20);
    for (int k = 0; k < 64; ++k) CHECK(c.table[k] == (k < 34 ? k : -1));
    c = plan_cov(1000 * 24, 2, nullptr, 4);
    CHECK(c.NB == 1 && c.chunks == 47 && c.W == 47);
    CHECK(plan_cov(12, 600, cols, 64).NB == 4 && cov_tiles(4) == 10 && cov_partial(4) == 2624 && 8 * (cov_partial(4) + 64 * 64) <= 64 * 1024);
    CHECK(kCovChunk % (4 * (kCovWG / 64)) == 0);
}

void cov_refusals() {
    int32_t cols[66];
    for (int k = 0; k < 66; ++k) cols[k] = k;
    const char* count = "demc_covariance: n_cols must be in 1 .. 64";
    const char* all = "demc_covariance: cols == NULL selects all D + 2 series: n_cols must equal D + 2 (at most 64)";
    const char* range = "demc_covariance: a column is outside [0, D + 2)";
    const char* twice = "demc_covariance: a column is repeated";
    CHECK(refused_with(plan_cov(100, 70, cols, 0).refused, count) && refused_with(plan_cov(100, 70, cols, 65).refused, count) && !plan_cov(100, 70, cols, 64).refused);
    CHECK(refused_with(plan_cov(100, 70, nullptr, 65).refused, count));  // the count is looked at first
    CHECK(refused_with(plan_cov(100, 5, nullptr, 6).refused, all) && refused_with(plan_cov(100, 5, nullptr, 8).refused, all) && !plan_cov(100, 5, nullptr, 7).refused);
    CHECK(refused_with(plan_cov(100, 70, nullptr, 64).refused, all));  // (72 series: they cannot all be selected)
    CHECK(!plan_cov(100, 5, cols, 7).refused && refused_with(plan_cov(100, 5, cols, 8).refused, range));
    const int32_t neg[3] = {0, -1, 0}, rep[3] = {2, 2, 99}, last[4] = {6, 0, 3, 6};
    CHECK(refused_with(plan_cov(100, 5, neg, 3).refused, range));   // column 1 is looked at before column 2 repeats column 0
    CHECK(refused_with(plan_cov(100, 5, rep, 3).refused, twice));   // ... and column 1 repeats before column 2 is out of range
    CHECK(refused_with(plan_cov(100, 5, last, 4).refused, twice) && !plan_cov(100, 5, last, 3).refused);
    int table[kCovMaxCols];
    CHECK(refused_with(select_columns(5, rep, 3, table), twice) && !select_columns(5, last, 3, table) && table[0] == 6 && table[2] == 3 && table[3] == -1);
}

void cov_brute_force() {
    const long long Ns[] = {1, 2, 3, 4, 5, 23, 24, 511, 512, 513, 1024, 2049, 24000, 512 * 512 - 1, 512 * 512, 512 * 512 + 1, 4096000, (1LL << 33) + 1};
    for (long long N : Ns) for (int D : {1, 2, 9, 14, 15, 30, 62, 600}) for (int K = 1; K <= 64 && K <= D + 2; ++K) for (int given = 0; given < 2; ++given) {
        int32_t cols[64];
        for (int k = 0; k < K; ++k) cols[k] = (int32_t)((k * 67 + 3) % K + (D + 2 - K));  // a permutation of the last K series
        if (!given && K != D + 2) continue;
        const CovPlan c = plan_cov(N, D, given ? cols : nullptr, K);
        CHECK(!c.refused && c.K == K);
        for (int k = 0; k < 64; ++k) CHECK(c.table[k] == (k >= K ? -1 : given ? cols[k] : k));
        int nb = 0;  // blocks of 16 columns that hold a column
        for (int k0 = 0; k0 < K; k0 += 16) ++nb;
        int tiles = 0;
        for (int bi = 0; bi < nb; ++bi) for (int bj = bi; bj < nb; ++bj) ++tiles;
        CHECK(c.NB == nb && cov_tiles(c.NB) == tiles && cov_partial(c.NB) == tiles * 16 * 16 + nb * 16);
        CHECK(c.chunks == ceil_div(N, 512) && c.W == (c.chunks < 512 ? c.chunks : 512) && c.W >= 1);
        CHECK(c.n_cols == 64 && c.n_part1 == (size_t)c.W * 64 && c.n_mhat == 64 && c.n_part2 == (size_t)c.W * (tiles * 256 + nb * 16));
        CHECK(c.n_mean == (size_t)K && c.n_mat == (size_t)K * K);
    }
}

// ---- --dump -----------------------------------------------------------------------------------------------------------------------
bool dump_refusal(char kind, const Refusal& r) {
    if (r) std::printf("%c refused=%d message=%s\n", kind, r.code, r.message.c_str());
    return (bool)r;
}

int dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "const") {
            std::printf("const kSumLagBlock=%d kSumWG=%d kSumMaxJT=%d kSumMaxWorkers=%d kSumLdsSmall=%zu kSumLdsMax=%zu kSumGlobalTile=%zu", kSumLagBlock, kSumWG,
                        kSumMaxJT, kSumMaxWorkers, kSumLdsSmall, kSumLdsMax, kSumGlobalTile);
            std::printf(" kQBits=%d kQWG=%d kQMaxWG=%d kQSlots=%d kQProbes=%d kQMaxTargets=%d kQMaxChunksPerWG=%lld kQPasses=%d kQKeyNegInf=%llu kQKeyPosInf=%llu",
                        kQBits, kQWG, kQMaxWG, kQSlots, kQProbes, kQMaxTargets, kQMaxChunksPerWG, kQPasses, kQKeyNegInf, kQKeyPosInf);
            std::printf(" kCovMaxCols=%d kCovWG=%d kCovChunk=%d kCovMaxWorkers=%d kCovFinalWG=%d DEMC_QUANTILE_MAX_PROBS=%d DEMC_COV_MAX_COLS=%d\n", kCovMaxCols, kCovWG,
                        kCovChunk, kCovMaxWorkers, kCovFinalWG, DEMC_QUANTILE_MAX_PROBS, DEMC_COV_MAX_COLS);
        } else if (kind == "L") {
            long long D; int partner;
            if (!(in >> D >> partner)) return 2;
            std::printf("L ld=%d\n", history_cell_stride((size_t)D, partner));
        } else if (kind == "S") {
            long long n, P, rho_len; int D, max_lag, wants;
            if (!(in >> n >> P >> D >> max_lag >> rho_len >> wants)) return 2;
            const SummaryPlan s = plan_summary(n, P, D, max_lag, rho_len, wants != 0);
            if (dump_refusal('S', s.refused)) continue;
            std::printf("S refused=0 h=%lld L=%d lag_blocks=%d lds=%d JT=%d tiles=%d workers=%d lds_bytes=%zu rho_cols=%lld n_inv=%zu n_mu=%zu n_part=%zu n_part_g=%zu "
                        "n_small=%zu n_flags=%zu n_xg=%zu n_rho=%zu\n", s.h, s.L, s.lag_blocks, (int)s.lds, s.JT, s.tiles, s.workers, s.lds_bytes, s.rho_cols, s.n_inv,
                        s.n_mu, s.n_part, s.n_part_g, s.n_small, s.n_flags, s.n_xg, s.n_rho);
        } else if (kind == "Q") {
            long long N; int D, ld;
            if (!(in >> N >> D >> ld)) return 2;
            std::vector<double> probs;
            for (std::string w; in >> w;) probs.push_back(std::strtod(w.c_str(), nullptr));  // (hexadecimal floats: exact)
            const QuantilePlan q = plan_quantiles(N, D, ld, probs.data(), (int)probs.size());
            if (dump_refusal('Q', q.refused)) continue;
            std::printf("Q refused=0 T=%d cpi=%d chunks=%lld W=%d lds_max=%zu n_cells=%zu n_table=%zu n_series=%zu n_out=%zu slots=", q.T, q.cpi, q.chunks, q.W, q.lds_max,
                        q.n_cells, q.n_table, q.n_series, q.n_out);
            for (int i = 0; i < kQPasses; ++i) std::printf("%s%d", i ? "," : "", q.slots[i]);
            std::printf(" lds_bytes=");
            for (int i = 0; i < kQPasses; ++i) std::printf("%s%zu", i ? "," : "", q.lds_bytes[i]);
            std::printf(" rank=");
            for (int t = 0; t < q.T; ++t) std::printf("%s%llu", t ? "," : "", q.tg.rank[t]);
            std::printf(" gamma=");
            for (int k = 0; k < q.tg.n_probs; ++k) std::printf("%s%a", k ? "," : "", q.tg.gamma[k]);
            std::printf(" ia=");
            for (int k = 0; k < q.tg.n_probs; ++k) std::printf("%s%d", k ? "," : "", q.tg.ia[k]);
            std::printf(" ib=");
            for (int k = 0; k < q.tg.n_probs; ++k) std::printf("%s%d", k ? "," : "", q.tg.ib[k]);
            std::printf("\n");
        } else if (kind == "C") {
            long long N; int D;
            if (!(in >> N >> D)) return 2;
            std::vector<int32_t> cols;
            for (int v; in >> v;) cols.push_back(v);
            const CovPlan c = cols.empty() ? plan_cov(N, D, nullptr, D + 2) : plan_cov(N, D, cols.data(), (int)cols.size());
            if (dump_refusal('C', c.refused)) continue;
            std::printf("C refused=0 K=%d NB=%d tiles=%d partial=%d chunks=%lld W=%d n_cols=%zu n_part1=%zu n_mhat=%zu n_part2=%zu n_mean=%zu n_mat=%zu table=", c.K, c.NB,
                        cov_tiles(c.NB), cov_partial(c.NB), c.chunks, c.W, c.n_cols, c.n_part1, c.n_mhat, c.n_part2, c.n_mean, c.n_mat);
            for (int k = 0; k < kCovMaxCols; ++k) std::printf("%s%d", k ? "," : "", c.table[k]);
            std::printf("\n");
        } else
            return 2;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) return dump();
    history_rules();
    window_checks();
    summary_statements();
    summary_brute_force();
    quantile_statements();
    quantile_refusals();
    quantile_brute_force();
    cov_statements();
    cov_refusals();
    cov_brute_force();
    if (failures) std::fprintf(stderr, "%d of %d checks failed\n", failures, checks);
    else std::printf("postplan ok: %d checks\n", checks);
    return failures ? 1 : 0;
}
