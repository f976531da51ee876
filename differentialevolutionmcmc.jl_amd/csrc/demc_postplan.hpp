// demc_postplan.hpp -- everything the three posterior-statistics calls (demc_summarize, demc_quantiles, demc_covariance) decide
// before they touch the device: the constants of their kernels, the record of the history window they read, the checks they share,
// and one planner each that turns plain sizes into lag blocks, tiles, chunks, workers, LDS bytes, target ranks, the column table
// and the scratch element counts.  Pure functions of plain values, host only: plain C++17, no device header, no handle, no call
// into the runtime; pointers are carried, never dereferenced (the caller's probs and cols are host arrays).  The kernel headers
// include this file for the constants; the *_run functions do what a plan says.  tests/postplan_host.cpp runs all of it on the CPU
// under the sanitizers.
//
// Plans are stack records and nothing here allocates; a refusal's text becomes a message only where one occurs.  The order of the
// floating-point operations in plan_quantiles is part of the results.
#pragma once
#include "../../include/demc.h"
#include "../../include/demc_cov.h"       // DEMC_COV_MAX_COLS
#include "../../include/demc_quantile.h"  // DEMC_QUANTILE_MAX_PROBS

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>

#include "demc_hostbase.hpp"  // Refusal, pow2_ceil

namespace demc {

// ---- the constants of the kernels ---------------------------------------------------------------------------------------------

constexpr int kSumLagBlock = 64;        // lags per pass = lanes of a wave (pairs never straddle a block)
constexpr int kSumWG = 256;             // threads of the gathering kernels
constexpr int kSumMaxJT = 8;            // series per tile: two per wave of the moments kernel
constexpr int kSumMaxWorkers = 1024;    // chain workers: bounds partial[worker][D+2][64] (17.8 MB at D + 2 = 34)
constexpr size_t kSumLdsSmall = 64 * 1024;   // preferred LDS per workgroup (two workgroups per CU)
constexpr size_t kSumLdsMax = 144 * 1024;    // ... and the most one asks for: a single series of up to kSumLdsRows rows
constexpr size_t kSumGlobalTile = (size_t)64 << 20;  // budget of the global staging tiles of series too long for LDS

constexpr int kQBits = 8;                 // bits per digit: 256 bins, 8 passes
constexpr int kQWG = 512;                 // threads of k_q_hist
constexpr int kQMaxWG = 512;              // workgroups of k_q_hist: two per CU, all resident
constexpr int kQSlots = 64;               // LDS tables of 256 32-bit counts (64 KiB); a launch uses a power of two of them
constexpr int kQProbes = 4;               // slots a group looks at before it counts in the global table
constexpr int kQMaxTargets = 32;          // two ranks per prob (DEMC_QUANTILE_MAX_PROBS = 16)
constexpr long long kQMaxChunksPerWG = 1LL << 22;  // * kQWG values < 2^32: the 32-bit counts cannot wrap
constexpr int kQPasses = 64 / kQBits;
constexpr unsigned long long kQKeyNegInf = 0x000FFFFFFFFFFFFFull;  // k(-inf): keys below are NaNs with the sign set
constexpr unsigned long long kQKeyPosInf = 0xFFF0000000000000ull;  // k(+inf): keys above are NaNs without it

constexpr int kCovMaxCols = 64;       // DEMC_COV_MAX_COLS: four blocks of 16 columns
constexpr int kCovWG = 512;           // threads of k_cov_mean and k_cov_syrk: 8 waves
constexpr int kCovChunk = 512;        // cells of a chunk: 128 k-steps, 16 per wave
constexpr int kCovMaxWorkers = 512;   // workgroups of a pass: two per CU
constexpr int kCovFinalWG = 1024;     // threads of k_cov_final

constexpr int cov_tiles(int nb) { return nb * (nb + 1) / 2; }
constexpr int cov_partial(int nb) { return cov_tiles(nb) * 256 + nb * 16; }  // doubles a worker writes in pass 2

static_assert(kQMaxTargets == 2 * DEMC_QUANTILE_MAX_PROBS && kCovMaxCols == DEMC_COV_MAX_COLS, "the public caps are the kernels' caps");

struct QTargets {  // by value to k_q_init and k_q_final
    unsigned long long rank[kQMaxTargets];  // 0-based, ascending, distinct
    double gamma[kQMaxTargets / 2];
    int ia[kQMaxTargets / 2], ib[kQMaxTargets / 2];  // targets of x_(j) and x_(j+1) of a prob; ia == ib: the pool has one value
    int n_probs;
};

// ---- the history and its window -----------------------------------------------------------------------------------------------

struct HistView {  // rows [row0, row1) of the slot-keyed history, as all three calls read it
    const double* hist;          // [n_rows][P][ld]
    const unsigned char* acc;    // [n_rows][P]
    const double* lp;            // [n_rows][P]
    const int* idh;              // [n_rows][P]
    long long P, row0, row1, id0;
    int D, ld;
};

// History cells that partners are GATHERED from (DE-MC_Z: `resample`, crossover.jl:113-124) are padded to whole cache lines --
// rows of up to 16 scalars to the next power of two, up to 64 to the next multiple of 16 doubles: a cell of 31 doubles at an
// 8-byte boundary touches 2.9 lines of 128 bytes on average (376 B fetched for 248), at a 256-byte boundary exactly two.  Only
// then: a history that is only written (partners from the population) stays dense -- padded cells would be partial-line stores.
inline int history_cell_stride(size_t D, int partner_kind) {
    if (partner_kind == DEMC_PARTNER_HISTORY && D <= 64) return D <= 16 ? pow2_ceil((int)D) : (int)((D + 15) & ~(size_t)15);
    return (int)D;
}

// rows of a padded history that go through the dense device staging buffer at a time: 64 MiB of them, at least one
inline size_t history_stage_rows(size_t P, size_t D) { return std::max<size_t>(1, ((size_t)64 << 20) / (P * D * sizeof(double))); }

constexpr const char* kHistoryNotStored = "history is not stored on this handle";

enum PostCall { POST_SUMMARIZE, POST_QUANTILES, POST_COVARIANCE };
struct WindowTexts { const char *rows, *sharded; };
constexpr WindowTexts kWindowTexts[3] = {
    {"bad rows: demc_summarize needs at least one row of the history", "sharded handle: gather demc_get_history from every rank and summarise on the host"},
    {"bad rows: demc_quantiles needs at least one row of the history", "sharded handle: gather demc_get_history from every rank and take the quantiles on the host"},
    {"bad rows: demc_covariance needs at least one row of the history", "sharded handle: gather demc_get_history from every rank and take the covariance on the host"}};

// The checks the three calls share, in the order they refuse: no history, a bad row window, `args` -- what the call has against
// its own arguments (check_probs, select_columns; demc_summarize has nothing) --, a sharded handle.
inline Refusal check_history_window(PostCall call, bool stored, long long row0, long long row1, long long n_rows, bool sharded,
                                    Refusal args = Refusal()) {
    if (!stored) return Refusal{DEMC_EINVAL, kHistoryNotStored};
    if (row0 < 0 || row1 - row0 < 1 || row1 > n_rows) return Refusal{DEMC_EINVAL, kWindowTexts[call].rows};
    if (args) return args;
    if (sharded) return Refusal{DEMC_EINVAL, kWindowTexts[call].sharded};
    return Refusal();
}

// ---- demc_summarize (demc_summary.hpp) ------------------------------------------------------------------------------------------

struct SummaryPlan {
    Refusal refused;
    long long h = 0;          // rows of a half chain
    int L = -1;               // the last lag that may be evaluated (-1: none, h < 2)
    int lag_blocks = 0;       // passes of kSumLagBlock lags
    bool lds = true;          // a chain's rows are staged in LDS (false: in a global tile of the worker)
    int JT = 1, tiles = 0;    // series per tile, series tiles
    int workers = 0;
    size_t lds_bytes = 0;     // of the gathering kernels
    long long rho_cols = 0;   // autocorrelations kept per series (0: none asked for)
    // elements of the scratch buffers: inv (int), mu, part (part_sum and part_ss each), part_g, small (mean | bh | W | vplus |
    // p_prev | p_sum | out[6]), flags (K | stopped, int), xg (global mode only), rho
    size_t n_inv = 0, n_mu = 0, n_part = 0, n_part_g = 0, n_small = 0, n_flags = 0, n_xg = 0, n_rho = 0;
};

// n rows of P chains, D parameters; max_lag = 0: no lag cap.  As many series per tile as kSumLdsSmall holds (<= kSumMaxJT), one
// series while it fits in kSumLdsMax, a global tile per (worker, series) beyond that.
inline SummaryPlan plan_summary(long long n, long long P, int D, int max_lag, long long rho_len, bool wants_rho) {
    SummaryPlan s;
    const int D2 = D + 2;
    const long long h = s.h = n / 2;
    if (h - 1 > (long long)std::numeric_limits<int>::max() / 2) { s.refused = Refusal{DEMC_EINVAL, "demc_summarize: too many rows"}; return s; }
    s.L = h >= 2 ? (int)(max_lag > 0 ? std::min<long long>(h - 1, max_lag) : h - 1) : -1;
    s.lag_blocks = h >= 2 ? s.L / kSumLagBlock + 1 : 0;
    const size_t per_series = ((size_t)n + 2 * kSumLagBlock) * sizeof(double);
    s.workers = (int)std::min<long long>(P, kSumMaxWorkers);
    if (per_series <= kSumLdsSmall) s.JT = (int)std::min<size_t>(std::min(D2, kSumMaxJT), kSumLdsSmall / per_series);
    else if (per_series > kSumLdsMax) {
        s.lds = false;
        s.workers = (int)std::max<size_t>(1, std::min<size_t>((size_t)s.workers, kSumGlobalTile / ((size_t)n * D2 * sizeof(double))));
    }
    s.tiles = (D2 + s.JT - 1) / s.JT;
    s.lds_bytes = s.lds ? (size_t)s.JT * per_series : (size_t)2 * kSumLagBlock * sizeof(double);
    s.rho_cols = wants_rho ? std::max<long long>(0, std::min<long long>(rho_len, (long long)s.L + 1)) : 0;
    s.n_inv = (size_t)n * P; s.n_mu = (size_t)D2 * 2 * P; s.n_part = (size_t)s.workers * D2; s.n_part_g = s.n_part * kSumLagBlock;
    s.n_small = (size_t)D2 * 12; s.n_flags = (size_t)D2 * 2; s.n_xg = s.lds ? 0 : s.n_part * n; s.n_rho = (size_t)D2 * s.rho_cols;
    return s;
}

// ---- demc_quantiles (demc_quantile.hpp) -----------------------------------------------------------------------------------------

inline Refusal check_probs(const double* probs, int n_probs) {
    if (n_probs < 1 || n_probs > DEMC_QUANTILE_MAX_PROBS) return Refusal{DEMC_EINVAL, "demc_quantiles: n_probs must be in 1 .. 16"};
    for (int k = 0; k < n_probs; ++k)
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return Refusal{DEMC_EINVAL, "demc_quantiles: a prob is outside [0, 1]"};
    return Refusal();
}

struct QuantilePlan {
    Refusal refused;
    QTargets tg{};
    int T = 0;                // distinct ranks (<= kQMaxTargets)
    int cpi = 0;              // cells of a chunk
    long long chunks = 0;
    int W = 0;                // workgroups of k_q_hist: workgroup b takes the chunks b, b + W, ...
    int slots[kQPasses] = {}; // LDS tables of each pass: the power of two that holds the groups there can be, up to kQSlots
    size_t lds_bytes[kQPasses] = {}, lds_max = 0;  // tables and owner words
    // elements of the scratch buffers: cells (gprefix, trank, tgrp each), table, series (ng and nanflag each), out
    size_t n_cells = 0, n_table = 0, n_series = 0, n_out = 0;
};

// A pool of N values per series, D parameters in cells ld doubles apart.  The targets: aleph = N p + (1 - p) as a
// rounded product and a rounded sum, j = clamp(trunc(aleph), 1, N - 1); x_(j) has the 0-based rank j - 1.
inline QuantilePlan plan_quantiles(long long N, int D, int ld, const double* probs, int n_probs) {
    QuantilePlan q;
    if ((q.refused = check_probs(probs, n_probs))) return q;
    const int D2 = D + 2;
    QTargets& tg = q.tg;
    tg.n_probs = n_probs;
    unsigned long long ranks[kQMaxTargets];
    long long js[kQMaxTargets / 2];
    int nr = 0;
    for (int k = 0; k < n_probs; ++k) {
        const double p = probs[k];
        const double prod = (double)N * p;
        const double aleph = prod + (1.0 - p);
        long long j = (long long)std::trunc(aleph);
        j = std::max<long long>(1, std::min<long long>(j, N - 1));
        if (N == 1) j = 1;
        tg.gamma[k] = N == 1 ? 0.0 : std::min(1.0, std::max(0.0, aleph - (double)j));
        js[k] = j;
        ranks[nr++] = (unsigned long long)(j - 1);
        if (N > 1) ranks[nr++] = (unsigned long long)j;
    }
    std::sort(ranks, ranks + nr);
    unsigned long long* const end = std::unique(ranks, ranks + nr);
    const int T = q.T = (int)(end - ranks);
    for (int t = 0; t < T; ++t) tg.rank[t] = ranks[t];
    for (int k = 0; k < n_probs; ++k) {
        tg.ia[k] = (int)(std::lower_bound(ranks, end, (unsigned long long)(js[k] - 1)) - ranks);
        tg.ib[k] = N == 1 ? tg.ia[k] : (int)(std::lower_bound(ranks, end, (unsigned long long)js[k]) - ranks);
    }
    // geometry (demc_quantile.hpp): a chunk is cpi whole cells, a workgroup takes every W-th chunk
    q.cpi = kQWG / std::min(ld, kQWG);
    q.chunks = (N + q.cpi - 1) / q.cpi;
    q.W = (int)std::min<long long>(q.chunks, kQMaxWG);
    if ((q.chunks + q.W - 1) / q.W > kQMaxChunksPerWG) {
        q.refused = Refusal{DEMC_EINVAL, "demc_quantiles: too many rows for the 32-bit counts of a workgroup"};
        return q;
    }
    for (int i = 0; i < kQPasses; ++i) {  // the first pass has one group per series
        int slots = 1;
        while (slots < kQSlots && slots < (i == 0 ? (long long)D2 : (long long)D2 * T)) slots *= 2;
        q.slots[i] = slots;
        q.lds_bytes[i] = (size_t)slots * 257 * sizeof(unsigned int);
    }
    q.lds_max = (size_t)kQSlots * 257 * sizeof(unsigned int);
    q.n_cells = (size_t)D2 * T; q.n_table = q.n_cells * 256; q.n_series = (size_t)D2; q.n_out = (size_t)D2 * n_probs;
    return q;
}

// ---- demc_covariance (demc_cov.hpp) -----------------------------------------------------------------------------------------------

// table[kCovMaxCols]: the series of column k (cols == NULL: all D + 2, in order), -1 beyond n_cols
inline Refusal select_columns(int D, const int32_t* cols, int n_cols, int* table) {
    if (n_cols < 1 || n_cols > DEMC_COV_MAX_COLS) return Refusal{DEMC_EINVAL, "demc_covariance: n_cols must be in 1 .. 64"};
    const int D2 = D + 2;
    if (!cols && n_cols != D2) return Refusal{DEMC_EINVAL, "demc_covariance: cols == NULL selects all D + 2 series: n_cols must equal D + 2 (at most 64)"};
    for (int k = 0; k < kCovMaxCols; ++k) table[k] = -1;
    for (int k = 0; k < n_cols; ++k) {
        table[k] = cols ? (int)cols[k] : k;
        if (table[k] < 0 || table[k] >= D2) return Refusal{DEMC_EINVAL, "demc_covariance: a column is outside [0, D + 2)"};
        for (int j = 0; j < k; ++j)
            if (table[j] == table[k]) return Refusal{DEMC_EINVAL, "demc_covariance: a column is repeated"};
    }
    return Refusal();
}

struct CovPlan {
    Refusal refused;
    int table[kCovMaxCols] = {};  // select_columns
    int K = 0, NB = 0;        // columns, blocks of 16 of them (the k_cov_syrk instance)
    long long chunks = 0;     // of kCovChunk cells
    int W = 0;                // workers: worker b takes the chunks b, b + W, ...
    // elements of the scratch buffers: cols (int), part1, mhat, part2, mean, mat (cov and cor each)
    size_t n_cols = 0, n_part1 = 0, n_mhat = 0, n_part2 = 0, n_mean = 0, n_mat = 0;
};

inline CovPlan plan_cov(long long N, int D, const int32_t* cols, int n_cols) {
    CovPlan c;
    if ((c.refused = select_columns(D, cols, n_cols, c.table))) return c;
    c.K = n_cols;
    c.NB = (c.K + 15) / 16;
    c.chunks = (N + kCovChunk - 1) / kCovChunk;
    c.W = (int)std::min<long long>(c.chunks, kCovMaxWorkers);
    c.n_cols = c.n_mhat = (size_t)kCovMaxCols; c.n_part1 = (size_t)c.W * kCovMaxCols; c.n_part2 = (size_t)c.W * cov_partial(c.NB);
    c.n_mean = (size_t)c.K; c.n_mat = (size_t)c.K * c.K;
    return c;
}

}  // namespace demc
