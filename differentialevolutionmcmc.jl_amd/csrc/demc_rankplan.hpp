// demc_rankplan.hpp -- everything demc_rankstats and demc_rank_series (include/demc_rank.h) decide before they touch
// the device: the constants of their kernels, every refusal of their own with its text, the three quantile targets by section 5.6's
// arithmetic, and one planner that turns plain sizes into the batch of series that fits a fixed scratch budget, the tiles and grids
// of the sort, its passes and every scratch element count.  Pure functions of plain values, host only: plain C++17, no device
// header, no handle, no call into the runtime.  tests/rankplan_host.cpp runs all of it on the CPU under the sanitizers.
#pragma once
#include "../../include/demc.h"
#include "../../include/demc_rank.h"  // DEMC_RANK_COLS, DEMC_RANK_KIND_*

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "demc_hostbase.hpp"  // Refusal

namespace demc {

// ---- the constants of the kernels ---------------------------------------------------------------------------------------------

constexpr int kRankBits = 8;                  // bits of a digit of the LSD radix sort: 256 bins
constexpr int kRankPasses = 64 / kRankBits;   // digits of a key, least significant first
constexpr int kRankWave = 64;                 // threads of k_rank_hist and k_rank_scatter: one wave per tile
constexpr int kRankTile = 2048;               // (key, position) pairs of a tile: 32 rounds of a wave
constexpr int kRankScanWG = 1024;             // threads of k_rank_scan, one workgroup per series
constexpr int kRankWG = 256;                  // threads of the streaming kernels (keys, range, ties, derive)
constexpr int kRankMaxBlocks = 4096;          // ... and the most workgroups one series of them gets (grid-stride beyond)
constexpr int kRankMaxBatch = 16;             // series sorted side by side at most: 64 derived series per summary run
constexpr int kRankDerived = 4;               // derived series per series: z | x <= q05 | x <= q95 | zeta, then z'
constexpr size_t kRankBudget = (size_t)4 << 30;  // scratch a batch may take (a single series is run whatever it takes)
constexpr long long kRankMaxN = (1LL << 31) - 1;  // positions are 32-bit
// bytes of scratch per pooled value of one series: two (key, position) buffers, the ranks, four derived series
constexpr size_t kRankBytesPerValue = 2 * (8 + 4) + 8 + kRankDerived * 8;

static_assert(kRankTile % kRankWave == 0 && kRankPasses * kRankBits == 64, "the sort is written for whole rounds and whole digits");

// ---- refusals -----------------------------------------------------------------------------------------------------------------

constexpr const char* kRankNoHistory = "demc_rankstats: history is not stored on this handle";
constexpr const char* kRankBadRows = "bad rows: demc_rankstats needs at least one row of the history";
constexpr const char* kRankSharded = "sharded handle: gather demc_get_history from every rank and rank the pool on the host";
constexpr const char* kRankNoOutput = "demc_rankstats: out is NULL";
constexpr const char* kRankBadLag = "demc_rankstats: max_lag is negative";
constexpr const char* kRankBadSeries = "demc_rank_series: series is outside [0, D + 2)";
constexpr const char* kRankBadKind = "demc_rank_series: kind must be 0 (ranks), 1 (normal scores) or 2 (ranks of |x - med|)";
constexpr const char* kRankTooMany = "demc_rankstats: N = n P is 2^31 or more, positions in the pool are 32-bit; pass a narrower window";

// what a call has against its own arguments (series < 0 with kind < 0: demc_rankstats, which has neither)
inline Refusal rank_args(bool has_out, int max_lag, bool single, int series, int kind, int D) {
    if (!has_out) return Refusal{DEMC_EINVAL, kRankNoOutput};
    if (max_lag < 0) return Refusal{DEMC_EINVAL, kRankBadLag};
    if (single && (series < 0 || series >= D + 2)) return Refusal{DEMC_EINVAL, kRankBadSeries};
    if (single && (kind < DEMC_RANK_KIND_RANK || kind > DEMC_RANK_KIND_FOLDED)) return Refusal{DEMC_EINVAL, kRankBadKind};
    return Refusal();
}

// The window check of the posterior-statistics calls, in their order: no history, a bad row window, the call's own arguments, a
// sharded handle; then the cap on the pool.
inline Refusal check_rank_window(bool stored, long long row0, long long row1, long long n_rows, bool sharded, long long P, Refusal args) {
    if (!stored) return Refusal{DEMC_EINVAL, kRankNoHistory};
    if (row0 < 0 || row1 - row0 < 1 || row1 > n_rows) return Refusal{DEMC_EINVAL, kRankBadRows};
    if (args) return args;
    if (sharded) return Refusal{DEMC_EINVAL, kRankSharded};
    if (P < 1 || row1 - row0 > kRankMaxN / P) return Refusal{DEMC_EUNSUPPORTED, kRankTooMany};
    return Refusal();
}

// ---- the three quantiles (DESIGN.md 5.6's arithmetic: aleph = N p + (1 - p) as a rounded product and a rounded sum) --------------

constexpr double kRankProbs[3] = {0.5, 0.05, 0.95};  // med, q05, q95

struct RankTargets {  // by value to k_rank_ties
    long long j[3];   // x_(j) and x_(j+1) are the sorted positions j - 1 and j (N = 1: both 0)
    double gamma[3];
};

inline RankTargets rank_targets(long long N) {
    RankTargets t{};
    for (int k = 0; k < 3; ++k) {
        const double p = kRankProbs[k];
        const double prod = (double)N * p;
        const double aleph = prod + (1.0 - p);
        long long j = (long long)std::trunc(aleph);
        j = std::max<long long>(1, std::min<long long>(j, N - 1));
        if (N == 1) j = 1;
        t.j[k] = j;
        t.gamma[k] = N == 1 ? 0.0 : std::min(1.0, std::max(0.0, aleph - (double)j));
    }
    return t;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------

struct RankPlan {
    Refusal refused;
    long long n = 0, P = 0, N = 0;
    int series = 0;            // series the call ranks: D + 2, or 1 (demc_rank_series)
    int batch = 0;             // series sorted side by side
    int batches = 0, last_batch = 0;  // ... and how many of them the last batch holds
    int tiles = 0;             // of kRankTile pairs, per series
    int blocks = 0;            // workgroups per series of the streaming kernels
    long long scan_chunk = 0;  // consecutive (digit, tile) counts a thread of k_rank_scan adds
    int passes = kRankPasses;
    RankTargets tg{};
    // elements of the scratch buffers of a batch: keys (64-bit, two buffers), pos (32-bit, two buffers), rk (ranks), der (the derived
    // history [N][4 batch]), hist (32-bit counts [batch][256][tiles]), zero_lp / zero_acc (the two internal series of the derived
    // history: N doubles, N bytes), word (64-bit: or | and | distinct per series and round), flag (int: NaN per series and
    // round), q (med | q05 | q95 per series), out ([series][8])
    size_t n_keys = 0, n_pos = 0, n_rk = 0, n_der = 0, n_hist = 0, n_zero = 0, n_word = 0, n_flag = 0, n_q = 0, n_out = 0;
    size_t bytes_per_series = 0;
};

// n rows of P chains; `series` of them are ranked (D + 2, or 1).  The batch is what kRankBudget holds, at least one series and at
// most kRankMaxBatch.
inline RankPlan plan_rank(long long n, long long P, int series) {
    RankPlan r;
    if (n < 1 || P < 1 || series < 1) { r.refused = Refusal{DEMC_EINVAL, kRankBadRows}; return r; }
    if (n > kRankMaxN / P) { r.refused = Refusal{DEMC_EUNSUPPORTED, kRankTooMany}; return r; }
    r.n = n; r.P = P; r.series = series;
    const long long N = r.N = n * P;
    r.tiles = (int)((N + kRankTile - 1) / kRankTile);
    r.blocks = (int)std::min<long long>((N + kRankWG - 1) / kRankWG, kRankMaxBlocks);
    r.bytes_per_series = (size_t)N * kRankBytesPerValue + (size_t)r.tiles * 256 * 4;
    const size_t fit = std::max<size_t>(1, kRankBudget / r.bytes_per_series);
    r.batch = (int)std::min<size_t>(fit, (size_t)std::min(series, kRankMaxBatch));
    r.batches = (series + r.batch - 1) / r.batch;
    r.last_batch = series - (r.batches - 1) * r.batch;
    const long long entries = (long long)r.tiles * 256;
    r.scan_chunk = (entries + kRankScanWG - 1) / kRankScanWG;
    r.tg = rank_targets(N);
    const size_t B = (size_t)r.batch;
    r.n_keys = 2 * B * (size_t)N; r.n_pos = 2 * B * (size_t)N; r.n_rk = B * (size_t)N; r.n_der = (size_t)N * kRankDerived * B;
    r.n_hist = B * 256 * (size_t)r.tiles; r.n_zero = (size_t)N; r.n_word = B * 6; r.n_flag = B * 2; r.n_q = B * 3;
    r.n_out = (size_t)series * DEMC_RANK_COLS;
    return r;
}

}  // namespace demc
