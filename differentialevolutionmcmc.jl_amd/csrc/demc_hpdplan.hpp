// demc_hpdplan.hpp -- everything demc_hpd (include/demc_hpd.h) decides before it touches the device: the constants of
// its two kernels, every refusal of its own with its text, the number of candidates m of an alpha, and one planner that takes the
// sort of one series as demc_rankplan.hpp planned it (tiles, scan, streaming grid) and adds the batch of series that fits the
// scratch budget -- two (key, position) buffers and the counts, no ranks and no derived series --, the grid of the window kernel
// and every scratch element count.  Pure functions of plain values, host only: plain C++17, no device header, no handle, no call
// into the runtime.  tests/hpdplan_host.cpp runs all of it on the CPU under the sanitizers.
#pragma once
#include "../../include/demc.h"
#include "../../include/demc_hpd.h"  // DEMC_HPD_COLS, DEMC_HPD_MAX_ALPHAS

#include <algorithm>
#include <cmath>
#include <cstddef>

#include "demc_hostbase.hpp"  // Refusal
#include "demc_rankplan.hpp"  // RankPlan, kRankBudget, kRankMaxBatch, kRankMaxN: the sort is section 5.11's

namespace demc {

// ---- the constants of the kernels ---------------------------------------------------------------------------------------------

constexpr int kHpdWG = 256;        // threads of k_hpd_window: lanes on consecutive candidates
constexpr int kHpdMaxBlocks = 64;  // the most workgroups one (series, alpha) gets; a thread strides by workgroups x kHpdWG beyond
constexpr int kHpdFinalWG = 64;    // threads of k_hpd_final: one wave per (series, alpha)
// bytes of scratch per pooled value of one series: two (key, position) buffers
constexpr size_t kHpdBytesPerValue = 2 * (8 + 4);

// ---- refusals -----------------------------------------------------------------------------------------------------------------

constexpr const char* kHpdNoHistory = "demc_hpd: history is not stored on this handle";
constexpr const char* kHpdBadRows = "bad rows: demc_hpd needs at least one row of the history";
constexpr const char* kHpdNoOutput = "demc_hpd: out is NULL";
constexpr const char* kHpdNoAlphas = "demc_hpd: alphas is NULL";
constexpr const char* kHpdBadCount = "demc_hpd: n_alphas must be between 1 and 16";
constexpr const char* kHpdBadAlpha = "demc_hpd: every alpha must be finite and strictly inside (0, 1)";
constexpr const char* kHpdSharded = "sharded handle: gather demc_get_history from every rank and take the intervals of the pool on the host";
constexpr const char* kHpdTooMany = "demc_hpd: N = n P is 2^31 or more, positions in the pool are 32-bit; pass a narrower window";

static_assert(DEMC_HPD_MAX_ALPHAS == 16, "kHpdBadCount names the cap");

// what the call has against its own arguments
inline Refusal hpd_args(bool has_out, const double* alphas, int n_alphas) {
    if (!has_out) return Refusal{DEMC_EINVAL, kHpdNoOutput};
    if (!alphas) return Refusal{DEMC_EINVAL, kHpdNoAlphas};
    if (n_alphas < 1 || n_alphas > DEMC_HPD_MAX_ALPHAS) return Refusal{DEMC_EINVAL, kHpdBadCount};
    for (int k = 0; k < n_alphas; ++k)
        if (!(std::isfinite(alphas[k]) && alphas[k] > 0.0 && alphas[k] < 1.0)) return Refusal{DEMC_EINVAL, kHpdBadAlpha};
    return Refusal();
}

// The window check of the posterior-statistics calls, in their order: no history, a bad row window, the call's own arguments, a
// sharded handle; then the cap on the pool.
inline Refusal check_hpd_window(bool stored, long long row0, long long row1, long long n_rows, bool sharded, long long P, Refusal args) {
    if (!stored) return Refusal{DEMC_EINVAL, kHpdNoHistory};
    if (row0 < 0 || row1 - row0 < 1 || row1 > n_rows) return Refusal{DEMC_EINVAL, kHpdBadRows};
    if (args) return args;
    if (sharded) return Refusal{DEMC_EINVAL, kHpdSharded};
    if (P < 1 || row1 - row0 > kRankMaxN / P) return Refusal{DEMC_EUNSUPPORTED, kHpdTooMany};
    return Refusal();
}

// ---- the candidates: m = max(1, ceil(alpha N)), the product one rounded multiplication of alpha by (double)N ---------------------

inline long long hpd_candidates(long long N, double alpha) {
    const double prod = alpha * (double)N;
    const long long m = (long long)std::ceil(prod);
    return std::max<long long>(1, std::min<long long>(m, N));  // (alpha < 1: the rounded product never exceeds N)
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------

struct HpdGrid {  // by value to the two kernels
    long long m[DEMC_HPD_MAX_ALPHAS];  // candidates of alpha k
    int wgs[DEMC_HPD_MAX_ALPHAS];      // workgroups that take them: workgroup x, thread t, trip s has candidate (s wgs + x) kHpdWG + t
    int n_alphas;
    int slots;                         // partials per (series, alpha): the largest wgs
};

struct HpdPlan {
    Refusal refused;
    long long n = 0, P = 0, N = 0;
    int series = 0;            // D + 2
    int batch = 0;             // series sorted side by side
    int batches = 0, last_batch = 0;
    int tiles = 0, blocks = 0, passes = 0;  // the sort of one series, as section 5.11 plans it
    long long scan_chunk = 0;
    HpdGrid grid{};
    // elements of the scratch buffers of a batch: keys (64-bit, two buffers), pos (32-bit, two buffers), hist (32-bit counts
    // [batch][256][tiles]), word (64-bit: or | and | unused per series), flag (int: NaN per series), the partials [batch][alpha][slots]
    // as a width (part_w) and a candidate (part_i) each, out ([series][alpha][4])
    size_t n_keys = 0, n_pos = 0, n_hist = 0, n_word = 0, n_flag = 0, n_part = 0, n_out = 0;
    size_t bytes_per_series = 0;
};

// `sort`: the plan of ONE series of the same window (n rows of P chains); `series` of them (D + 2) get their intervals.  The batch
// is what kRankBudget holds of this call's smaller scratch, at least one series and at most kRankMaxBatch.
inline HpdPlan plan_hpd(const RankPlan& sort, int series, const double* alphas, int n_alphas) {
    HpdPlan r;
    if (sort.refused) { r.refused = sort.refused.code == DEMC_EUNSUPPORTED ? Refusal{DEMC_EUNSUPPORTED, kHpdTooMany} : Refusal{DEMC_EINVAL, kHpdBadRows}; return r; }
    if (series < 1) { r.refused = Refusal{DEMC_EINVAL, kHpdBadRows}; return r; }
    if (Refusal a = hpd_args(true, alphas, n_alphas)) { r.refused = a; return r; }
    r.n = sort.n; r.P = sort.P; r.N = sort.N; r.series = series;
    r.tiles = sort.tiles; r.blocks = sort.blocks; r.passes = sort.passes; r.scan_chunk = sort.scan_chunk;
    r.bytes_per_series = (size_t)r.N * kHpdBytesPerValue + (size_t)r.tiles * 256 * 4;
    const size_t fit = std::max<size_t>(1, kRankBudget / r.bytes_per_series);
    r.batch = (int)std::min<size_t>(fit, (size_t)std::min(series, kRankMaxBatch));
    r.batches = (series + r.batch - 1) / r.batch;
    r.last_batch = series - (r.batches - 1) * r.batch;
    r.grid.n_alphas = n_alphas;
    r.grid.slots = 1;
    for (int k = 0; k < DEMC_HPD_MAX_ALPHAS; ++k) {
        r.grid.m[k] = k < n_alphas ? hpd_candidates(r.N, alphas[k]) : 0;
        r.grid.wgs[k] = k < n_alphas ? (int)std::min<long long>((r.grid.m[k] + kHpdWG - 1) / kHpdWG, kHpdMaxBlocks) : 0;
        r.grid.slots = std::max(r.grid.slots, r.grid.wgs[k]);
    }
    const size_t B = (size_t)r.batch;
    r.n_keys = 2 * B * (size_t)r.N; r.n_pos = 2 * B * (size_t)r.N; r.n_hist = B * 256 * (size_t)r.tiles;
    r.n_word = B * 3; r.n_flag = B; r.n_part = B * (size_t)n_alphas * (size_t)r.grid.slots;
    r.n_out = (size_t)series * (size_t)n_alphas * DEMC_HPD_COLS;
    return r;
}

}  // namespace demc
