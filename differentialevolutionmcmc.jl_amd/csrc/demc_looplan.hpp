// demc_looplan.hpp -- everything demc_loo (include/demc_loo.h) decides before it touches the device: the constants
// of its kernels, the tail length M(S), the cap on the draws, every refusal of its own with its text, and one planner that turns
// plain sizes into observation blocks, the grid of the term kernel, the LDS of the column kernel and the scratch element counts.
// The families and the window check are those of demc_pwplan.hpp (pw_family, check_pw_window) under the name demc_loo.  Pure
// functions of plain values, host only: plain C++17, no device header, no handle, no call into the runtime.  tests/looplan_host.cpp
// runs all of it on the CPU under the sanitizers.
#pragma once
#include "../../include/demc.h"
#include "../../include/demc_loo.h"  // DEMC_LOO_NTOTAL, DEMC_LOO_NPOINT, DEMC_LOO_MAX_DRAWS

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <string>

#include "demc_pwplan.hpp"  // PwModel, PwFamily, pw_family, pw_constants, check_pw_window, kPwWG, kPwPrepWG

namespace demc {

// ---- the constants of the kernels ---------------------------------------------------------------------------------------------

constexpr int kLooObs = 64;              // observations of a tile of k_loo_terms: one per lane, the four waves share the draws
constexpr int kLooTile = 16;             // draws of a tile: 16 doubles of a column are one 128-byte line
constexpr int kLooTargetWG = 2048;       // workgroups a launch of k_loo_terms aims at
constexpr int kLooWG = 512;              // threads of k_loo_column, one workgroup per observation
constexpr int kLooCap = 8192;            // keys the column kernel holds in LDS: the tail and what ties or floors keep beside it
constexpr int kLooMaxTail = 6144;        // M(DEMC_LOO_MAX_DRAWS)
constexpr int kLooBits = 11;             // bits of a digit of the select: 2048 bins, six digits (the last one of nine bits)
constexpr int kLooFitMax = 128;          // profile points of the fit at most: 30 + floor(sqrt(kLooMaxTail)) = 108
constexpr int kLooTotalsWG = 1024;       // threads of k_loo_totals, one workgroup
constexpr long long kLooMaxDraws = DEMC_LOO_MAX_DRAWS;
constexpr long long kLooMaxCells = 1LL << 27;  // terms of an observation block: the 1 GiB staging budget of demc_pointwise_loglik
// LDS of k_loo_column: keys [kLooCap] | tail values [kLooMaxTail] | histogram [2048] | two reduction rows [kLooWG] | bin sums [256] | words [16]
constexpr size_t kLooLdsBytes = (size_t)kLooCap * 8 + (size_t)kLooMaxTail * 8 + ((size_t)1 << kLooBits) * 4 + (size_t)kLooWG * 16 + 256 * 4 + 16 * 8;

static_assert(kLooCap > kLooMaxTail && kLooFitMax <= kLooWG && kLooObs * 4 == kPwWG, "the kernels are written for these shapes");

// M = ceil(min(0.2 S, 3 sqrt(S))) in FP64 as written
inline long long loo_tail_len(long long S) { return (long long)std::ceil(std::min(0.2 * (double)S, 3.0 * std::sqrt((double)S))); }

// ---- refusals -----------------------------------------------------------------------------------------------------------------

constexpr const char* kLooBadRows = "bad rows: demc_loo needs at least one row of the history";
constexpr const char* kLooSharded = "sharded handle: demc_loo reads the whole history of one handle";
constexpr const char* kLooNoOutput = "demc_loo: total_out and pointwise_out are both NULL";

inline Refusal loo_args(const Refusal& model, bool any_output) {
    if (model) return model;
    return any_output ? Refusal() : Refusal{DEMC_EINVAL, kLooNoOutput};
}
inline Refusal check_loo_draws(long long S) {
    if (S > kLooMaxDraws)
        return Refusal{DEMC_EINVAL, "demc_loo: S = " + std::to_string(S) + " draws are above the cap of " + std::to_string(kLooMaxDraws) +
                                        " (DEMC_LOO_MAX_DRAWS: the tail of an observation is sorted in LDS); pass a narrower window"};
    return Refusal();
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------

struct LooPlan {
    Refusal model;             // what pw_family has against the model (ranks where demc_waic ranks it)
    Refusal refused;           // that, or the cap on the draws
    PwFamily fam = PW_NONE;
    int K = 0;                 // constants per draw
    long long S = 0;           // draws
    int M = 0;                 // tail length; 0: S <= 20, no tail is formed
    long long Nb = 0;          // observations of a block (the last one ragged)
    int blocks = 0;
    int tiles = 0;             // of kLooObs observations, in a full block
    int chunks = 0;            // of chunk_len draws (a multiple of kLooTile), the last one ragged
    long long chunk_len = 0;
    int prep_blocks = 0;
    size_t lds_bytes = 0;
    // elements of the scratch buffers: cst [S][K], terms [Nb][S], point [N][6], total [8]
    size_t n_cst = 0, n_terms = 0, n_point = 0, n_total = 0;
};

inline LooPlan plan_loo(const PwModel& m, long long S) {
    LooPlan p;
    if ((p.model = pw_family(PW_LOO, m, &p.fam))) { p.refused = p.model; return p; }
    if (S < 1) { p.refused = Refusal{DEMC_EINVAL, "demc_loo: no draws (S < 1)"}; return p; }
    if ((p.refused = check_loo_draws(S))) return p;
    p.S = S;
    p.K = pw_constants(p.fam, m.n_acc, m.dp);
    p.M = S <= 20 ? 0 : (int)loo_tail_len(S);
    p.Nb = std::min<long long>(m.N, kLooMaxCells / S);
    p.blocks = (int)((m.N + p.Nb - 1) / p.Nb);
    p.tiles = (int)((p.Nb + kLooObs - 1) / kLooObs);
    const long long want = std::max<long long>(1, std::min<long long>(kLooTargetWG / p.tiles, (S + kLooTile - 1) / kLooTile));
    p.chunk_len = ((S + want - 1) / want + kLooTile - 1) / kLooTile * kLooTile;
    p.chunks = (int)((S + p.chunk_len - 1) / p.chunk_len);
    p.prep_blocks = (int)std::min<long long>((S + kPwPrepWG - 1) / kPwPrepWG, 1 << 20);
    p.lds_bytes = kLooLdsBytes;
    p.n_cst = (size_t)S * p.K;
    p.n_terms = (size_t)p.Nb * (size_t)S;
    p.n_point = (size_t)m.N * DEMC_LOO_NPOINT;
    p.n_total = DEMC_LOO_NTOTAL;
    return p;
}

}  // namespace demc
