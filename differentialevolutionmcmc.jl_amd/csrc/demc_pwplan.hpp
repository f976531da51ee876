// demc_pwplan.hpp -- everything the two per-observation calls (demc_pointwise_loglik, demc_waic; include/demc_pointwise.h,
// DESIGN.md 5.8) decide before they touch the device: the constants of their kernels, which families they serve, every refusal
// and its text, and one planner that turns plain sizes into observation tiles, draw chunks, the constants per draw and the scratch
// element counts.  Pure functions of plain values, host only: plain C++17, no device header, no handle, no call into the runtime.
// The kernel header includes this file for the constants; the *_run functions do what a plan says.  tests/pwplan_host.cpp runs all
// of it on the CPU under the sanitizers.
#pragma once
#include "../../include/demc.h"
#include "../../include/demc_pointwise.h"  // DEMC_PW_MAX_CELLS, DEMC_WAIC_NTOTAL, DEMC_WAIC_NPOINT

#include <algorithm>
#include <cstddef>
#include <string>

#include "demc_postplan.hpp"  // HistView, kHistoryNotStored, Refusal

namespace demc {

// ---- the constants of the kernels ---------------------------------------------------------------------------------------------

constexpr int kPwWG = 256;            // threads of k_pw_accumulate / k_pw_matrix = observations of a tile, one per lane
constexpr int kPwMinChunk = 64;       // draws a chunk holds at least: below that the partials cost more than the walk
constexpr int kPwTargetWG = 2048;     // workgroups a launch aims at (eight per CU) ...
constexpr int kPwMaxChunks = 1024;    // ... and the most chunks it is cut into: bounds partial[chunks][5][N]
constexpr int kPwPartial = 5;         // a lane's partial of a chunk: M, E, mean, M2, flags
constexpr int kPwPrepWG = 256;        // threads of k_pw_prepare: a draw each
constexpr int kPwTotalsWG = 1024;     // threads of k_pw_totals, one workgroup
constexpr long long kPwMaxCells = DEMC_PW_MAX_CELLS;  // n N of demc_pointwise_loglik: 1 GiB of staging
constexpr long long kPwMaxDraws = 1LL << 40;          // S of either call: far beyond any history, keeps S K inside 64 bits

// the families as the kernels are instantiated (the handle's family and likelihood mode decide: pw_family)
enum PwFamily : int { PW_NONE = -1, PW_GAUSSIAN = 0, PW_BINOMIAL = 1, PW_LNR = 2, PW_LBA = 3, PW_MVN_ISO = 4, PW_MVN_FULL = 5 };
enum PwCall : int { PW_LOGLIK = 0, PW_WAIC = 1, PW_LOO = 2 };  // (PW_LOO: demc_loo of demc_looplan.hpp borrows pw_family and the window check)
constexpr const char* kPwWho[3] = {"demc_pointwise_loglik", "demc_waic", "demc_loo"};

constexpr int kPwFamSim = 101;  // the runtime's internal family of a simulation likelihood (FAM_SIM of demc_simlike.hpp: the runtime asserts that they agree)

// what the handle knows of its model: `family` is the DEMC_FAM_* code, -1 without a model, kPwFamSim for a simulation likelihood
struct PwModel {
    int family = -1;
    bool direct = false;  // loglike_mode = DEMC_LOGLIKE_DIRECT
    long long N = 0;      // observations
    int n_acc = 0;        // LBA / LNR
    int d = 0, dp = 0;    // MvNormal: row length and the padded length of a whitened row (8 / 16 / 32 / 64)
};

// Constants a draw is turned into by k_pw_prepare (demc_pointwise.hpp says which); the last one is the draw's flag (1.0: every
// term of the draw is NaN -- a row outside the bounds, a NaN in the row).
inline int pw_constants(PwFamily f, int n_acc, int dp) {
    switch (f) {
        case PW_GAUSSIAN: return 3 + 1;        // mu, 1 / sigma, -log sigma - log(2 pi) / 2
        case PW_BINOMIAL: return 2 + 1;        // log p, log1p(-p)
        case PW_LNR: return n_acc + 1 + 1;     // nu[a], tau
        case PW_LBA: return 2 * n_acc + 6 + 1; // nu[a], S nu[a], S k, S b, tau, 1 / A, 1 / (S A), 1 / (1 - P(all drifts <= 0))
        case PW_MVN_ISO: return dp + 2 + 1;    // m[dp], -d log(2 pi) / 2 - d log sigma, 1 / (2 sigma^2)
        case PW_MVN_FULL: return dp + 1;       // m[dp]
        default: return 0;
    }
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------

inline const char* pw_family_name(int family) {
    switch (family) {
        case DEMC_FAM_HIER_BINOMIAL: return "DEMC_FAM_HIER_BINOMIAL";
        case DEMC_FAM_HIER_GAUSSIAN: return "DEMC_FAM_HIER_GAUSSIAN";
        case DEMC_FAM_RASTRIGIN: return "DEMC_FAM_RASTRIGIN";
        case DEMC_FAM_ODE_LV: return "DEMC_FAM_ODE_LV";
        case DEMC_FAM_USER: return "DEMC_FAM_USER (a hiprtc plug-in)";
        case kPwFamSim: return "a simulation likelihood (demc_set_model_sim)";
        default: return "this family";
    }
}

// which instance serves the model, or why none does.  A served family whose model holds no observation (the race models accept
// dims = [0, n_acc]) has nothing to answer about: refused, so that no plan divides by its tiles and no lane reads observation -1.
inline Refusal pw_family(PwCall call, const PwModel& m, PwFamily* out) {
    const std::string who = kPwWho[call];
    *out = PW_NONE;
    const bool served = m.family == DEMC_FAM_GAUSSIAN || m.family == DEMC_FAM_BINOMIAL || m.family == DEMC_FAM_LNR || m.family == DEMC_FAM_LBA ||
                        ((m.family == DEMC_FAM_MVN_ISO || m.family == DEMC_FAM_MVN_FULL) && m.direct);
    if (served && m.N < 1) return Refusal{DEMC_EINVAL, who + ": the model holds no observations (N < 1)"};
    switch (m.family) {
        case -1: return Refusal{DEMC_EINVAL, who + ": no model is set on this handle"};
        case DEMC_FAM_GAUSSIAN: *out = PW_GAUSSIAN; return Refusal();
        case DEMC_FAM_BINOMIAL: *out = PW_BINOMIAL; return Refusal();
        case DEMC_FAM_LNR: *out = PW_LNR; return Refusal();
        case DEMC_FAM_LBA: *out = PW_LBA; return Refusal();
        case DEMC_FAM_MVN_ISO:
        case DEMC_FAM_MVN_FULL:
            if (!m.direct)
                return Refusal{DEMC_EUNSUPPORTED, who + ": the MvNormal families keep sums over the data in this likelihood mode, not its rows; create the handle "
                                                        "with loglike_mode = direct (DEMC_LOGLIKE_DIRECT) for per-observation terms"};
            *out = m.family == DEMC_FAM_MVN_ISO ? PW_MVN_ISO : PW_MVN_FULL;
            return Refusal();
        default:
            return Refusal{DEMC_EUNSUPPORTED, who + ": " + pw_family_name(m.family) + " has no per-observation log-density on the device"};
    }
}

constexpr const char* kPwBadRows = "bad rows: demc_waic needs at least one row of the history";
constexpr const char* kPwSharded = "sharded handle: gather demc_get_history from every rank and evaluate demc_pointwise_loglik on one";
constexpr const char* kPwNoOutput = "demc_waic: total_out and pointwise_out are both NULL";
constexpr const char* kPwNoRows = "demc_pointwise_loglik: n < 1";

// demc_waic's window, in the order check_history_window refuses: no history, a bad row window, `args` (what the call has against
// its model, then against its outputs: pw_waic_args), a sharded handle
inline Refusal pw_waic_args(const Refusal& model, bool any_output) {
    if (model) return model;
    return any_output ? Refusal() : Refusal{DEMC_EINVAL, kPwNoOutput};
}
inline Refusal check_pw_window(bool stored, long long row0, long long row1, long long n_rows, bool sharded, Refusal args = Refusal(),
                               const char* bad_rows = kPwBadRows, const char* sharded_text = kPwSharded) {
    if (!stored) return Refusal{DEMC_EINVAL, kHistoryNotStored};
    if (row0 < 0 || row1 - row0 < 1 || row1 > n_rows) return Refusal{DEMC_EINVAL, bad_rows};
    if (args) return args;
    if (sharded) return Refusal{DEMC_EINVAL, sharded_text};
    return Refusal();
}

// demc_pointwise_loglik's own arguments
inline Refusal check_pw_rows(long long n, long long N) {
    if (n < 1) return Refusal{DEMC_EINVAL, kPwNoRows};
    if (N > 0 && n > kPwMaxCells / N)
        return Refusal{DEMC_EINVAL, "demc_pointwise_loglik: n N = " + std::to_string(n) + " x " + std::to_string(N) + " is above the cap of " +
                                        std::to_string(kPwMaxCells) + " cells (DEMC_PW_MAX_CELLS: the matrix is staged on the device); pass fewer rows per call"};
    return Refusal();
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------

struct PwPlan {
    Refusal refused;
    PwFamily fam = PW_NONE;
    int K = 0;                 // constants per draw
    long long S = 0;           // draws
    int tiles = 0;             // of kPwWG observations
    int chunks = 0;            // of chunk_len draws, the last one ragged
    long long chunk_len = 0;
    int prep_blocks = 0, final_blocks = 0;
    // elements of the scratch buffers: cst [S][K], part [chunks][kPwPartial][N], point [N][4], total [8], matrix [S][N], theta [S][D]
    size_t n_cst = 0, n_part = 0, n_point = 0, n_total = 0, n_matrix = 0, n_theta = 0;
};

// S draws of D scalars under model m.  The grid of the walking kernels is tiles x chunks: as many chunks as bring the launch to
// kPwTargetWG workgroups, none shorter than kPwMinChunk draws, at most kPwMaxChunks; the draws are dealt evenly (chunk_len =
// ceil(S / chunks), then as many chunks as that length needs).
inline PwPlan plan_pointwise(PwCall call, const PwModel& m, long long S, int D) {
    PwPlan p;
    if ((p.refused = pw_family(call, m, &p.fam))) return p;
    if (call == PW_LOGLIK && (p.refused = check_pw_rows(S, m.N))) return p;
    if (S < 1) { p.refused = Refusal{DEMC_EINVAL, std::string(kPwWho[call]) + ": no draws (S < 1)"}; return p; }
    if (S > kPwMaxDraws) { p.refused = Refusal{DEMC_EINVAL, std::string(kPwWho[call]) + ": too many draws"}; return p; }
    p.S = S;
    p.K = pw_constants(p.fam, m.n_acc, m.dp);
    p.tiles = (int)((m.N + kPwWG - 1) / kPwWG);
    const long long fill = std::max<long long>(1, kPwTargetWG / p.tiles);
    const long long want = std::max<long long>(1, std::min<long long>(std::min<long long>(fill, kPwMaxChunks), (S + kPwMinChunk - 1) / kPwMinChunk));
    p.chunk_len = (S + want - 1) / want;
    p.chunks = (int)((S + p.chunk_len - 1) / p.chunk_len);
    p.prep_blocks = (int)std::min<long long>((S + kPwPrepWG - 1) / kPwPrepWG, 1 << 20);
    p.final_blocks = p.tiles;
    p.n_cst = (size_t)S * p.K;
    if (call == PW_WAIC) {
        p.n_part = (size_t)p.chunks * kPwPartial * (size_t)m.N;
        p.n_point = (size_t)m.N * DEMC_WAIC_NPOINT;
        p.n_total = DEMC_WAIC_NTOTAL;
    } else {
        p.n_matrix = (size_t)S * (size_t)m.N;
        p.n_theta = (size_t)S * D;
    }
    return p;
}

}  // namespace demc
