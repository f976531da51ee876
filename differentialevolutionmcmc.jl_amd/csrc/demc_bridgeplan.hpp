// demc_bridgeplan.hpp -- everything demc_bridge (include/demc_bridge.h) decides before it touches the device, and
// the little host arithmetic it does between its kernels: the constants of the kernels, the split of the window into the fit half
// and the estimate half, the number of proposal draws, the chunks of P rows the log posterior is evaluated in, the geometry of the
// reductions, every refusal with its text, the kind of transform a scalar's bounds ask for with the transform itself (one text
// for the kernels and for the host), the Cholesky factorisation of the proposal's covariance, and the assembly of the twelve
// outputs.  Pure functions of plain values: plain C++17, no device header, no handle, no call into the runtime.
// tests/bridgeplan_host.cpp runs all of it on the CPU under the sanitizers.
#pragma once
#include "../../include/demc.h"
#include "../../include/demc_bridge.h"  // DEMC_BRIDGE_NOUT, DEMC_BRIDGE_MAX_D, DEMC_BRIDGE_MAX_DRAWS, DEMC_BRIDGE_MAX_ITER

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>

#include "demc_hostbase.hpp"  // Refusal
#include "demc_postplan.hpp"  // kHistoryNotStored, kCovMaxCols

#if defined(__HIPCC__)
#define DEMC_BRIDGE_HD __host__ __device__
#else
#define DEMC_BRIDGE_HD
#endif

namespace demc {

// ---- the constants of the kernels ---------------------------------------------------------------------------------------------

constexpr uint32_t kBridgeStream = 7;      // the Philox stream of the proposal draws (demc_philox.hpp's streams end at 6)
constexpr int kBridgeWG = 256;             // threads of the element-wise and the reduction kernels
constexpr int kBridgeLane = 64;            // threads of the draw kernel and of the triangular solve: one wave, a draw per lane
constexpr int kBridgeMaxW = 256;           // workgroups of a reduction over one of the two vectors at most
constexpr int kBridgePerThread = 4;        // elements a thread of a reduction takes before another workgroup is added
constexpr int kBridgeBatch = 8;            // iterations enqueued between two looks at the convergence flag
constexpr int kBridgeMaxIter = DEMC_BRIDGE_MAX_ITER;
constexpr double kBridgeTol = 1e-10;
constexpr int kBridgeFamSim = 101;         // the runtime's family of a simulation likelihood (the runtime asserts that they agree)
constexpr long long kBridgeMaxDraws = DEMC_BRIDGE_MAX_DRAWS;

static_assert(DEMC_BRIDGE_MAX_D == kCovMaxCols, "the proposal's covariance is demc_covariance's");

// words of the device state (unsigned long long) and its doubles
enum BridgeWord { BW_FLAG = 0, BW_ITER, BW_ZERO, BW_NONFINITE, BW_BAD, BW_FIRST_BAD, BW_LSTAR_KEY, BW_COUNT };
enum BridgeVal { BV_R = 0, BV_REL, BV_MEAN1, BV_MEAN2, BV_SS1, BV_SS2, BV_LSTAR, BV_COUNT };
enum BridgeFlag { BF_RUNNING = 0, BF_CONVERGED = 1, BF_STOPPED = 2 };

// ---- the transform to the real line ---------------------------------------------------------------------------------------------

enum BridgeKind : int { BK_NONE = 0, BK_LOWER = 1, BK_UPPER = 2, BK_BOTH = 3 };

// unset bounds are -Inf / +Inf (a NaN bound counts as unset)
DEMC_BRIDGE_HD inline int bridge_kind(double lo, double hi) {
    const double inf = std::numeric_limits<double>::infinity();
    return (lo > -inf ? 1 : 0) | (hi < inf ? 2 : 0);
}

// xi of theta.  On or outside a finite bound the result is not finite (the call refuses such a window).
DEMC_BRIDGE_HD inline double bridge_forward(double theta, double lo, double hi) {
    switch (bridge_kind(lo, hi)) {
        case BK_LOWER: return log(theta - lo);
        case BK_UPPER: return log(hi - theta);
        case BK_BOTH: {
            const double u = (theta - lo) / (hi - lo);
            return log(u) - log1p(-u);
        }
        default: return theta;
    }
}

// theta of xi
DEMC_BRIDGE_HD inline double bridge_inverse(double xi, double lo, double hi) {
    switch (bridge_kind(lo, hi)) {
        case BK_LOWER: return lo + exp(xi);
        case BK_UPPER: return hi - exp(xi);
        case BK_BOTH: return lo + (hi - lo) / (1.0 + exp(-xi));
        default: return xi;
    }
}

// log |d theta / d xi| at xi
DEMC_BRIDGE_HD inline double bridge_logjac(double xi, double lo, double hi) {
    switch (bridge_kind(lo, hi)) {
        case BK_LOWER:
        case BK_UPPER: return xi;
        case BK_BOTH: {
            const double a = fabs(xi);
            return log(hi - lo) - a - 2.0 * log1p(exp(-a));
        }
        default: return 0.0;
    }
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------

constexpr const char* kBridgeBadRows = "bad rows: demc_bridge needs at least two rows of the history";
constexpr const char* kBridgeNoModel = "demc_bridge: no model is set on this handle";
constexpr const char* kBridgeSim =
    "demc_bridge: a simulation likelihood (demc_set_model_sim) gives a noisy log posterior; bridge sampling needs an exact one";
constexpr const char* kBridgeNoOut = "demc_bridge: out is NULL";
constexpr const char* kBridgeSharded = "sharded handle: demc_bridge reads the whole history of one handle";
constexpr const char* kBridgeNegProp = "demc_bridge: n_prop must be >= 0 (0: as many proposal draws as the estimate half holds)";

// what the call is asked and what the handle knows: `family` is the DEMC_FAM_* code, -1 without a model, kBridgeFamSim for a
// simulation likelihood
struct BridgeCall {
    bool stored = false;       // the handle keeps a history
    long long row0 = 0, row1 = 0, n_rows = 0;
    int family = -1;
    bool has_out = false;
    bool sharded = false;
    long long n_prop = 0;
    int D = 0;
    long long P = 0;
};

struct BridgePlan {
    Refusal refused;
    long long R = 0, rmid = 0;   // rows of the window; the first row of the estimate half
    long long n_win = 0;         // draws of the window
    long long n_fit = 0, N1 = 0, N2 = 0;
    long long chunks1 = 0;       // evaluations of P rows over the estimate half (whole rows of the history: none is padded)
    long long chunks2 = 0;       // ... over the proposal draws; the last one is padded with copies of draw N2 - 1
    long long pad2 = 0;          // rows of the proposal buffer = chunks2 P
    long long last2 = 0;         // valid rows of the last chunk
    int W1 = 0, W2 = 0;          // workgroups of a reduction over the estimate half / over the proposal draws
    double s1 = 0.0, s2 = 0.0;
    int draw_blocks = 0, solve_blocks = 0;  // workgroups of kBridgeLane lanes
    size_t lds_bytes = 0;        // of the draw kernel and the solve: D doubles per lane
};

inline int bridge_workers(long long n) {
    const long long per = (long long)kBridgeWG * kBridgePerThread;
    return (int)std::max<long long>(1, std::min<long long>((n + per - 1) / per, kBridgeMaxW));
}

// The refusals in the order they rank (include/demc_bridge.h), then the plan.
inline BridgePlan plan_bridge(const BridgeCall& c) {
    BridgePlan p;
    auto refuse = [&](int code, const std::string& text) { p.refused = Refusal{code, text}; return p; };
    if (!c.stored) return refuse(DEMC_EINVAL, kHistoryNotStored);
    if (c.row0 < 0 || c.row1 > c.n_rows || c.row1 - c.row0 < 2) return refuse(DEMC_EINVAL, kBridgeBadRows);
    if (c.family < 0) return refuse(DEMC_EINVAL, kBridgeNoModel);
    if (c.family == kBridgeFamSim) return refuse(DEMC_EUNSUPPORTED, kBridgeSim);
    if (!c.has_out) return refuse(DEMC_EINVAL, kBridgeNoOut);
    if (c.sharded) return refuse(DEMC_EINVAL, kBridgeSharded);
    if (c.n_prop < 0) return refuse(DEMC_EINVAL, kBridgeNegProp);
    if (c.D > DEMC_BRIDGE_MAX_D)
        return refuse(DEMC_EINVAL, "demc_bridge: D = " + std::to_string(c.D) + " is above the cap of " + std::to_string(DEMC_BRIDGE_MAX_D) +
                                       " (DEMC_BRIDGE_MAX_D: the covariance of the proposal)");
    p.R = c.row1 - c.row0;
    p.rmid = c.row0 + p.R / 2;
    p.n_win = p.R * c.P;
    p.n_fit = (p.rmid - c.row0) * c.P;
    p.N1 = (c.row1 - p.rmid) * c.P;
    p.N2 = c.n_prop > 0 ? c.n_prop : p.N1;
    if (p.n_fit <= c.D)
        return refuse(DEMC_EINVAL, "demc_bridge: the fit half holds N_fit = " + std::to_string(p.n_fit) + " draws, the covariance of the proposal needs more than D = " +
                                       std::to_string(c.D) + "; pass a wider window");
    if (p.N1 > kBridgeMaxDraws || p.N2 > kBridgeMaxDraws)
        return refuse(DEMC_EINVAL, "demc_bridge: N1 = " + std::to_string(p.N1) + " and N2 = " + std::to_string(p.N2) + " draws: one is above the cap of " +
                                       std::to_string(kBridgeMaxDraws) + " (DEMC_BRIDGE_MAX_DRAWS); pass a narrower window or a smaller n_prop");
    p.chunks1 = p.N1 / c.P;
    p.chunks2 = (p.N2 + c.P - 1) / c.P;
    p.pad2 = p.chunks2 * c.P;
    p.last2 = p.N2 - (p.chunks2 - 1) * c.P;
    p.W1 = bridge_workers(p.N1);
    p.W2 = bridge_workers(p.N2);
    p.s1 = (double)p.N1 / (double)(p.N1 + p.N2);
    p.s2 = (double)p.N2 / (double)(p.N1 + p.N2);
    p.draw_blocks = (int)((p.pad2 + kBridgeLane - 1) / kBridgeLane);
    p.solve_blocks = (int)((p.N1 + kBridgeLane - 1) / kBridgeLane);
    p.lds_bytes = (size_t)std::max(c.D, 1) * kBridgeLane * sizeof(double);
    return p;
}

// a window draw whose xi is not finite: `first` is the linear index (draw of the window) D + scalar of the first one
inline Refusal bridge_bad_draws(long long count, long long first, long long row0, long long P, int D) {
    const long long e = first / D, k = first % D;
    return Refusal{DEMC_EINVAL, "demc_bridge: " + std::to_string(count) + " scalar(s) of the window lie on or outside a finite bound or are NaN (the first: row " +
                                    std::to_string(row0 + e / P) + ", slot " + std::to_string(e % P) + ", scalar " + std::to_string(k) +
                                    "); the transform to the real line needs every draw strictly inside the bounds"};
}

// ---- the Cholesky factorisation -------------------------------------------------------------------------------------------------

// V [D][D] (its lower triangle is read) -> L [D][D] row-major, lower, the upper triangle 0.0; column by column, the sums in index
// order.  Returns -1, or the index of the first pivot that is not positive (a NaN included); L is then not to be used.
inline int bridge_cholesky(const double* V, int D, double* L) {
    for (int i = 0; i < D * D; ++i) L[i] = 0.0;
    for (int j = 0; j < D; ++j) {
        double s = V[(size_t)j * D + j];
        for (int k = 0; k < j; ++k) s -= L[(size_t)j * D + k] * L[(size_t)j * D + k];
        if (!(s > 0.0) || !std::isfinite(s)) return j;
        const double d = std::sqrt(s);
        L[(size_t)j * D + j] = d;
        for (int i = j + 1; i < D; ++i) {
            double t = V[(size_t)i * D + j];
            for (int k = 0; k < j; ++k) t -= L[(size_t)i * D + k] * L[(size_t)j * D + k];
            L[(size_t)i * D + j] = t / d;
        }
    }
    return -1;
}

inline Refusal bridge_bad_pivot(int j, int D) {
    return Refusal{DEMC_EINVAL, "demc_bridge: the covariance of the fit half is not positive definite (pivot " + std::to_string(j) + " of " + std::to_string(D) +
                                    " is not positive): a scalar is constant or the draws are collinear"};
}

// sum_k log L_kk + (D / 2) log 2 pi, in index order: what log g subtracts from -|z|^2 / 2
inline double bridge_lognorm(const double* L, int D) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += std::log(L[(size_t)k * D + k]);
    return s + 0.5 * (double)D * 1.8378770664093454835606594728112;
}

// ---- the outputs ----------------------------------------------------------------------------------------------------------------

// out[DEMC_BRIDGE_NOUT] from the device state after the last kernel.  An iterate r that is not a positive finite number (0 by
// underflow, +Inf, NaN) has stopped the iteration: the count includes that iteration, converged is 0 whatever the flag says (the
// kernel's test |change| <= tol |r| holds at r = +Inf), and logml, the error terms and the last change are NaN, as under n_nonfinite.
inline void bridge_outputs(const BridgePlan& p, const double* val, const unsigned long long* word, double* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double r = val[BV_R];
    const bool r_ok = std::isfinite(r) && r > 0.0;
    const bool bad = word[BW_NONFINITE] > 0 || !std::isfinite(val[BV_LSTAR]) || !r_ok;
    out[0] = bad ? nan : std::log(r) + val[BV_LSTAR];
    out[1] = bad ? nan : val[BV_SS1] / (double)(p.N2 - 1) / (val[BV_MEAN1] * val[BV_MEAN1]) / (double)p.N2;
    out[2] = bad ? nan : val[BV_SS2] / (double)(p.N1 - 1) / (val[BV_MEAN2] * val[BV_MEAN2]) / (double)p.N1;
    out[3] = (double)word[BW_ITER];
    out[4] = word[BW_FLAG] == BF_CONVERGED && r_ok ? 1.0 : 0.0;
    out[5] = (double)p.n_fit;
    out[6] = (double)p.N1;
    out[7] = (double)p.N2;
    out[8] = val[BV_LSTAR];
    out[9] = (double)word[BW_ZERO];
    out[10] = (double)word[BW_NONFINITE];
    out[11] = bad ? nan : val[BV_REL];
}

}  // namespace demc
