// demc_bridge.hpp -- the marginal likelihood on the device by bridge sampling (include/demc_bridge.h: demc_bridge; the definition
// is DESIGN.md 5.10).  The window is cut into a fit half and an estimate half (demc_bridgeplan.hpp); then, all on the handle's stream:
//
//   k_bridge_transform   a thread per draw of the window: xi[e][D] dense from the history's cells (ld doubles apart), logJ[e], and
//                        the dense theta rows of the estimate half; a xi that is not finite is counted and the first one kept
//                        (integer atomics: a count and a minimum).  The bounds are read wave-uniformly from the handle's table.
//   cov_run              demc_covariance's own kernels (demc_cov.cpp, unchanged) over the fit half of xi, presented as a history
//                        with ld = D: m and V.  The Cholesky factorisation is the host's (bridge_cholesky).
//   k_bridge_draw        a lane per proposal draw, a wave per workgroup: Philox blocks of stream 7, Box-Muller, z parked in the
//                        lane's column of LDS, xi = m + L z with L read wave-uniformly, theta, logJ and log g, written straight
//                        into the rows of the P-row chunks the evaluation reads; the rows that pad the last chunk repeat draw N2 - 1.
//   k_bridge_solve       a lane per draw of the estimate half: y = L^-1 (xi - m) by forward substitution, y parked in LDS, log g.
//   (the callback)       the handle's own evaluate path over every chunk: lp.
//   k_bridge_logs        l1 and l2, the two counts, and l* = max l1 as an integer atomic maximum of the order-preserving keys: exact,
//                        whatever the order.
//   k_bridge_exp         exp(x1) and exp(-x2), once; r = 1; the iteration is stopped at once where a NaN or +Inf was counted.
//   k_bridge_part<MODE>  grid = W2 + W1 workgroups: workgroup b sums its elements (thread t of it takes t, t + W 256, ...) by a halving
//                        tree -> part[b].  MODE 0: the two means of an iteration; 1: f1 and f2; 2: their squared deviations.
//   k_bridge_final<MODE> one workgroup: the partial sums in index order by the same tree; MODE 0 forms r_{t+1}, the change and the
//                        flag.  Both kernels of an iteration return at once when the flag is set: what is enqueued past convergence
//                        does nothing, and the result does not depend on how many iterations a batch holds.
// No floating-point atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>

#include "demc_bridgeplan.hpp"  // host-only: the kBridge* constants, BridgePlan, the transform, the Cholesky
#include "demc_dimtab.hpp"      // DimTab: the bounds
#include "demc_postplan.hpp"    // HistView

namespace demc {

struct BridgeKParams {
    const double* hist;  // at row row0: [n_win][ld]
    const DimTab* tab;   // [D] the bounds
    int D, ld;
    long long n_win, n_fit, N1, N2, pad2;
    double* xi;          // [n_win][D]
    double* lj1;         // [n_win] logJ of the window's draws
    double *th1, *lp1, *lg1;  // [N1][D], [N1], [N1]
    double *th2, *lp2;   // [pad2][D], [pad2]
    double *lj2, *lg2;   // [N2]
    double *l1, *l2;     // [N1], [N2]
    double *e1, *e2;     // exp(x1) [N1], exp(-x2) [N2]
    const double* fit;   // m [D] | L [D][D] | sum log L_kk + (D / 2) log 2 pi
    double* part;        // [2 kBridgeMaxW]
    double* val;         // [BV_COUNT]
    unsigned long long* word;  // [BW_COUNT]
    unsigned long long seed;
    double s1, s2;
    int W1, W2;
};

// evaluates the P rows at theta_dev ([P][D] dense) into lp_dev [P], enqueued on the handle's stream; 0 or a DEMC_* code
using BridgeEval = std::function<int(double* theta_dev, double* lp_dev)>;

// host: what plan_bridge planned, on `stream` (fitplan: the covariance of the D columns of the fit half, planned by the runtime where
// demc_covariance plans its own); 0 or a DEMC_* code with a message
int bridge_run(const HistView& v, const DimTab* tab, const BridgePlan& plan, const CovPlan& fitplan, unsigned long long seed, hipStream_t stream, const BridgeEval& eval,
               double* out, double* prop_out, double* post_out, double* fit_out, std::string& err);

}  // namespace demc
