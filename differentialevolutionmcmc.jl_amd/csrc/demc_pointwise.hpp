// demc_pointwise.hpp -- per-observation log-densities and WAIC on the device (include/demc_pointwise.h: demc_pointwise_loglik,
// demc_waic; the definition is DESIGN.md 5.8).  S draws times N observations of density evaluations, with three running reductions
// over the draws for each observation: the OBSERVATION sits on the lane and the DRAW on the wave.  A lane keeps its observation in
// registers for the whole walk; what a draw contributes is wave-uniform and arrives by scalar loads from a dense table of constants;
// the running maximum, sum of exponentials and shifted sums stay in the lane's registers.  No cross-lane reduction in the loop, no
// floating-point atomics anywhere.
//
//   k_pw_prepare            a thread per draw: a history cell (or a row of the caller's theta) -> the K constants of the draw,
//                           cst[S][K] (pw_constants of demc_pwplan.hpp says what they are), so that log sigma or the LBA's
//                           normalisation are formed once per draw, not once per wave.  cst[s][K - 1] is the draw's flag: 1.0
//                           when the row holds a NaN or (demc_pointwise_loglik) lies outside the bounds -- every term is NaN then.
//   k_pw_accumulate<F, X>   grid = (observation tiles of kPwWG, draw chunks).  Each lane walks its chunk's draws once: the online
//                           maximum M with the rescaled E = sum exp(l - M) over the draws that are neither -Inf nor NaN, and
//                           a1 = sum (l - l0), a2 = sum (l - l0)^2 shifted by the chunk's first term l0.  One partial per
//                           (chunk, i): M, E, mean = l0 + a1 / n, M2 = a2 - a1^2 / n, flags (1: a term was -Inf or NaN, 2: NaN).
//   k_pw_final              a thread per observation: the chunks in index order (a fixed left-leaning tree) -- M = max M_c,
//                           E = sum E_c exp(M_c - M); mean and M2 by the pairwise rule of Chan et al. -- then the four values of
//                           the observation, written through the LBA's permutation into the caller's order.
//   k_pw_totals             one workgroup over the N x 4 table in the caller's order: thread t adds rows t, t + 1024, ... and the
//                           threads combine by a halving tree in LDS; var_i(elpd_i) in a second pass about the mean of the first.
//   k_pw_matrix<F, X>       the accumulate kernel's term written out instead of reduced: out[s][i], caller's order.
// X: the accumulators of the LBA (2, 3; 0: read at run time), the padded row length of a whitened MvNormal row (8, 16, 32, 64).
// The terms are formed by the helpers of demc_device.hpp (lba_trial, log_Phi_neg_table) and the expressions of obs_range_sum /
// lnr_range_sum on the same constants, under -ffp-contract=off: a term here and in demc_pointwise_loglik are the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "demc_dimtab.hpp"  // DimTab: the bounds in force
#include "demc_pwplan.hpp"  // host-only: the kPw* constants, PwFamily, PwPlan, HistView

namespace demc {

struct PwKParams {
    // the model
    int fam;                  // PwFamily
    int n_acc, d, dp;
    long long N;
    const double* data;       // family specific, as the likelihood kernels read it
    const double* data2;
    const double* M;          // MVN_FULL: (L^-1)' [d][d]
    const double* xbar;       // MVN: [d]
    double c0;                // LNR: sigma; MVN_FULL: -(d log 2 pi + log det Sigma) / 2
    const int* order;         // LBA: the caller's index of sorted trial k; null: the identity
    // the draws
    const double* theta;      // [S] rows, ld doubles apart, D values each
    long long S, ld;
    int D, K;
    const DimTab* bounds;     // [D], null: the rows are evaluated as stored
    long long chunk_len;
    int chunks;
    // scratch and results
    double* cst;              // [S][K]
    double* part;             // [chunks][kPwPartial][N]
    double* point;            // [N][4], caller's order
    double* total;            // [8]
    double* matrix;           // [S][N], caller's order
};

// what the handle lends a run: the model on the device
struct PwModelView {
    PwModel m;
    const double* data;
    const double* data2;
    const double* M;
    const double* xbar;
    double c0;
    const int* order;
};

// host: what plan_pointwise planned, on `stream`; 0 or a DEMC_* code with a message
int pw_waic_run(const PwModelView& mv, const HistView& v, const PwPlan& plan, hipStream_t stream, double* total_out, double* point_out, std::string& err);
int pw_matrix_run(const PwModelView& mv, const double* theta_host, int D, const DimTab* bounds_dev, const PwPlan& plan, hipStream_t stream,
                  double* out, std::string& err);

}  // namespace demc
