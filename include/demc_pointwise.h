/* demc_pointwise.h -- model comparison on the device: the log-density of every observation under given parameter rows, and WAIC
 * over the history, next to the posterior tables that demc_summary.h, demc_quantile.h and demc_cov.h declare.
 *
 * demc.h is the boundary of the SAMPLER; its functions are counted and pinned.  This header declares the two calls that answer
 * per OBSERVATION on the same handle, under the same rules (demc.h: status codes, demc_last_error, no exception crosses, the call
 * runs on the handle's stream and returns after it has drained).
 */
#ifndef DEMC_POINTWISE_H
#define DEMC_POINTWISE_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The definition is DESIGN.md section 5.8.  l_is = log p(y_i | theta_s) is the family's own term of observation i under draw s:
 * its sum over i is the log-likelihood demc_logpost adds the prior to.  All arithmetic is FP64.
 *
 * Families served: DEMC_FAM_GAUSSIAN, DEMC_FAM_BINOMIAL, DEMC_FAM_LNR and DEMC_FAM_LBA in any likelihood mode (an observation is a
 * data point, a (n, k) pair, a trial); DEMC_FAM_MVN_ISO and DEMC_FAM_MVN_FULL when the handle was created with
 * loglike_mode = DEMC_LOGLIKE_DIRECT (an observation is a data row).  DEMC_EUNSUPPORTED: the MvNormal families in the other two
 * modes, the hierarchical families, DEMC_FAM_RASTRIGIN, DEMC_FAM_ODE_LV, a simulation likelihood, a hiprtc plug-in.
 * Observations are numbered as the caller passed them to demc_set_model (the library sorts the trials of an LBA for its own
 * kernels; both calls answer in the caller's order). */

/* out[s][i] = l_is for the n rows theta[n][D] (host).  A row outside the bounds in force (demc_set_bounds), or with a NaN in it,
 * gives a row of NaN.  n N may not exceed DEMC_PW_MAX_CELLS (the matrix is staged on the device: 1 GiB).
 * DEMC_EINVAL: no model or a model without observations (the race models accept dims = [0, n_acc]), n < 1, n N above the cap. */
#define DEMC_PW_MAX_CELLS 134217728 /* 2^27 */
int32_t demc_pointwise_loglik(demc_handle* h, const double* theta /*[n][D] host*/, int64_t n,
                              double* out /*[n][N] host, caller's observation order*/);

/* WAIC of history rows [row0,row1).  The draws are all S = (row1 - row0) P cells of the window, chains pooled as demc_quantiles and
 * demc_covariance pool them, evaluated as stored (no bounds are applied; a cell with a NaN in it gives NaN terms); padding columns
 * of a history cell are not values.  With M_i = max_s l_is:
 *   lppd_i   = M_i + log(sum_s exp(l_is - M_i)) - log S
 *   mean_i   = (sum_s l_is) / S
 *   p_waic_i = sum_s (l_is - mean_i)^2 / (S - 1)          (S = 1: NaN)
 *   elpd_i   = lppd_i - p_waic_i
 * pointwise_out[i] = (lppd_i, p_waic_i, mean_i, elpd_i), or NULL.  total_out[DEMC_WAIC_NTOTAL], or NULL:
 *   0 elpd_waic = sum_i elpd_i       1 se_elpd = sqrt(N var_i(elpd_i)) (N - 1 in the variance; N = 1: NaN)
 *   2 p_waic = sum_i p_waic_i        3 lppd = sum_i lppd_i       4 waic = -2 elpd_waic       5 dbar = -2 sum_i mean_i
 *   6 n_high = observations with p_waic_i > 0.4       7 n_nonfinite = observations whose lppd_i or p_waic_i is not finite
 * Non-finite terms: an observation with l_is = -Inf in some draws has a finite lppd_i if any draw is finite (every draw -Inf:
 * lppd_i = -Inf) and NaN mean_i and p_waic_i; a NaN l_is makes all four NaN.  Totals follow by ordinary arithmetic: nothing is
 * dropped, n_nonfinite counts what was affected.  The sums run in an order fixed by the code (no floating-point atomics): two
 * calls give the same bits.  Reads the history and the model only: nothing the sampler reads changes.
 * DEMC_EINVAL, in this order: no history on the handle, bad rows or row1 - row0 < 1, no model or a model without observations, both
 * outputs NULL, a sharded handle. */
#define DEMC_WAIC_NTOTAL 8
#define DEMC_WAIC_NPOINT 4 /* lppd_i, p_waic_i, mean_i, elpd_i */
int32_t demc_waic(demc_handle* h, int64_t row0, int64_t row1, double* total_out /*[8]*/, double* pointwise_out /*[N][4] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_POINTWISE_H */
