/* demc_loo.h -- PSIS-LOO on the device: Pareto-smoothed importance-sampling leave-one-out cross-validation over the history, with
 * the per-observation diagnostic khat, next to demc_waic of demc_pointwise.h.
 *
 * demc.h is the boundary of the SAMPLER; its functions are counted and pinned, and so are those of the four headers beside it.
 * This header declares one call on the same handle, under the same rules (demc.h: status codes, demc_last_error, no exception
 * crosses, the call runs on the handle's stream and returns after it has drained).
 */
#ifndef DEMC_LOO_H
#define DEMC_LOO_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The definition is DESIGN.md section 5.9; l_is = log p(y_i | theta_s) is the term of section 5.8 (demc_pointwise.h).  Families,
 * draws and observation order are demc_waic's: DEMC_FAM_GAUSSIAN, DEMC_FAM_BINOMIAL, DEMC_FAM_LNR and DEMC_FAM_LBA in any likelihood
 * mode, DEMC_FAM_MVN_ISO and DEMC_FAM_MVN_FULL with loglike_mode = DEMC_LOGLIKE_DIRECT; the draws are all S = (row1 - row0) P cells
 * of history rows [row0,row1), chains pooled, evaluated as stored; rows are answered in the caller's observation order.  All
 * arithmetic is FP64.
 *
 * For observation i the log ratios are -l_is.  The M = ceil(min(S / 5, 3 sqrt(S))) smallest terms form the tail (selected exactly;
 * ties at the cutoff and ratios below DBL_MIN times the largest stay outside), a generalised Pareto distribution is fitted to it by
 * the profile method of Zhang and Stephens, the tail's weights are replaced by the fitted quantiles, and
 *   elpd_loo_i = log(sum_s w_s exp(l_is)) - log(sum_s w_s).
 * pointwise_out[i] = (elpd_loo_i, p_loo_i = lppd_i - elpd_loo_i, khat_i, lppd_i, n_tail_i, l_cut_i), or NULL: khat_i is the fitted
 * shape (+Inf where no tail was fitted: S <= 20, five or fewer distinct tail terms), n_tail_i the terms that were smoothed, l_cut_i
 * the (M + 1)-th smallest term.  total_out[DEMC_LOO_NTOTAL], or NULL:
 *   0 elpd_loo = sum_i elpd_loo_i    1 se_elpd = sqrt(N var_i(elpd_loo_i)) (N - 1 in the variance; N = 1: NaN)
 *   2 p_loo = sum_i p_loo_i          3 lppd = sum_i lppd_i         4 looic = -2 elpd_loo
 *   5 n_k_high = observations with khat_i > 0.7 (+Inf counted)     6 n_k_bad = observations with khat_i > 1
 *   7 n_nonfinite = observations whose elpd_loo_i or lppd_i is not finite
 * Non-finite terms: a NaN (or +Inf) l_is makes all six values of the observation NaN; otherwise a -Inf l_is gives elpd_loo_i = -Inf,
 * khat_i = +Inf, n_tail_i = 0, l_cut_i = -Inf.  Nothing is dropped from the totals.  The sums run in an order fixed by the code (no
 * floating-point atomics): two calls give the same bits.  Reads the history and the model only.
 * DEMC_EINVAL, in this order: no history on the handle, bad rows or row1 - row0 < 1, no model or a model without observations, both
 * outputs NULL, a sharded handle, S above DEMC_LOO_MAX_DRAWS (pass a narrower window).  DEMC_EUNSUPPORTED: as demc_waic. */
#define DEMC_LOO_NTOTAL 8
#define DEMC_LOO_NPOINT 6 /* elpd_loo_i, p_loo_i, khat_i, lppd_i, n_tail_i, l_cut_i */
#define DEMC_LOO_MAX_DRAWS 4194304 /* 2^22: a tail of at most 6144 terms */
int32_t demc_loo(demc_handle* h, int64_t row0, int64_t row1, double* total_out /*[8] or NULL*/,
                 double* pointwise_out /*[N][6] or NULL, caller's observation order*/);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_LOO_H */
