/* demc_cov.h -- posterior covariance and correlation on the device: the joint structure of the posterior, next to the two tables of
 * describe(chains) that demc_summary.h and demc_quantile.h declare.
 *
 * demc.h is the boundary of the SAMPLER; its functions are counted and pinned.  This header declares the one call that forms the
 * covariance and correlation matrices of the history on the same handle, under the same rules (demc.h: status codes,
 * demc_last_error, no exception crosses, the call runs on the handle's stream and returns after it has drained).
 */
#ifndef DEMC_COV_H
#define DEMC_COV_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cov(chains) and cor(chains) without the chains: the sample covariance and correlation of history rows [row0,row1) computed on the
 * device, between series of the Chains value array (j < D: parameter j, j = D: acceptance as 0.0 / 1.0, j = D+1: lp).  The pool of
 * a series is all N = (row1 - row0) P values of those rows, chains appended as cov(Array(chains)) appends them (the result does not
 * depend on which particle id sits in which slot); padding columns of a history cell are not values.  All arithmetic is FP64; the
 * definition is DESIGN.md section 5.7, the corrected two-pass form: with m_j a first mean of series j, c_ej = x_ej - m_j,
 * s_j = sum_e c_ej, Q_ij = sum_e c_ei c_ej and S_ij = Q_ij - (s_i s_j) / N,
 *   mean_j = m_j + s_j / N,  cov_ij = S_ij / (N - 1),  cor_ij = clamp(S_ij / (sqrt(S_ii) sqrt(S_jj)), -1, 1), cor_ii = 1.
 * N = 1: cov and cor are NaN throughout.  A constant series has zeros in its row and column of cov and NaN in its row and column
 * of cor, the diagonal included.  A series whose pool holds a non-finite value has NaN in its row and column of both tables (and a
 * NaN mean); no other entry is touched.  The sums run in an order fixed by the code (no floating-point atomics): two calls give
 * the same bits.  The products are formed by the FP64 matrix instruction of the device.
 *   cols[n_cols]: K = n_cols distinct series, in any order, 1 <= K <= DEMC_COV_MAX_COLS; NULL: all D + 2 series in their order, and
 *                 then n_cols must equal D + 2 (and D + 2 <= DEMC_COV_MAX_COLS)
 *   mean_out[K], cov_out[K*K], cor_out[K*K]: row-major in the order of cols, exactly symmetric (the lower triangle is a copy of the
 *                 upper one); each may be NULL, not all three
 * Reads the history only: nothing the sampler reads changes.  Only the three outputs reach the host.
 * DEMC_EINVAL: no history on the handle, bad rows or row1 - row0 < 1, n_cols outside 1 .. 64, a column outside [0, D+2), a repeated
 * column, every output NULL, a sharded handle (gather and use the host function). */
#define DEMC_COV_MAX_COLS 64
int32_t demc_covariance(demc_handle* h, int64_t row0, int64_t row1, const int32_t* cols, int32_t n_cols,
                        double* mean_out, double* cov_out, double* cor_out);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_COV_H */
