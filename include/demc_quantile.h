/* demc_quantile.h -- posterior quantiles on the device: the second table of describe(chains), next to demc_summary.h's first.
 *
 * demc.h is the boundary of the SAMPLER and demc_summary.h declares the summary statistics; the functions of both are counted and
 * pinned.  This header declares the one call that selects order statistics of the history on the same handle, under the same
 * rules (demc.h: status codes, demc_last_error, no exception crosses, the call runs on the handle's stream and returns after it
 * has drained).
 */
#ifndef DEMC_QUANTILE_H
#define DEMC_QUANTILE_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* quantile(chains) without the chains: quantiles of history rows [row0,row1) computed on the device, per series of the Chains
 * value array (j < D: parameter j, j = D: acceptance as 0.0 / 1.0, j = D+1: lp).  The pool of a series is all N = (row1 - row0) P
 * values of those rows, chains appended (the result does not depend on which particle id sits in which slot); padding columns
 * of a history cell are not values.  The definition, to the last operation, is DESIGN.md section 5.6: values are ordered by the
 * key bits(x) ^ (sign ? ~0 : 1 << 63) compared unsigned (IEEE order, -0.0 before +0.0); with x_(1) <= ... <= x_(N),
 * aleph = (double)N p + (1 - p) (a rounded product, then a rounded sum), j = clamp(trunc(aleph), 1, N - 1), g = clamp(aleph - j,
 * 0, 1), a = x_(j), b = x_(j+1): a + g (b - a) when both are finite, else a if g == 0, b if g == 1, (1 - g) a + g b otherwise;
 * x_(1) when N == 1 (Julia's quantile default, type 7).  A series whose pool holds a NaN has NaN for every quantile.
 * The selection is an exact radix select: results are equal to the definition bit for bit.
 *   probs[n_probs]: in [0, 1], in any order, repeats allowed; 1 <= n_probs <= DEMC_QUANTILE_MAX_PROBS
 *   out[j*n_probs + k]: the quantile probs[k] of series j, j < D+2
 * Reads the history only: nothing the sampler reads changes, two calls give the same bits.  Only out reaches the host.
 * DEMC_EINVAL: no history on the handle, bad rows or row1 - row0 < 1, n_probs outside 1 .. 16, a prob outside [0, 1] or NaN, a
 * sharded handle (gather and use the host function). */
#define DEMC_QUANTILE_MAX_PROBS 16
int32_t demc_quantiles(demc_handle* h, int64_t row0, int64_t row1, const double* probs, int32_t n_probs, double* out);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_QUANTILE_H */
