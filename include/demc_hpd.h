/* demc_hpd.h -- highest-density intervals on the device: the entry point of libdemc_hip.so that reads them off the sorted pool.  A
 * header of its own for the reason demc_summary.h gives: the entry points of demc.h and of the other headers are counted.  The same
 * rules hold (demc.h: status codes, demc_last_error, no exception crosses, the call runs on the handle's stream and returns after it
 * has drained).
 */
#ifndef DEMC_HPD_H
#define DEMC_HPD_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MCMCChains' hpd(chains; alpha) with the chains pooled, for history rows [row0,row1), per series of the Chains value array (j < D:
 * parameter j, j = D: acceptance as 0/1, j = D+1: lp) and per alpha; n = row1 - row0 rows, N = n P pooled values.  The definition, to
 * the last operation, is DESIGN.md section 5.12: y[0..N) is the pool sorted by the 64-bit key of section 5.6 (so -0.0 sorts before
 * +0.0); m = max(1, ceil(alpha N)), the product one rounded double multiplication of alpha, as the caller passed it, by (double)N;
 * candidate i in [0, m) is the interval [y[i], y[N - m + i]] of width w_i = y[N - m + i] - y[i], one rounded double subtraction; the
 * answer is the candidate of the smallest width in the order of Julia's findmin -- a NaN width (both ends the same infinity) ranks
 * below every number, other widths compare by value, among equal widths the smallest i wins.  A pool that holds a NaN has NaN in
 * lower, upper and first; m is still reported.  There is no per-chain variant.
 *   out[(j*n_alphas + k)*DEMC_HPD_COLS + (0 lower, 1 upper, 2 first: the 0-based sorted position of lower, 3 m)], j in [0, D + 2)
 * Reads the history only: nothing the sampler reads changes, two calls give the same bits.  Only out reaches the host.
 * DEMC_EINVAL: no history on the handle, bad rows or row1 - row0 < 1, out or alphas NULL, n_alphas outside [1, DEMC_HPD_MAX_ALPHAS],
 * an alpha that is not finite or not strictly inside (0, 1), a sharded handle.
 * DEMC_EUNSUPPORTED: N >= 2^31 (positions are 32-bit). */
#define DEMC_HPD_COLS 4
#define DEMC_HPD_MAX_ALPHAS 16
int32_t demc_hpd(demc_handle* h, int64_t row0, int64_t row1, const double* alphas, int32_t n_alphas, double* out);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_HPD_H */
