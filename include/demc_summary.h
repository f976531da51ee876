/* demc_summary.h -- chain summaries on the device: the one entry point of libdemc_hip.so that is declared outside demc.h.
 *
 * demc.h is the boundary of the SAMPLER: its entry points are counted, mirrored one for one by every binding, and that count is
 * pinned.  This header is the boundary of what follows a run -- describe(chains), the call every example and every statistical
 * gate of the reference ends with -- on the same handle, under the same rules (demc.h: status codes, demc_last_error, no
 * exception crosses, the call runs on the handle's stream and returns after it has drained).
 */
#ifndef DEMC_SUMMARY_H
#define DEMC_SUMMARY_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* describe(chains) without the chains: summary statistics of history rows [row0,row1) computed on the device, per series of the
 * Chains value array (j < D: parameter j, j = D: acceptance as 0/1, j = D+1: lp), chain c = particle id c (re-keyed as
 * demc_export_chains does), n = row1 - row0 rows, h = n / 2 (integer), m = P chains, M = 2m split chains.  The definition, to
 * the last operation, is DESIGN.md section 5.5: mean and std (ddof 1) over all n m values; split-R-hat; the effective sample
 * size from Geyer's initial monotone sequence over rho_t (split chains, no rank normalisation), max_lag > 0 capping the lags at
 * min(h - 1, max_lag), 0: all h - 1; mcse = std / sqrt(ess); pairs = the number K of pairs P_k = rho_2k + rho_2k+1 kept.  The
 * sequence was cut by the cap (or the end of the half) rather than by a negative pair exactly when K == (L + 1) / 2, L the last
 * lag.  rhat is NaN when h < 2 or W == 0, ess and mcse when h < 4 or W == 0 (pairs is 0 then).
 *   out[j*DEMC_SUMMARY_COLS + (0 mean, 1 std, 2 rhat, 3 ess, 4 mcse, 5 pairs)]
 *   rho_out: NULL, or [D+2][rho_len] receiving rho_0 .. rho_{rho_len-1}.  Lags are evaluated in blocks of 64 and a series stops
 *   at the block in which its sequence ends: entries beyond the last lag the call evaluated for the series are NaN.
 * Reads the history only: nothing the sampler reads changes, two calls give the same bits.  Only out and rho_out reach the host.
 * DEMC_EINVAL: no history on the handle, bad rows or row1 - row0 < 1, a sharded handle (ids must be local). */
#define DEMC_SUMMARY_COLS 6
int32_t demc_summarize(demc_handle* h, int64_t row0, int64_t row1, int32_t max_lag, double* out, double* rho_out,
                       int64_t rho_len);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_SUMMARY_H */
