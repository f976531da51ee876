/* demc_rank.h -- rank-normalised chain diagnostics on the device: the two entry points of libdemc_hip.so that rank the pooled
 * history.  A header of its own for the reason demc_summary.h gives: the entry points of demc.h and of the other headers are
 * counted.  The same rules hold (demc.h: status codes, demc_last_error, no exception crosses, the call runs on the handle's stream
 * and returns after it has drained).
 */
#ifndef DEMC_RANK_H
#define DEMC_RANK_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ess_bulk, ess_tail and the rank-normalised rhat of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) for history rows
 * [row0,row1), per series of the Chains value array (j < D: parameter j, j = D: acceptance as 0/1, j = D+1: lp), chain c = particle
 * id c, n = row1 - row0 rows, N = n P pooled values.  The definition, to the last operation, is DESIGN.md section 5.11: values are
 * ordered by the 64-bit key of section 5.6 (so -0.0 < +0.0, and two values tie exactly when their keys are equal); r = L + (E + 1) / 2
 * is the average rank (L keys below, E keys equal, itself included); z = Phi^-1((r - 3/8) / (N + 1/4)) with Wichura's AS 241
 * (PPND16); rhat_bulk and ess_bulk are section 5.5's rhat and ess of z (split halves, Geyer's sequence, max_lag and the NaN rules
 * unchanged); rhat_folded is the rhat of the normal scores of |x - med|, med the section 5.6 quantile at 0.5; rhat is the larger of
 * the two; ess_q05 and ess_q95 are the ess of the indicators x <= q05 and x <= q95 (section 5.6 quantiles), ess_tail the smaller;
 * distinct counts the distinct keys of the pool.  A pool that holds a NaN has NaN in every column; a NaN among |x - med| (an
 * infinite median) makes rhat_folded and rhat NaN only.  No antithetic tail term (as section 5.5); quantiles are type 7.
 *   out[j*DEMC_RANK_COLS + (0 rhat, 1 ess_bulk, 2 ess_tail, 3 rhat_bulk, 4 rhat_folded, 5 ess_q05, 6 ess_q95, 7 distinct)]
 * Reads the history only: nothing the sampler reads changes, two calls give the same bits.  Only out reaches the host.
 * DEMC_EINVAL: no history on the handle, bad rows or row1 - row0 < 1, a sharded handle, out NULL, max_lag < 0.
 * DEMC_EUNSUPPORTED: N >= 2^31 (positions are 32-bit). */
#define DEMC_RANK_COLS 8
int32_t demc_rankstats(demc_handle* h, int64_t row0, int64_t row1, int32_t max_lag, double* out);

/* One series of the same pool, slot-keyed as the history is: out[n][P], out[i*P + slot] belongs to the value of row row0 + i in
 * slot `slot`.  kind DEMC_RANK_KIND_RANK: the average ranks r; DEMC_RANK_KIND_SCORE: the normal scores z; DEMC_RANK_KIND_FOLDED:
 * the average ranks of |x - med|.  What a rank plot needs (per-chain rank histograms) at 1 / (D + 2) of an export.  Ranks are by
 * key whatever the pool holds: a NaN has a key beyond the infinities and is ranked there.
 * DEMC_EINVAL: as above, and series outside [0, D + 2) or kind outside 0 .. 2.  DEMC_EUNSUPPORTED: N >= 2^31. */
#define DEMC_RANK_KIND_RANK 0
#define DEMC_RANK_KIND_SCORE 1
#define DEMC_RANK_KIND_FOLDED 2
int32_t demc_rank_series(demc_handle* h, int64_t row0, int64_t row1, int32_t series, int32_t kind, double* out);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_RANK_H */
