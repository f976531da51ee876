/* demc_bridge.h -- the marginal likelihood on the device: bridge sampling over the history (Meng and Wong's iteration with a Normal
 * proposal fitted to the draws), next to demc_waic of demc_pointwise.h and demc_loo of demc_loo.h.
 *
 * demc.h is the boundary of the SAMPLER; its functions are counted and pinned, and so are those of the five headers beside it.
 * This header declares one call on the same handle, under the same rules (demc.h: status codes, demc_last_error, no exception
 * crosses, the call runs on the handle's stream and returns after it has drained).
 */
#ifndef DEMC_BRIDGE_H
#define DEMC_BRIDGE_H
#include "demc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The definition is DESIGN.md section 5.10.  The window is history rows [row0,row1), R = row1 - row0 >= 2, chains pooled.  Rows
 * [row0, rmid), rmid = row0 + R / 2 (floor), are the FIT half (N_fit = (rmid - row0) P draws); rows [rmid, row1) are the ESTIMATE
 * half (N1 draws).  Every scalar is taken to the real line by the bounds of demc_set_bounds (none: xi = theta; lower only:
 * xi = log(theta - lo); upper only: xi = log(hi - theta); both: the logit of (theta - lo) / (hi - lo)); logJ = log |d theta / d xi|
 * summed over the scalars.  The proposal g is the Normal with the mean m and the covariance V = L L' (N_fit - 1 divisor) of xi over
 * the fit half.  N2 = n_prop (0: N1) proposal draws xi = m + L z are taken from Philox stream 7 under `seed` (draw j is entity j,
 * its block k gives z_2k, z_2k+1 by Box-Muller).  The log posterior lp of the estimate half and of the proposal draws is evaluated
 * anew by the handle's own evaluate path (what demc_logpost returns), in chunks of P rows; with
 *   l1_i = lp_i + logJ_i - log g(xi_i) (estimate half),   l2_j likewise (proposal draws),   l* = max_i l1_i,   x = l - l*,
 * r_0 = 1 and r_{t+1} = mean_j[1 / (s1 + s2 r_t exp(-x2_j))] / mean_i[1 / (s1 exp(x1_i) + s2 r_t)], s1 = N1 / (N1 + N2), s2 = 1 - s1,
 * runs until |r_{t+1} - r_t| <= 1e-10 |r_{t+1}| or DEMC_BRIDGE_MAX_ITER iterations; logml = log r + l*.  An iterate r_{t+1} that is
 * not finite or not > 0 (0 by underflow where the two densities do not overlap, +Inf, NaN) stops the iteration: n_iter counts that
 * iteration, converged is 0, and logml, the error terms and the last change are NaN, as under n_nonfinite.
 * out[DEMC_BRIDGE_NOUT]:
 *   0 logml          1 re2_prop = var(f1) / mean(f1)^2 / N2      2 re2_post_iid = var(f2) / mean(f2)^2 / N1
 *     (f1_j = 1 / (s1 + s2 r exp(-x2_j)), f2_i = 1 / (s1 exp(x1_i) / r + s2), the variances with the N - 1 divisor: the approximate
 *     relative mean squared error of Fruehwirth-Schnatter with the autocorrelation factor of the draws taken as 1)
 *   3 n_iter         4 converged (1 or 0)     5 N_fit      6 N1      7 N2      8 l_star
 *   9 n_zero_prop = proposal draws with lp = -Inf (they contribute 0)
 *  10 n_nonfinite = NaN or +Inf among l1 and l2: any makes logml, the error terms and the last change NaN, and no iteration runs
 *  11 the last relative change |r_{t+1} - r_t| / |r_{t+1}|
 * prop_out[N2][D + 3], or NULL: theta, lp, logJ, log g of every proposal draw.  post_out[N1][3], or NULL: lp, logJ, log g of the
 * estimate half, draws in (row, slot) order.  fit_out[D + D D], or NULL: m, then L row-major (upper triangle 0).
 * The sums run in an order fixed by the code (no floating-point atomics): two calls with the same arguments give the same bits.
 * Reads the history and the model; like demc_logpost it may change what demc_last_kernels reports, and leaves the state, the
 * history and the addressing of later steps' random numbers as they were.
 * DEMC_EINVAL, in this order: no history on the handle; bad rows or row1 - row0 < 2; no model; out NULL; a sharded handle;
 * n_prop < 0; D above DEMC_BRIDGE_MAX_D; N_fit <= D; N1 or N2 above DEMC_BRIDGE_MAX_DRAWS; then, found while running: a window draw
 * whose xi is not finite (on or outside a finite bound, or a NaN: the message gives the count and the first row, slot, scalar), a
 * non-positive pivot of the Cholesky factorisation of V.  DEMC_EUNSUPPORTED, where "no model" ranks: a simulation likelihood
 * (demc_set_model_sim), whose lp is noise.  Every other model is served. */
#define DEMC_BRIDGE_NOUT 12
#define DEMC_BRIDGE_MAX_D 64           /* the cap of demc_covariance */
#define DEMC_BRIDGE_MAX_DRAWS 4194304  /* 2^22, for each of N1 and N2 */
#define DEMC_BRIDGE_MAX_ITER 1000
int32_t demc_bridge(demc_handle* h, int64_t row0, int64_t row1, int64_t n_prop, uint64_t seed, double* out /*[DEMC_BRIDGE_NOUT]*/,
                    double* prop_out /*[N2][D+3]: theta, lp, logJ, log g; or NULL*/,
                    double* post_out /*[N1][3]: lp, logJ, log g, draws in (row, slot) order; or NULL*/,
                    double* fit_out /*[D + D*D]: m, then L row-major; or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* DEMC_BRIDGE_H */
