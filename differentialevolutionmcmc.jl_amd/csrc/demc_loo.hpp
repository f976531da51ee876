// demc_loo.hpp -- PSIS-LOO on the device (include/demc_loo.h: demc_loo; the definition is DESIGN.md 5.9).  The N observations are
// cut into blocks of Nb columns whose terms fit the 1 GiB staging budget; per block:
//
//   k_loo_prepare           a thread per draw, once per call: pw_prepare_draw of demc_pwterm.hpp, cst[S][K].
//   k_loo_terms<F, X>       grid = (tiles of kLooObs observations, draw chunks).  The observation sits on the lane as in k_pw_matrix;
//                           the four waves of a workgroup take four draws each of a tile of kLooTile, the 64 x 16 terms go through
//                           LDS and leave as whole 128-byte lines of the COLUMN-major block terms[Nb][S]: the draws of one
//                           observation are contiguous.  pw_term is the text demc_pointwise_loglik runs: the same bits.
//   k_loo_column            one workgroup of kLooWG threads per observation, four to nine reads of its column:
//                           (1) min and max key, flags, and lppd_i by an online log-sum-exp per thread, combined by a halving tree;
//                           (2) an MSD radix select of the (M + 1)-th smallest key, 11 bits a digit, the histogram in LDS (integer
//                           LDS atomics); a digit on which min and max agree costs no read, and the select stops as soon as the
//                           keys up to the chosen bin fit the kLooCap keys of LDS;
//                           (3) one read that compacts those keys into LDS and adds everything else to the two non-tail sums
//                           (thread t takes draws t, t + 512, ...; the threads combine by a halving tree);
//                           (4) a bitonic sort of the compacted keys -- their order no longer depends on which thread came first --,
//                           the cutoff, the floor and the tail; (5) the profile fit, the m points dealt over the eight waves, each
//                           wave summing log1p over the tail lane-strided and then by a butterfly; (6) the smoothed weights, the two
//                           log-sum-exps and the row of six, written through the LBA's permutation.
//   k_loo_totals            one workgroup over the N x 6 table in the caller's order, as k_pw_totals.
// No floating-point atomics anywhere, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "demc_looplan.hpp"    // host-only: the kLoo* constants, LooPlan
#include "demc_pointwise.hpp"  // PwKParams, PwModelView, HistView

namespace demc {

// host: what plan_loo planned, on `stream`; 0 or a DEMC_* code with a message
int loo_run(const PwModelView& mv, const HistView& v, const LooPlan& plan, hipStream_t stream, double* total_out, double* point_out, std::string& err);

}  // namespace demc
