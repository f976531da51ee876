// demc_rank.hpp -- rank-normalised chain diagnostics on the device (include/demc_rank.h: demc_rankstats, demc_rank_series; the
// definition is DESIGN.md 5.11): an exact rank of every draw in the pooled history -- a full LSD radix sort of (key, position)
// pairs with tie handling -- then the normal scores, the two tail indicators and the folded series, laid out as a history of their
// own on which demc_summarize's kernels (demc_summary.hpp, unchanged) form R-hat and ESS.  Only the (D+2) x 8 table reaches the host.
//
// Per batch of series (demc_rankplan.hpp says how many fit the scratch budget), blockIdx.y the series of the batch:
//   k_rank_keys     reads the slot-keyed history straight through -- consecutive lanes on consecutive doubles, padded columns
//                   skipped, then acc_hist and lp_hist -- and writes key and 32-bit pool position t = i P + slot.
//   k_rank_range    OR and AND of a series' keys (a wave's by shuffles, then one integer atomic each: order cannot matter) and the
//                   NaN flag.  A digit in which OR and AND agree is shared by the whole pool: its pass is skipped, by every
//                   kernel alike, and which of the two buffers holds the pairs before digit d follows from the same two words.
//   per digit d, least significant first:
//   k_rank_hist     one wave per tile of kRankTile pairs: the tile's 256 counts in LDS (integer atomics), written to hist[d][tile].
//   k_rank_scan     one workgroup per series: exclusive prefix sum over (digit, tile), digit-major, in index order.
//   k_rank_scatter  one wave per tile, 32 rounds of 64 pairs in position order: the lanes that share a digit find one another by
//                   eight ballots, a lane's offset is the tile's running count of its digit plus the number of such lanes below
//                   it.  Stable within a round, across rounds, across tiles: the order of equal keys never depends on timing.
//   k_rank_ties     for each sorted position the first and last position of its run of equal keys (its neighbours say whether
//                   it is alone; if not, two binary searches in the sorted keys -- runs may span any number of tiles), r = L + (E + 1) / 2
//                   to the draw's own position; the number of run heads is `distinct`; three lanes read med, q05 and q95 off
//                   the sorted keys by section 5.6's arithmetic.
//   k_rank_derive   z = ppnd16((r - 3/8) / (N + 1/4)), x <= q05, x <= q95, zeta = |x - med| into the derived history
//                   der[t][4 b + (0 .. 3)]; a second keys / sort / ties round on zeta and k_rank_score replace zeta by z'.
//   summary_enqueue (demc_summary.cpp) on a HistView of der: the tested kernels of section 5.5.
//   k_rank_final    gathers the eight columns of every series of the batch.
// No floating-point atomics, no scratch memory; two calls give the same bits.
//
// demc_hpd (include/demc_hpd.h; the definition is DESIGN.md 5.12) is the same sort -- keys, range, then hist / scan / scatter per
// digit, the positions riding along unused -- followed by:
//   k_hpd_window    blockIdx.y the series of the batch, blockIdx.z the alpha, lanes on consecutive candidates i < m: y[i] and
//                   y[N - m + i] from the buffer rank_src(diff, kRankPasses) names (which of the two it is depends on how many
//                   passes ran), one subtraction, the running best as (width, i) under findmin's order -- NaN first, then by
//                   value, then the smaller i --, reduced over the wave by shuffles and over the workgroup through LDS: one
//                   partial per workgroup.  Beyond kHpdMaxBlocks workgroups a thread strides.
//   k_hpd_final     one wave per (series, alpha): the partials in index order, the NaN flag of the pool, keys back to values,
//                   the four columns.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "demc_hpdplan.hpp"   // host-only: the kHpd* constants, HpdPlan, HpdGrid
#include "demc_postplan.hpp"  // HistView, SummaryPlan
#include "demc_rankplan.hpp"  // host-only: the kRank* constants, RankPlan, RankTargets

namespace demc {

// host: what plan_rank planned for the rows of `v`, on `stream`; `full` and `last` are the summary plans of a derived history of a
// whole batch and of the last one.  series < 0: the table of demc_rankstats into out[D+2][8]; otherwise demc_rank_series: `kind`
// of that one series into out[n][P].  0 or a DEMC_* code with a message.
int rank_run(const HistView& v, const RankPlan& plan, const SummaryPlan& full, const SummaryPlan& last, int series, int kind, hipStream_t stream,
             double* out, std::string& err);

// host: what plan_hpd planned for the rows of `v`, on `stream`: the table of demc_hpd into out[D+2][n_alphas][4].  0 or a DEMC_* code
// with a message.
int hpd_run(const HistView& v, const HpdPlan& plan, hipStream_t stream, double* out, std::string& err);

}  // namespace demc
