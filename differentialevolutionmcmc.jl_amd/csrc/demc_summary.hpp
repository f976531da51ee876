// demc_summary.hpp -- chain summaries on the device (include/demc_summary.h: demc_summarize; the definition is DESIGN.md 5.5): mean, std,
// split-R-hat, effective sample size by Geyer's initial monotone sequence, its Monte-Carlo standard error and the autocorrelation,
// of every series of the Chains value array (D parameters, acceptance, lp), straight from the slot-keyed history.  Nothing but the
// (D+2) x 6 results (and the autocorrelations, when asked for) goes to the host.
//
// Chain c is particle id c: the history is keyed by slot, so one pass over id_hist builds the inverse map inv[row][id] = slot
// (k_sum_invmap, 32-bit entries) and every later kernel GATHERS a chain through it -- no re-keyed copy of theta.  History cells are
// hist_ld doubles apart (padded when partners are gathered from the history), not D.
//
// Geometry of the three gathering kernels (k_sum_moments, k_sum_acf): grid (chain workers, series tiles), 256 threads.  A workgroup
// takes the chains c = blockIdx.x, blockIdx.x + gridDim.x, ... one after the other and a tile of JT consecutive series; it stages
// the n rows of its chain for those series in LDS (x[jl][i], i fastest), works on them, and ADDS the chain's contribution to
// accumulators of its own, which it writes once at its end: partial[worker][series](...).  Scratch is therefore bounded by the
// number of workers (kSumMaxWorkers), not by the population.  A series too long for LDS (n > kSumLdsRows) is staged in a global
// tile of the worker instead (template argument LDS = false): the same code on a pointer into another address space.
//
// Autocovariances come in BLOCKS of kSumLagBlock = 64 lags: a wave's lanes are the lags t0 .. t0+63 of one (series, half), the
// lane's loop runs over i with x[i] a broadcast read and x[i+t] consecutive addresses (conflict-free).  After every block
// k_sum_geyer -- one workgroup per series -- adds the workers' partials in worker order, turns them into rho_t and advances
// Geyer's sequence over the block's 32 pairs; a series whose sequence has ended is flagged and the next block's workgroups skip it
// (a workgroup whose whole tile has ended leaves before it gathers anything).  The work is proportional to the autocorrelation
// time, and which pairs enter tau is exactly what the all-lags definition gives: pairs never straddle a block, and a block is
// only started for a series that has not stopped.
//
// Every sum has a fixed order: lanes stride over rows and are combined by a butterfly of shuffles, chains are added in the order a
// worker visits them, workers in index order, threads by a tree in LDS.  No floating-point atomics: two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "demc_postplan.hpp"  // host-only: the kSum* constants, HistView, SummaryPlan

namespace demc {

struct SumKParams {
    const double* hist;          // [n_rows][P][ld]
    const unsigned char* acc;    // [n_rows][P]
    const double* lp;            // [n_rows][P]
    const int* idh;              // [n_rows][P]
    long long P, row0, n, h, id0;
    int D, ld, JT, L;            // L: the last lag that may be evaluated
    int* inv;                    // [n][P] slot of id (row-local)
    double* xg;                  // LDS = false: [D+2][workers][n] staging tiles (JT = 1)
    double* mu;                  // [D+2][2P] mean of split chain 2c + s
    double* part_sum;            // [workers][D+2] sum of the worker's chains (all n rows)
    double* part_ss;             // [workers][D+2] centred squares around mean[j]
    double* part_g;              // [workers][D+2][64] sum over the worker's split chains of gamma_s(t0 + lane)
    double* mean;                // [D+2]
    double* bh;                  // [D+2] B / h
    double* W;                   // [D+2]
    double* vplus;               // [D+2]
    double* p_prev;              // [D+2] Geyer: the last (monotone) pair
    double* p_sum;               // [D+2] ... the sum of the pairs kept
    int* K;                      // [D+2] ... their number
    int* stopped;                // [D+2] 0: running, 1: ended, 2: ended on a NaN pair (ess is NaN)
    double* rho;                 // [D+2][rho_cols] or null
    long long rho_cols;
    double* out;                 // [D+2][6]
};

// host: what plan_summary planned for the rows of `v`, on `stream`; 0 or a DEMC_* code with a message
int summary_run(const HistView& v, const SummaryPlan& plan, hipStream_t stream, double* out, double* rho_out, long long rho_len, std::string& err);
// host: the launches of summary_run without its end, for a caller that reads the table on the device (demc_rankstats): on return
// `p` names the buffers, p.out the table [D+2][6]; they live in `s`, and nothing has been waited for.  `who` names the call in `err`.
struct Scratch;
int summary_enqueue(const char* who, const HistView& v, const SummaryPlan& plan, hipStream_t stream, Scratch& s, SumKParams& p, std::string& err);

#ifdef DEMC_SUMMARY_KERNELS  // (demc_summary.cpp only: the runtime's unit sees the declarations above and no device code)
// ---- one pass over id_hist: inv[i][id - id0] = slot
__global__ __launch_bounds__(256) void k_sum_invmap(SumKParams p) {
    const long long total = p.n * p.P;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t / p.P, slot = t - i * p.P;
        const long long id = (long long)p.idh[(size_t)(p.row0 + i) * p.P + slot] - p.id0;
        if (id >= 0 && id < p.P) p.inv[(size_t)i * p.P + id] = (int)slot;
    }
}

__device__ __forceinline__ double sum_wave(double v) {  // butterfly: every lane ends with the same bits
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// rows [0, n) of chain c for the series j0 .. j0+JT-1 -> x[jl * n + i]
__device__ __forceinline__ void sum_gather(const SumKParams& p, long long c, int j0, int jt, const int* skip, double* x) {
    const long long total = p.n * jt;
    for (long long t = threadIdx.x; t < total; t += kSumWG) {
        const long long i = t / jt;
        const int jl = (int)(t - i * jt), j = j0 + jl;
        if (skip && skip[j]) continue;
        const size_t hrow = (size_t)(p.row0 + i) * p.P + (size_t)p.inv[(size_t)i * p.P + c];
        x[(size_t)jl * p.n + i] = j < p.D ? p.hist[hrow * p.ld + j] : (j == p.D ? (double)p.acc[hrow] : p.lp[hrow]);
    }
}

// MODE 0: the sums of a chain and the means of its two halves.  MODE 1: squared deviations from the mean over all chains.
template <bool LDS, int MODE>
__global__ __launch_bounds__(kSumWG) void k_sum_moments(SumKParams p) {
    extern __shared__ __align__(16) double sum_lds[];
    double* x = LDS ? sum_lds : p.xg + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * p.n;
    const int D2 = p.D + 2, j0 = blockIdx.y * p.JT, jt = min(p.JT, D2 - j0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double wacc[2] = {0.0, 0.0};  // this wave's series jl = wave, wave + 4 (JT <= kSumMaxJT)
    for (long long c = blockIdx.x; c < p.P; c += gridDim.x) {
        sum_gather(p, c, j0, jt, nullptr, x);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int jl = wave + 4 * q;
            if (jl >= jt) continue;
            const double* xs = x + (size_t)jl * p.n;
            if (MODE == 0) {
                double s0 = 0.0, s1 = 0.0;
                for (long long i = lane; i < p.h; i += 64) { s0 += xs[i]; s1 += xs[p.h + i]; }
                s0 = sum_wave(s0); s1 = sum_wave(s1);
                double tot = s0 + s1;
                if (p.n > 2 * p.h) tot += xs[2 * p.h];
                wacc[q] += tot;
                if (lane == 0) {
                    p.mu[(size_t)(j0 + jl) * 2 * p.P + 2 * c] = s0 / (double)p.h;
                    p.mu[(size_t)(j0 + jl) * 2 * p.P + 2 * c + 1] = s1 / (double)p.h;
                }
            } else {
                const double m = p.mean[j0 + jl];
                double s = 0.0;
                for (long long i = lane; i < p.n; i += 64) { const double d = xs[i] - m; s = fma(d, d, s); }
                wacc[q] += sum_wave(s);
            }
        }
        __syncthreads();
    }
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (wave + 4 * q < jt) (MODE == 0 ? p.part_sum : p.part_ss)[(size_t)blockIdx.x * D2 + j0 + wave + 4 * q] = wacc[q];
}

__device__ __forceinline__ double sum_block(double v, double* sh) {  // 256 threads, tree in LDS; everyone gets the total
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// one workgroup per series: the mean over all values; B / h = var of the split-chain means (ddof 1, centred)
__global__ __launch_bounds__(256) void k_sum_means(SumKParams p, int workers) {
    __shared__ double sh[256];
    const int j = blockIdx.x, D2 = p.D + 2;
    double s = 0.0;
    for (int w = threadIdx.x; w < workers; w += 256) s += p.part_sum[(size_t)w * D2 + j];
    s = sum_block(s, sh);
    const long long M = 2 * p.P;
    const double* mu = p.mu + (size_t)j * M;
    double a = 0.0;
    for (long long k = threadIdx.x; k < M; k += 256) a += mu[k];
    const double mbar = sum_block(a, sh) / (double)M;
    double b = 0.0;
    for (long long k = threadIdx.x; k < M; k += 256) { const double d = mu[k] - mbar; b = fma(d, d, b); }
    b = sum_block(b, sh);
    if (threadIdx.x == 0) {
        p.mean[j] = s / ((double)p.n * (double)p.P);
        p.bh[j] = b / (double)(M - 1);
    }
}

// lags t0 .. t0+63 of every running series: part_g[worker][j][lane] = sum over the worker's split chains of gamma_s(t0 + lane)
template <bool LDS>
__global__ __launch_bounds__(kSumWG) void k_sum_acf(SumKParams p, int t0) {
    extern __shared__ __align__(16) double sum_lds[];
    const int D2 = p.D + 2, j0 = blockIdx.y * p.JT, jt = min(p.JT, D2 - j0);
    bool any = false;
    for (int jl = 0; jl < jt; ++jl) any = any || p.stopped[j0 + jl] == 0;
    if (!any) return;  // (uniform over the workgroup)
    double* gacc = sum_lds;                               // [2 JT][64]
    double* x = LDS ? sum_lds + 2 * p.JT * kSumLagBlock : p.xg + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * p.n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = threadIdx.x; t < 2 * jt * kSumLagBlock; t += kSumWG) gacc[t] = 0.0;
    const long long h = p.h;
    const int t = t0 + lane;
    const long long cnt = t <= p.L ? h - t : 0;  // (L <= h - 1)
    for (long long c = blockIdx.x; c < p.P; c += gridDim.x) {
        sum_gather(p, c, j0, jt, p.stopped, x);
        __syncthreads();
        for (long long u = threadIdx.x; u < 2 * h * jt; u += kSumWG) {  // centre each half on its own mean
            const int jl = (int)(u / (2 * h));
            const long long i = u - (long long)jl * 2 * h;
            if (p.stopped[j0 + jl]) continue;
            x[(size_t)jl * p.n + i] -= p.mu[(size_t)(j0 + jl) * 2 * p.P + 2 * c + (i >= h ? 1 : 0)];
        }
        __syncthreads();
        for (int item = wave; item < 2 * jt; item += 4) {  // (series, half): a wave each, its lanes the lags
            const int jl = item >> 1, s = item & 1;
            if (p.stopped[j0 + jl]) continue;
            const double* ys = x + (size_t)jl * p.n + (size_t)s * h;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            long long i = 0;
            for (; i + 3 < cnt; i += 4) {
                a0 = fma(ys[i], ys[i + t], a0);
                a1 = fma(ys[i + 1], ys[i + 1 + t], a1);
                a2 = fma(ys[i + 2], ys[i + 2 + t], a2);
                a3 = fma(ys[i + 3], ys[i + 3 + t], a3);
            }
            for (; i < cnt; ++i) a0 = fma(ys[i], ys[i + t], a0);
            gacc[item * kSumLagBlock + lane] += ((a0 + a1) + (a2 + a3)) / (double)h;  // (only this wave touches the row)
        }
        __syncthreads();
    }
    for (int u = threadIdx.x; u < jt * kSumLagBlock; u += kSumWG) {
        const int jl = u >> 6, l = u & 63;
        p.part_g[((size_t)blockIdx.x * D2 + j0 + jl) * kSumLagBlock + l] = gacc[(2 * jl) * kSumLagBlock + l] + gacc[(2 * jl + 1) * kSumLagBlock + l];
    }
}

// one workgroup (a wave) per series: the workers' partials of the block -> rho_t -> Geyer's sequence over the block's pairs
__global__ __launch_bounds__(64) void k_sum_geyer(SumKParams p, int t0, int workers) {
    __shared__ double rho[kSumLagBlock];
    const int j = blockIdx.x, D2 = p.D + 2, lane = threadIdx.x;
    if (p.stopped[j]) return;
    double g = 0.0;
    for (int w = 0; w < workers; ++w) g += p.part_g[((size_t)w * D2 + j) * kSumLagBlock + lane];
    g /= (double)(2 * p.P);  // mean over the split chains
    const double hd = (double)p.h;
    double W, vp;
    if (t0 == 0) {
        W = __shfl(g, 0, 64) * hd / (hd - 1.0);
        vp = W * (hd - 1.0) / hd + p.bh[j];
        if (lane == 0) { p.W[j] = W; p.vplus[j] = vp; }
    } else {
        W = p.W[j]; vp = p.vplus[j];
    }
    const int t = t0 + lane;
    const double r = t == 0 ? 1.0 : 1.0 - (W - g) / vp;
    rho[lane] = r;
    if (p.rho && t <= p.L && t < p.rho_cols) p.rho[(size_t)j * p.rho_cols + t] = r;
    __syncthreads();
    if (lane != 0) return;
    if (t0 == 0 && (p.h < 4 || W == 0.0)) {  // ess is NaN by definition: no pair is looked at
        p.stopped[j] = 2;
        return;
    }
    int K = p.K[j], stop = 0;
    double prev = p.p_prev[j], sum = p.p_sum[j];
    for (int k = 0; k < kSumLagBlock / 2; ++k) {
        if (t0 + 2 * k + 1 > p.L) { stop = 1; break; }  // the lag cap (or the end of the half) cut the sequence
        double P = rho[2 * k] + rho[2 * k + 1];
        if (!(P >= 0.0)) { stop = P < 0.0 ? 1 : 2; break; }  // the first negative pair is excluded; a NaN pair ends it too
        if (K > 0) P = fmin(P, prev);
        sum += P;
        prev = P;
        ++K;
    }
    p.K[j] = K; p.p_prev[j] = prev; p.p_sum[j] = sum;
    if (stop) p.stopped[j] = stop;
}

// one thread per series: out[j] = (mean, std, rhat, ess, mcse, pairs)
__global__ __launch_bounds__(64) void k_sum_final(SumKParams p, int workers) {
    const int j = blockIdx.x * 64 + threadIdx.x, D2 = p.D + 2;
    if (j >= D2) return;
    double ss = 0.0;
    for (int w = 0; w < workers; ++w) ss += p.part_ss[(size_t)w * D2 + j];
    const double nm = (double)p.n * (double)p.P, Mh = (double)(2 * p.P) * (double)p.h;
    const double sd = sqrt(ss / (nm - 1.0));
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double W = p.W[j];
    double rhat = nan, ess = nan;
    if (p.h >= 2 && W != 0.0) rhat = sqrt(p.vplus[j] / W);
    if (p.h >= 4 && W != 0.0 && p.stopped[j] != 2) {
        double tau = -1.0 + 2.0 * p.p_sum[j];
        tau = fmax(tau, 1.0 / log10(Mh));
        ess = Mh / tau;
    }
    double* o = p.out + (size_t)j * 6;
    o[0] = p.mean[j]; o[1] = sd; o[2] = rhat; o[3] = ess; o[4] = sd / sqrt(ess); o[5] = (double)p.K[j];
}
#endif  // DEMC_SUMMARY_KERNELS

}  // namespace demc
