// demc_cov.hpp -- posterior covariance and correlation on the device (include/demc_cov.h: demc_covariance; the definition is
// DESIGN.md 5.7): the corrected two-pass form, the rank-N symmetric update X_c^T X_c on v_mfma_f64_16x16x4_f64.  The chains are
// pooled, so no inverse id map is needed and the history is read straight through, once per pass.  Nothing but mean / cov / cor
// goes to the host, and nothing is read back between the passes.
//
// The pool: cell e < N = n P of rows [row0,row1) is hist + (row0 P + e) ld (D parameters, then padding that is never read),
// acc_hist[row0 P + e] (u8) and lp_hist[row0 P + e].  The K <= 64 selected series sit in ceil(K / 16) BLOCKS of 16 columns; cols[]
// (device, padded with -1 to 64) says which series of the Chains value array column k is.
//
// Geometry, the same in both passes: a K-STEP is 4 consecutive cells, and in it lane l of a wave holds column 16 b + (l & 15) of
// cell 4 q + (l >> 4) for every block b -- one double per block.  A CHUNK is kCovChunk = 512 cells = 128 k-steps; wave w of the
// kCovWG / 64 = 8 of a workgroup takes the k-steps w, w + 8, ... of it (16 each).  WORKER b of the W = min(chunks, kCovMaxWorkers)
// workgroups takes the chunks b, b + W, ...: which lane adds which value, and in which order, depends on (N, K) alone.
//   k_cov_mean        per lane the running sum of its columns; the four cells of a k-step by butterfly (xor 16, 32), the waves in
//                     wave order through LDS -> part1[worker][64]
//   k_cov_mean_final  one workgroup, a thread per column: the workers in index order, divided by N -> mhat[64]
//   k_cov_syrk<NB>    NB = ceil(K / 16).  c = x - mhat, 0.0 for a lane past the end of the pool or past column K (masked AFTER
//                     centring: 0 times a NaN column stays out of every other entry because the masked c is a zero, not the x).
//                     Both fragment layouts of the instruction index lane l as (l & 15, l >> 4) -- A[l & 15][l >> 4] and
//                     B[l >> 4][l & 15] -- so the register of block b is the A operand of tiles (b, .) and the B operand of tiles
//                     (., b).  Tiles bi <= bj only: NB (NB + 1) / 2 accumulators of 4 doubles (10 at K = 64).  s_j: VALU adds of
//                     the same registers.  Waves are combined in wave order through LDS -> part2[worker][tiles 256 + NB 16]: a
//                     tile row-major, (row = (lane >> 4) + 4 reg, col = lane & 15), then s.
//   k_cov_final       one workgroup: the workers in index order, S = Q - (s_i s_j) / N, mean / cov / cor, both triangles from the
//                     same S so that the matrices are symmetric to the bit.
// Scratch is bounded by the workers (kCovMaxWorkers (10 256 + 64 + 64) doubles = 11 MB at K = 64), not by the pool.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "demc_postplan.hpp"  // host-only: the kCov* constants, cov_tiles, cov_partial, HistView, CovPlan

namespace demc {

struct CovKParams {
    const double* hist;          // at row row0: [N][ld]
    const unsigned char* acc;    // at row row0: [N]
    const double* lp;            // at row row0: [N]
    long long N;                 // cells of the pool
    int D, ld, K, W;             // W workers
    const int* cols;             // [64] series of column k, -1 beyond K
    double* part1;               // [W][64] column sums of a worker
    double* mhat;                // [64] the first mean
    double* part2;               // [W][cov_partial(NB)]
    double* mean;                // [K]
    double* cov;                 // [K][K]
    double* cor;                 // [K][K]
};

// host: what plan_cov planned for the rows of `v`, on `stream`; 0 or a DEMC_* code with a message
int cov_run(const HistView& v, const CovPlan& plan, hipStream_t stream, double* mean_out, double* cov_out, double* cor_out, std::string& err);

#ifdef DEMC_COV_KERNELS  // (demc_cov.cpp only: the runtime's unit sees the declarations above and no device code)
typedef double cov_d4 __attribute__((ext_vector_type(4)));  // C/D fragment of v_mfma_f64_16x16x4_f64

struct CovSrc {  // where a lane finds its column of block b: x(e) = kind == 2 ? (double)u8[e * ustride] : f64[e * stride]; kind 0: the
    const double* f64;          // column is past K.  Both pointers are always readable (a stride of 0 on the start of lp / acc where
    const unsigned char* u8;    // they are not the source), so the loads of a k-step carry no branch and go out together
    long long stride, ustride;
    int kind;
};

__device__ __forceinline__ CovSrc cov_src(const CovKParams& p, int k) {
    CovSrc s{p.lp, p.acc, 0, 0, 0};
    const int col = p.cols[k];  // (k < 64 always)
    if (col < 0) return s;
    if (col < p.D) { s.f64 = p.hist + col; s.stride = p.ld; s.kind = 1; }
    else if (col == p.D) { s.ustride = 1; s.kind = 2; }
    else { s.stride = 1; s.kind = 1; }
    return s;
}

// the value and whether there is one: false for a column past K or a cell past the pool (the loads then read cell N - 1 or the
// first cell: inside the pool in every case)
__device__ __forceinline__ bool cov_load(const CovSrc& s, long long e, long long N, double& x) {
    const long long ec = e < N ? e : N - 1;
    const double xf = s.f64[(size_t)ec * s.stride];
    const unsigned char xu = s.u8[(size_t)ec * s.ustride];
    x = s.kind == 2 ? (double)xu : xf;
    return s.kind != 0 && e < N;
}

// pass 1: column sums of a worker's chunks
__global__ __launch_bounds__(kCovWG) void k_cov_mean(CovKParams p) {
    __shared__ double w_sum[kCovWG / 64][kCovMaxCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & 15, sub = lane >> 4;
    const int nb = (p.K + 15) >> 4;
    CovSrc src[4];
    double sum[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) { src[b] = cov_src(p, 16 * b + cl); sum[b] = 0.0; }
    const long long chunks = (p.N + kCovChunk - 1) / kCovChunk;
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const long long e0 = ch * kCovChunk;
#pragma unroll 4
        for (int i = 0; i < kCovChunk / 4 / (kCovWG / 64); ++i) {
            const long long e = e0 + (long long)(wave + i * (kCovWG / 64)) * 4 + sub;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (b < nb) {
                    double x;
                    const bool ok = cov_load(src[b], e, p.N, x);
                    sum[b] += ok ? x : 0.0;
                }
        }
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        sum[b] += __shfl_xor(sum[b], 16, 64);
        sum[b] += __shfl_xor(sum[b], 32, 64);
        if (sub == 0) w_sum[wave][16 * b + cl] = sum[b];
    }
    __syncthreads();
    if (threadIdx.x < kCovMaxCols) {
        double t = w_sum[0][threadIdx.x];
        for (int w = 1; w < kCovWG / 64; ++w) t += w_sum[w][threadIdx.x];
        p.part1[(size_t)blockIdx.x * kCovMaxCols + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(kCovMaxCols) void k_cov_mean_final(CovKParams p) {
    const int k = threadIdx.x;
    double t = 0.0;
    if (k < p.K) {
        t = p.part1[k];
        for (int w = 1; w < p.W; ++w) t += p.part1[(size_t)w * kCovMaxCols + k];
        t = t / (double)p.N;
    }
    p.mhat[k] = t;
}

// pass 2: Q and s of a worker's chunks
template <int NB>
__global__ __launch_bounds__(kCovWG) void k_cov_syrk(CovKParams p) {
    constexpr int T = cov_tiles(NB);
    __shared__ double tot[cov_partial(NB)];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), cl = lane & 15, sub = lane >> 4;
    CovSrc src[NB];
    double m[NB], s[NB];
    cov_d4 acc[T];
#pragma unroll
    for (int b = 0; b < NB; ++b) { src[b] = cov_src(p, 16 * b + cl); m[b] = p.mhat[16 * b + cl]; s[b] = 0.0; }
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = cov_d4{0.0, 0.0, 0.0, 0.0};
    const long long chunks = (p.N + kCovChunk - 1) / kCovChunk;
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const long long e0 = ch * kCovChunk;
#pragma unroll 2
        for (int i = 0; i < kCovChunk / 4 / (kCovWG / 64); ++i) {
            const long long q = e0 + (long long)(wave + i * (kCovWG / 64)) * 4;
            if (q >= p.N) break;  // (the whole wave: its later k-steps lie further still)
            double c[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                double x;
                const bool ok = cov_load(src[b], q + sub, p.N, x);
                c[b] = ok ? x - m[b] : 0.0;
                s[b] += c[b];
            }
            int t = 0;
#pragma unroll
            for (int bi = 0; bi < NB; ++bi)
#pragma unroll
                for (int bj = bi; bj < NB; ++bj, ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(c[bi], c[bj], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        s[b] += __shfl_xor(s[b], 16, 64);
        s[b] += __shfl_xor(s[b], 32, 64);
    }
    for (int w = 0; w < kCovWG / 64; ++w) {  // the waves in wave order
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = t * 256 + (sub + 4 * r) * 16 + cl;
                    tot[i] = w == 0 ? acc[t][r] : tot[i] + acc[t][r];
                }
            if (sub == 0) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const int i = T * 256 + 16 * b + cl;
                    tot[i] = w == 0 ? s[b] : tot[i] + s[b];
                }
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < cov_partial(NB); i += kCovWG) p.part2[(size_t)blockIdx.x * cov_partial(NB) + i] = tot[i];
}

// the workers in index order, the correction, the three outputs (-ffp-contract=off: the expressions are the ones written)
__global__ __launch_bounds__(kCovFinalWG) void k_cov_final(CovKParams p) {
    __shared__ double tot[cov_partial(4)];
    __shared__ double S[kCovMaxCols * kCovMaxCols];  // the upper triangle, [i][j] with i <= j
    const int K = p.K, nb = (K + 15) >> 4, T = cov_tiles(nb), len = T * 256 + nb * 16;
    for (int i = threadIdx.x; i < len; i += kCovFinalWG) {
        double t = p.part2[i];
#pragma unroll 8
        for (int w = 1; w < p.W; ++w) t += p.part2[(size_t)w * len + i];
        tot[i] = t;
    }
    __syncthreads();
    const double N = (double)p.N;
    const double* s = tot + T * 256;
    for (int e = threadIdx.x; e < K * K; e += kCovFinalWG) {
        const int i = e / K, j = e - i * K;
        if (i > j) continue;
        const int bi = i >> 4, bj = j >> 4;
        const int t = bi * nb - bi * (bi - 1) / 2 + (bj - bi);  // tiles in the order (0,0) (0,1) .. (0,nb-1) (1,1) ..
        const double Q = tot[t * 256 + (i & 15) * 16 + (j & 15)];
        S[i * kCovMaxCols + j] = Q - (s[i] * s[j]) / N;
    }
    __syncthreads();
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (p.mean)
        for (int j = threadIdx.x; j < K; j += kCovFinalWG) p.mean[j] = p.mhat[j] + s[j] / N;
    for (int e = threadIdx.x; e < K * K; e += kCovFinalWG) {
        const int i = e / K, j = e - i * K, a = i < j ? i : j, b = i < j ? j : i;
        const double Sab = S[a * kCovMaxCols + b], Saa = S[a * kCovMaxCols + a], Sbb = S[b * kCovMaxCols + b];
        if (p.cov) p.cov[e] = p.N == 1 ? nan : Sab / (double)(p.N - 1);
        if (p.cor) {
            double r;
            if (p.N == 1) r = nan;
            else if (a == b) r = (isfinite(Saa) && Saa > 0.0) ? 1.0 : nan;
            else {
                r = Sab / (sqrt(Saa) * sqrt(Sbb));
                r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);  // (a NaN stays one)
            }
            p.cor[e] = r;
        }
    }
}
#endif  // DEMC_COV_KERNELS

}  // namespace demc
