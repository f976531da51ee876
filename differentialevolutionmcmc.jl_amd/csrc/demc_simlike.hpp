// demc_simlike.hpp -- simulation-based likelihoods: k_sim_loglike<SIM, EST>, the likelihood kernel (K2 slot) of models that hand the
// library a SIMULATOR instead of a density (include/demc.h: demc_set_model_sim).
//
// The reference runs such models with closures around KernelDensity.jl / a counting loop (Examples/KDE_Example.jl: per proposal
// 10 000 draws of Normal(mu, sigma), an Epanechnikov kernel density estimate, sum_j log max(1e-10, pdf(kde, x_j));
// Examples/Binomial_ABC.jl:21: 10 000 Binomial(N, theta) counts, log(#{sim == k} / n_sim)).  Here, per proposal row theta at
// address (iter, sweep, entity):
//   1. the simulated sample s_0 .. s_{n-1} from the Philox stream S_SIM = 7, draw_block(seed, S_SIM, sweep, iter, entity, block)
//      (demc_device.hpp), entity = the GLOBAL slot (group_offset + g) Np + p, so a shard draws what the single handle draws:
//        SIM_NORMAL   theta = (mu, sigma): block b gives z[4b .. 4b+3] = box_muller(x, y).{x, y}, box_muller(z, w).{x, y};
//                     s_i = mu + sigma z_i
//        SIM_BINOMIAL theta = p, n_trials = hyper: count i uses the blocks [i B, (i+1) B), B = ceil(n_trials / 4); trial t
//                     (word t of those blocks, x y z w in order) succeeds when u32unit(word) < p
//        SIM_USER     one call of the user's demc_user_sim per value; its generator hands out the words of the blocks
//                     (i << 8) | k, k = 0, 1, ... (mod 256), in order
//   2. the estimator over the scalar observations x_0 .. x_{N-1}:
//        EST_KDE   f(x) = 1/(n h) sum_i 3/4 max(0, 1 - ((x - s_i)/h)^2), loglike = sum_j log max(1e-10, f(x_j));
//                  h = the caller's bandwidth when > 0, else 0.9 sd n^(-1/5) with sd the two-pass sample standard deviation
//                  (n - 1); sd == 0 there makes the row -Inf
//        EST_FREQ  loglike = sum_j log(c_j / n), c_j = #{s_i == x_j}; c_j = 0 gives -Inf.  The n + 1 possible values of
//                  log(c / n) come from a table the host fills with its libm at demc_set_model_sim (one division, one log
//                  each): the kernel's part is integer counting, so the result is the same bits on every device and host.
//      A non-finite simulated value makes the row -Inf (never a NaN into the accept step).
//   3. PAIRS (k_sim_choice<SIM>, estimator EST_KDE_CHOICE): a simulated value is (c_i, t_i), a choice in [0, 255] and a response
//      time; an observation is (c_j, x_j), c_j >= 1 (obs = the N choices, then the N times: the layout of FAM_LBA / FAM_LNR).
//        SIM_LNR      theta = (nu[0 .. K-1], tau), K = D - 1 in [2, 8], hyper = [sigma]: value i uses the blocks [i B, (i+1) B),
//                     B = ceil(K / 4); accumulator k takes normal k of those blocks (box_muller(x, y).{x, y}, box_muller(z, w)
//                     .{x, y} per block); T_k = exp(nu_k + sigma z_k), c_i = 1 + argmin_k T_k (ties to the lower k),
//                     t_i = tau + min_k T_k
//        SIM_USER     one call of the user's demc_user_sim_choice per value (same generator, same block addressing); a choice
//                     outside [0, 255] makes the row -Inf
//        EST_KDE_CHOICE  the DEFECTIVE density of choice c, f(c, x) = 1/(n h_c) sum_{i: c_i = c} 3/4 max(0, 1 - ((x - t_i)/h_c)^2),
//                     loglike = sum_j log max(1e-10, f(c_j, x_j)): the normaliser is n, ALL simulated values, so f(c, .)
//                     integrates to n_c / n.  Choice 0 = no response: it counts towards n and belongs to no density; its t is
//                     ignored (not checked).  h_c = the caller's bandwidth when > 0 (the same for every choice), else
//                     0.9 sd_c n_c^(-1/5), sd_c the two-pass standard deviation (n_c - 1) of the t_i of choice c and
//                     n_c^(-1/5) ONE pow(n_c, -0.2) PER CHOICE IN THE KERNEL (no host table).  A choice without an estimate --
//                     n_c < 2 or sd_c == 0 under the rule of thumb, n_c == 0 under a fixed bandwidth -- gives f = 0: each of
//                     its observations contributes exactly log(1e-10) and the row stays finite.  A non-finite t_i with
//                     c_i >= 1 makes the row -Inf.
//      The kernel has a symbol of its own, k_sim_choice, beside k_sim_loglike; its instances are listed in
//      DEMC_SIM_CHOICE_INSTANCES and land in the same table (demc_instances.hpp: kSim, key <SIM, EST_KDE_CHOICE>).
// Two deviations from KernelDensity.jl as it is recalled (not pinned to a version, like StatsBase's samplers elsewhere in this
// library): the density is SUMMED EXACTLY, not binned on a 2048-point grid and interpolated; and the bandwidth rule drops the
// min(sd, IQR / 1.34) of Silverman's rule (a quantile of 10^4 values per proposal for a factor that is 1.007 on Normal data).
//
// Geometry: one 256-thread workgroup per proposal; the sample lives in LDS (n <= kSimMaxN = 16 384 doubles = 128 KB of the
// 150 KB a launch may ask for; 10 000 values = 80 KB: two workgroups per CU).  Pass 1: lane t draws the blocks t, t + 256, ...
// (Normal: four values a block) and writes the values; the moments are per-lane sums in index order, a __shfl_xor tree per wave,
// the four waves left to right.  Pass 2: observations in tiles of four, tile T on wave T mod 4; the wave's lanes stride over the
// sample (lane l reads s_l, s_{l+64}, ...: consecutive doubles, no bank conflict; each value read once for the four
// observations), tree, one log per observation on the wave's lanes alike; a wave adds its observations in index order and the
// four waves are combined (w0 + w1) + (w2 + w3).  Every sum therefore runs in an order fixed by (n, N) alone -- not by the grid,
// the shard, or what else is resident: same seed, same bits.
// Pairs keep this geometry.  LDS: the n times (double), the n choices (one byte each, behind the times, padded to 8 bytes), then
// kSimChoiceTabBytes of per-choice tables (four wave partials, 1/h_c and 3/4 / (n h_c) for the 256 choices): 9 n + 16 KB.
// 16 384 values would need 160 KB, more than a launch may ask for, so this estimator has its own cap kSimChoiceMaxN = 15 000
// (148 KB; 10 000 values = 104 KB).  Pass 1: lane t simulates the values t, t + 256, ...; per choice c = 1 .. k_max (the largest
// OBSERVED choice, from the host: no other density is read) the count and the sum, then the sum of squared deviations, are
// per-lane accumulators over the lane's values in index order, a wave tree, the four waves left to right.  Pass 2: the same
// tiles; each observation of a tile carries its own 1/h_c and the inner term is masked by c_i == c_j.  Every sum's order is
// fixed by (n, N, k_max) alone.
//
// ONE copy of the kernel text serves the library's instances (demc_simlike.cpp) and the user-simulator instance: the build embeds
// this file as a string (csrc/Makefile: demc_simlike_src.inc) and demc_set_model_sim hands it to hiprtc with DEMC_SIM_JIT
// defined, the user's source in front of the kernel.  Under DEMC_SIM_JIT the few helpers it needs from demc_device.hpp /
// demc_kernels.hpp (Philox4x32-10, draw_block, u32unit, box_muller) are restated below, since those headers pull in the host's
// <cmath> and the tables; tests/test_gpu_simlike.py compares the JIT instance with the same restatement as the built-in ones.
#pragma once
#ifndef DEMC_SIM_JIT
#include "demc_kernels.hpp"
#else
#ifndef INFINITY
#define INFINITY __builtin_huge_val()
#endif
#ifndef NAN
#define NAN __builtin_nan("")
#endif
namespace demc {
struct U4 {
    unsigned x, y, z, w;
};
__device__ inline U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (unsigned)(p1 >> 32) ^ c.y ^ k0;
        n.y = (unsigned)p1;
        n.z = (unsigned)(p0 >> 32) ^ c.w ^ k1;
        n.w = (unsigned)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
__device__ inline U4 draw_block(unsigned long long seed, unsigned stream, unsigned sweep, unsigned long long iter, unsigned entity, unsigned block) {
    U4 c;
    c.x = block;
    c.y = entity;
    c.z = (unsigned)iter;
    c.w = (stream << 24) | (sweep & 0xFFFFu);
    return philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
}
__device__ inline double u32unit(unsigned w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }
__device__ inline double2 box_muller(unsigned w0, unsigned w1) {
    const double rad = sqrt(-2.0 * log(1.0 - u32unit(w0)));
    double sn, cs;
    sincospi(2.0 * u32unit(w1), &sn, &cs);
    return make_double2(rad * cs, rad * sn);
}
}  // namespace demc
#endif

namespace demc {

constexpr unsigned S_SIM = 7;  // the Philox stream of the simulated samples (next to S_STEP .. S_MIG = 1 .. 6, demc_device.hpp)
constexpr int FAM_SIM = 101;   // internal family id of a handle whose model was set by demc_set_model_sim
constexpr int kSimMaxN = 16384;
constexpr int kSimChoiceMaxN = 15000;  // EST_KDE_CHOICE: 9 bytes a value and the per-choice tables under the LDS of a launch
// per-choice tables of k_sim_choice: [256][4] wave partials (double), [256] 1/h_c, [256] 3/4 / (n h_c), [256][4] wave counts (int)
constexpr int kSimChoiceTabBytes = 256 * (4 * 8 + 8 + 8 + 4 * 4);
enum SimKind : int { SIM_NORMAL = 0, SIM_BINOMIAL = 1, SIM_LNR = 2, SIM_USER = 100 };
enum SimEst : int { EST_KDE = 0, EST_FREQ = 1, EST_KDE_CHOICE = 2 };
// bytes of LDS k_sim_choice asks for at n simulated values
constexpr size_t sim_choice_lds(int n) { return (size_t)n * 8 + (size_t)((n + 7) / 8) * 8 + kSimChoiceTabBytes; }

// kernarg of k_sim_loglike (the JIT instance reads the same struct)
struct SimKParams {
    int n_groups, Np, D, a_lo, n_act, group_offset;
    int n_sim, nhyper;          // nhyper: the simulator's own hyper-parameters (behind the bandwidth)
    int k_max, pad_;            // EST_KDE_CHOICE: the largest observed choice
    long long n_obs, iter;
    unsigned long long seed;
    unsigned sweep, entity_base;  // entity = entity_base + (group_offset + g) Np + p
    double bandwidth;           // > 0: the KDE's h; else the rule of thumb
    double n_pow;               // n^(-1/5), from the host
    const double* prop;         // [P][D]
    double* partial;            // [P]
    const double* obs;          // [n_obs]; EST_KDE_CHOICE: [2 n_obs], the choices, then the times
    const double* hyper;        // [nhyper]
    const double* logtab;       // [n_sim + 1] log(c / n), EST_FREQ
    const int* glist;
};

// generator handed to a user simulator: value i reads the words of the blocks (i << 8) | k, k = 0, 1, ... in order
struct SimRng {
    unsigned long long seed, iter;
    unsigned sweep, entity, i, k, w;
    U4 cur;
};

}  // namespace demc

typedef demc::SimRng demc_sim_rng;
__device__ inline unsigned demc_sim_u32(demc_sim_rng* r) {
    if (r->w == 4) {
        r->cur = demc::draw_block(r->seed, demc::S_SIM, r->sweep, r->iter, r->entity, (r->i << 8) | (r->k & 255u));
        r->k += 1;
        r->w = 0;
    }
    const unsigned v = r->w == 0 ? r->cur.x : r->w == 1 ? r->cur.y : r->w == 2 ? r->cur.z : r->cur.w;
    r->w += 1;
    return v;
}
// uniform in (0, 1) from one word; a standard normal from two (Box-Muller's cosine branch)
__device__ inline double demc_sim_uniform(demc_sim_rng* r) { return demc::u32unit(demc_sim_u32(r)); }
__device__ inline double demc_sim_normal(demc_sim_rng* r) {
    const unsigned a = demc_sim_u32(r);
    const unsigned b = demc_sim_u32(r);
    return demc::box_muller(a, b).x;
}
#ifdef DEMC_SIM_JIT
#if DEMC_SIM_JIT_EST == 2  // (EST_KDE_CHOICE: the user's simulator returns t and sets *choice)
#define DEMC_SIM_JIT_CHOICE 1
__device__ double demc_user_sim_choice(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng, int* choice);
#else
__device__ double demc_user_sim(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng);
#endif
#define DEMC_SIM_KERNEL_HEAD extern "C" __global__ __launch_bounds__(256) void k_sim_loglike_user(demc::SimKParams p)
#define DEMC_SIM_CHOICE_KERNEL_HEAD DEMC_SIM_KERNEL_HEAD
#else
#define DEMC_SIM_KERNEL_HEAD template <int SIM, int EST> __global__ __launch_bounds__(256) void k_sim_loglike(SimKParams p)
#define DEMC_SIM_CHOICE_KERNEL_HEAD template <int SIM> __global__ __launch_bounds__(256) void k_sim_choice(SimKParams p)
#endif

#ifndef DEMC_SIM_JIT
namespace demc {
#else
using namespace demc;
constexpr int SIM = SIM_USER;
constexpr int EST = DEMC_SIM_JIT_EST;
#endif

#ifndef DEMC_SIM_JIT_CHOICE
DEMC_SIM_KERNEL_HEAD {
#ifdef DEMC_SIM_JIT
    __shared__ double s_smp[DEMC_SIM_JIT_N];  // (n is known when the source is compiled)
#else
    extern __shared__ double s_smp[];
#endif
    __shared__ double s_part[4];
    __shared__ int s_bad[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const int gq = q / p.n_act, pl = p.a_lo + (q - gq * p.n_act);
    const int g = p.glist ? p.glist[gq] : gq;
    const size_t slot = (size_t)g * p.Np + pl;
    const unsigned entity = p.entity_base + (unsigned)(p.group_offset + g) * (unsigned)p.Np + (unsigned)pl;
    const double* th = p.prop + slot * p.D;
    const int n = p.n_sim;

    // ---- pass 1: the sample, and its sum (per lane in index order; wave tree; waves left to right) ----
    double lsum = 0.0;
    int bad = 0;
    if (SIM == SIM_NORMAL) {
        const double mu = th[0], sg = th[1];
        for (int b = tid; 4 * b < n; b += 256) {
            const U4 r = draw_block(p.seed, S_SIM, p.sweep, (unsigned long long)p.iter, entity, (unsigned)b);
            const double2 za = box_muller(r.x, r.y), zb = box_muller(r.z, r.w);
            const double z[4] = {za.x, za.y, zb.x, zb.y};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * b + e < n) {
                    const double s = mu + sg * z[e];
                    s_smp[4 * b + e] = s;
                    lsum += s;
                    bad |= !(fabs(s) < INFINITY);
                }
        }
    } else if (SIM == SIM_BINOMIAL) {
        const double pr = th[0];
        const int n_trials = (int)p.hyper[0], B = (n_trials + 3) / 4;
        for (int i = tid; i < n; i += 256) {
            int c = 0;
            for (int b = 0; b < B; ++b) {
                const U4 r = draw_block(p.seed, S_SIM, p.sweep, (unsigned long long)p.iter, entity, (unsigned)(i * B + b));
                c += (4 * b + 0 < n_trials && u32unit(r.x) < pr) + (4 * b + 1 < n_trials && u32unit(r.y) < pr) +
                     (4 * b + 2 < n_trials && u32unit(r.z) < pr) + (4 * b + 3 < n_trials && u32unit(r.w) < pr);
            }
            const double s = (double)c;
            s_smp[i] = s;
            lsum += s;
        }
        bad |= !(pr == pr);
    } else {
#ifdef DEMC_SIM_JIT
        SimRng rng;
        rng.seed = p.seed; rng.iter = (unsigned long long)p.iter; rng.sweep = p.sweep; rng.entity = entity;
        for (int i = tid; i < n; i += 256) {
            rng.i = (unsigned)i; rng.k = 0; rng.w = 4;
            const double s = demc_user_sim(th, p.D, p.hyper, p.nhyper, &rng);
            s_smp[i] = s;
            lsum += s;
            bad |= !(fabs(s) < INFINITY);
        }
#endif
    }
    double inv_h = 0.0, scale = 0.0;
    if (EST == EST_KDE) {
        double h = p.bandwidth;
        if (!(h > 0.0)) {  // two-pass standard deviation (n - 1)
            for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o);
            if (lane == 0) s_part[wave] = lsum;
            __syncthreads();
            const double mean = (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) / (double)n;
            __syncthreads();
            double lss = 0.0;
            if (SIM == SIM_NORMAL) {  // (the lane's own values, in the order it wrote them)
                for (int b = tid; 4 * b < n; b += 256)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * b + e < n) {
                            const double dlt = s_smp[4 * b + e] - mean;
                            lss += dlt * dlt;
                        }
            } else {
                for (int i = tid; i < n; i += 256) {
                    const double dlt = s_smp[i] - mean;
                    lss += dlt * dlt;
                }
            }
            for (int o = 32; o > 0; o >>= 1) lss += __shfl_xor(lss, o);
            if (lane == 0) s_part[wave] = lss;
            __syncthreads();
            const double sd = sqrt((((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) / (double)(n - 1));
            h = (0.9 * sd) * p.n_pow;
            bad |= !(sd > 0.0);  // sd == 0 (or NaN): no density estimate
        }
        inv_h = 1.0 / h;
        scale = 0.75 / ((double)n * h);
    }
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();  // (also: the sample is complete, and s_part is free again)
    bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];

    // ---- pass 2: observations in tiles of four, tile T on wave T mod 4 ----
    double wsum = 0.0;
    const long long N = p.n_obs;
    if (!bad) {
        for (long long j0 = 4LL * wave; j0 < N; j0 += 16) {
            const double x0 = p.obs[j0], x1 = j0 + 1 < N ? p.obs[j0 + 1] : x0, x2 = j0 + 2 < N ? p.obs[j0 + 2] : x0,
                         x3 = j0 + 3 < N ? p.obs[j0 + 3] : x0;
            if (EST == EST_KDE) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                for (int i = lane; i < n; i += 64) {
                    const double s = s_smp[i];
                    const double u0 = (x0 - s) * inv_h, u1 = (x1 - s) * inv_h, u2 = (x2 - s) * inv_h, u3 = (x3 - s) * inv_h;
                    a0 += fmax(0.0, fma(-u0, u0, 1.0));
                    a1 += fmax(0.0, fma(-u1, u1, 1.0));
                    a2 += fmax(0.0, fma(-u2, u2, 1.0));
                    a3 += fmax(0.0, fma(-u3, u3, 1.0));
                }
                for (int o = 32; o > 0; o >>= 1) {
                    a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
                }
                // (lane e takes observation e of the tile: one log instruction stream for the four)
                const double a = (lane & 3) == 0 ? a0 : (lane & 3) == 1 ? a1 : (lane & 3) == 2 ? a2 : a3;
                const double t = log(fmax(1e-10, scale * a));
                const double t0 = __shfl(t, 0), t1 = __shfl(t, 1), t2 = __shfl(t, 2), t3 = __shfl(t, 3);
                wsum += t0;
                if (j0 + 1 < N) wsum += t1;
                if (j0 + 2 < N) wsum += t2;
                if (j0 + 3 < N) wsum += t3;
            } else {
                int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
                for (int i = lane; i < n; i += 64) {
                    const double s = s_smp[i];
                    c0 += s == x0; c1 += s == x1; c2 += s == x2; c3 += s == x3;
                }
                for (int o = 32; o > 0; o >>= 1) {
                    c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); c3 += __shfl_xor(c3, o);
                }
                wsum += p.logtab[c0];
                if (j0 + 1 < N) wsum += p.logtab[c1];
                if (j0 + 2 < N) wsum += p.logtab[c2];
                if (j0 + 3 < N) wsum += p.logtab[c3];
            }
        }
    }
    if (lane == 0) s_part[wave] = wsum;
    __syncthreads();
    if (tid == 0) p.partial[slot] = bad ? -INFINITY : (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

#endif  // !DEMC_SIM_JIT_CHOICE

#if !defined(DEMC_SIM_JIT) || defined(DEMC_SIM_JIT_CHOICE)
// ---- pairs (choice, response time) under the per-choice defective KDE (the file's head, 3.) ----
DEMC_SIM_CHOICE_KERNEL_HEAD {
#ifdef DEMC_SIM_JIT
    __shared__ double s_smp[(9 * DEMC_SIM_JIT_N + 7) / 8 + 8 + kSimChoiceTabBytes / 8];  // (>= sim_choice_lds(n) bytes)
#else
    extern __shared__ double s_smp[];
#endif
    __shared__ double s_part[4];
    __shared__ int s_bad[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const int gq = q / p.n_act, pl = p.a_lo + (q - gq * p.n_act);
    const int g = p.glist ? p.glist[gq] : gq;
    const size_t slot = (size_t)g * p.Np + pl;
    const unsigned entity = p.entity_base + (unsigned)(p.group_offset + g) * (unsigned)p.Np + (unsigned)pl;
    const double* th = p.prop + slot * p.D;
    const int n = p.n_sim;
    unsigned char* s_ch = (unsigned char*)(s_smp + n);                      // [n] choices, padded to 8 bytes
    double* s_tsum = (double*)(s_ch + (size_t)((n + 7) / 8) * 8);           // [256][4] wave partials: sums, then squared deviations
    double* s_invh = s_tsum + 256 * 4;                                      // [256] 1 / h_c (0: no estimate)
    double* s_scale = s_invh + 256;                                         // [256] 3/4 / (n h_c) (0: no estimate)
    int* s_tcnt = (int*)(s_scale + 256);                                    // [256][4] wave counts
    const int k_max = p.k_max;

    // ---- pass 1: the sample ----
    int bad = 0;
#ifndef DEMC_SIM_JIT
    if (SIM == SIM_LNR) {
        const int K = p.D - 1, B = (K + 3) / 4;
        double nu[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) nu[k] = k < K ? th[k] : 0.0;
        const double tau = th[K], sg = p.hyper[0];
        for (int i = tid; i < n; i += 256) {
            double best = 0.0;
            int arg = 0;
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (b < B) {
                    const U4 r = draw_block(p.seed, S_SIM, p.sweep, (unsigned long long)p.iter, entity, (unsigned)(i * B + b));
                    const double2 za = box_muller(r.x, r.y), zb = box_muller(r.z, r.w);
                    const double z[4] = {za.x, za.y, zb.x, zb.y};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * b + e < K) {
                            const double T = exp(nu[4 * b + e] + sg * z[e]);
                            if (4 * b + e == 0 || T < best) {  // (strict: ties go to the lower k)
                                best = T;
                                arg = 4 * b + e;
                            }
                        }
                }
            const double t = tau + best;
            s_smp[i] = t;
            s_ch[i] = (unsigned char)(arg + 1);
            bad |= !(fabs(t) < INFINITY);
        }
    }
#else
    {
        SimRng rng;
        rng.seed = p.seed; rng.iter = (unsigned long long)p.iter; rng.sweep = p.sweep; rng.entity = entity;
        for (int i = tid; i < n; i += 256) {
            rng.i = (unsigned)i; rng.k = 0; rng.w = 4;
            int c = 0;
            const double t = demc_user_sim_choice(th, p.D, p.hyper, p.nhyper, &rng, &c);
            s_smp[i] = t;
            s_ch[i] = (unsigned char)c;
            bad |= (c < 0) | (c > 255) | ((c >= 1) & !(fabs(t) < INFINITY));
        }
    }
#endif
    // ---- per-choice bandwidths.  Each lane reads back only the values it wrote: no barrier before the moments ----
    if (!(p.bandwidth > 0.0)) {
        for (int c = 1; c <= k_max; ++c) {  // counts and sums
            int lc = 0;
            double ls = 0.0;
            for (int i = tid; i < n; i += 256)
                if (s_ch[i] == c) {
                    lc += 1;
                    ls += s_smp[i];
                }
            for (int o = 32; o > 0; o >>= 1) {
                lc += __shfl_xor(lc, o);
                ls += __shfl_xor(ls, o);
            }
            if (lane == 0) {
                s_tcnt[4 * c + wave] = lc;
                s_tsum[4 * c + wave] = ls;
            }
        }
        __syncthreads();
        double lss_own = 0.0;  // (what this thread publishes below: thread c owns choice c)
        int n_own = 0;
        for (int c = 1; c <= k_max; ++c) {  // squared deviations from the choice's mean
            const int nc = ((s_tcnt[4 * c] + s_tcnt[4 * c + 1]) + s_tcnt[4 * c + 2]) + s_tcnt[4 * c + 3];
            const double mean = (((s_tsum[4 * c] + s_tsum[4 * c + 1]) + s_tsum[4 * c + 2]) + s_tsum[4 * c + 3]) / (double)nc;
            double lss = 0.0;
            for (int i = tid; i < n; i += 256)
                if (s_ch[i] == c) {
                    const double dlt = s_smp[i] - mean;
                    lss += dlt * dlt;
                }
            for (int o = 32; o > 0; o >>= 1) lss += __shfl_xor(lss, o);
            if (lane == 0) s_part[wave] = lss;
            __syncthreads();
            if (tid == c) {
                lss_own = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
                n_own = nc;
            }
            __syncthreads();
        }
        if (tid >= 1 && tid <= k_max) {
            double ih = 0.0, sc = 0.0;
            if (n_own >= 2) {
                const double sd = sqrt(lss_own / (double)(n_own - 1));
                if (sd > 0.0 && sd < INFINITY) {
                    const double h = (0.9 * sd) * pow((double)n_own, -0.2);
                    ih = 1.0 / h;
                    sc = 0.75 / ((double)n * h);
                }
            }
            s_invh[tid] = ih;
            s_scale[tid] = sc;
        }
    } else if (tid >= 1 && tid <= k_max) {
        s_invh[tid] = 1.0 / p.bandwidth;
        s_scale[tid] = 0.75 / ((double)n * p.bandwidth);
    }
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o);
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();  // (also: the sample and the tables are complete, and s_part is free again)
    bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];

    // ---- pass 2: observations in tiles of four, tile T on wave T mod 4 ----
    double wsum = 0.0;
    const long long N = p.n_obs;
    if (!bad) {
        for (long long j0 = 4LL * wave; j0 < N; j0 += 16) {
            const long long j1 = j0 + 1 < N ? j0 + 1 : j0, j2 = j0 + 2 < N ? j0 + 2 : j0, j3 = j0 + 3 < N ? j0 + 3 : j0;
            const int k0 = (int)p.obs[j0], k1 = (int)p.obs[j1], k2 = (int)p.obs[j2], k3 = (int)p.obs[j3];  // (in [1, k_max]: the host checked)
            const double x0 = p.obs[N + j0], x1 = p.obs[N + j1], x2 = p.obs[N + j2], x3 = p.obs[N + j3];
            const double h0 = s_invh[k0], h1 = s_invh[k1], h2 = s_invh[k2], h3 = s_invh[k3];
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int i = lane; i < n; i += 64) {
                const double s = s_smp[i];
                const int c = s_ch[i];
                const double u0 = (x0 - s) * h0, u1 = (x1 - s) * h1, u2 = (x2 - s) * h2, u3 = (x3 - s) * h3;
                a0 += c == k0 ? fmax(0.0, fma(-u0, u0, 1.0)) : 0.0;
                a1 += c == k1 ? fmax(0.0, fma(-u1, u1, 1.0)) : 0.0;
                a2 += c == k2 ? fmax(0.0, fma(-u2, u2, 1.0)) : 0.0;
                a3 += c == k3 ? fmax(0.0, fma(-u3, u3, 1.0)) : 0.0;
            }
            for (int o = 32; o > 0; o >>= 1) {
                a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
            }
            const double a = (lane & 3) == 0 ? a0 : (lane & 3) == 1 ? a1 : (lane & 3) == 2 ? a2 : a3;
            const double sc = s_scale[(lane & 3) == 0 ? k0 : (lane & 3) == 1 ? k1 : (lane & 3) == 2 ? k2 : k3];
            const double t = log(fmax(1e-10, sc * a));
            const double t0 = __shfl(t, 0), t1 = __shfl(t, 1), t2 = __shfl(t, 2), t3 = __shfl(t, 3);
            wsum += t0;
            if (j0 + 1 < N) wsum += t1;
            if (j0 + 2 < N) wsum += t2;
            if (j0 + 3 < N) wsum += t3;
        }
    }
    if (lane == 0) s_part[wave] = wsum;
    __syncthreads();
    if (tid == 0) p.partial[slot] = bad ? -INFINITY : (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}
#endif

#ifndef DEMC_SIM_JIT
#define DEMC_SIM_INSTANCES(X) X(SIM_NORMAL, EST_KDE) X(SIM_NORMAL, EST_FREQ) X(SIM_BINOMIAL, EST_KDE) X(SIM_BINOMIAL, EST_FREQ)
#define DEMC_SIM_CHOICE_INSTANCES(X) X(SIM_LNR)  // k_sim_choice<SIM>: the registered pair simulators (estimator EST_KDE_CHOICE)
#ifdef DEMC_SIMLIKE_EXTERN
#define DEMC_X_(...) extern template __global__ void k_sim_loglike<__VA_ARGS__>(SimKParams);
DEMC_SIM_INSTANCES(DEMC_X_)
#undef DEMC_X_
#define DEMC_X_(...) extern template __global__ void k_sim_choice<__VA_ARGS__>(SimKParams);
DEMC_SIM_CHOICE_INSTANCES(DEMC_X_)
#undef DEMC_X_
#endif
}  // namespace demc
#endif
