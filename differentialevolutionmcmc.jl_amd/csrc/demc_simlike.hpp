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
enum SimKind : int { SIM_NORMAL = 0, SIM_BINOMIAL = 1, SIM_USER = 100 };
enum SimEst : int { EST_KDE = 0, EST_FREQ = 1 };

// kernarg of k_sim_loglike (the JIT instance reads the same struct)
struct SimKParams {
    int n_groups, Np, D, a_lo, n_act, group_offset;
    int n_sim, nhyper;          // nhyper: the simulator's own hyper-parameters (behind the bandwidth)
    long long n_obs, iter;
    unsigned long long seed;
    unsigned sweep, entity_base;  // entity = entity_base + (group_offset + g) Np + p
    double bandwidth;           // > 0: the KDE's h; else the rule of thumb
    double n_pow;               // n^(-1/5), from the host
    const double* prop;         // [P][D]
    double* partial;            // [P]
    const double* obs;          // [n_obs]
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
__device__ double demc_user_sim(const double* theta, int D, const double* hyper, int nhyper, demc_sim_rng* rng);
#define DEMC_SIM_KERNEL_HEAD extern "C" __global__ __launch_bounds__(256) void k_sim_loglike_user(demc::SimKParams p)
#else
#define DEMC_SIM_KERNEL_HEAD template <int SIM, int EST> __global__ __launch_bounds__(256) void k_sim_loglike(SimKParams p)
#endif

#ifndef DEMC_SIM_JIT
namespace demc {
#else
using namespace demc;
constexpr int SIM = SIM_USER;
constexpr int EST = DEMC_SIM_JIT_EST;
#endif

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

#ifndef DEMC_SIM_JIT
#define DEMC_SIM_INSTANCES(X) X(SIM_NORMAL, EST_KDE) X(SIM_NORMAL, EST_FREQ) X(SIM_BINOMIAL, EST_KDE) X(SIM_BINOMIAL, EST_FREQ)
#ifdef DEMC_SIMLIKE_EXTERN
#define DEMC_X_(...) extern template __global__ void k_sim_loglike<__VA_ARGS__>(SimKParams);
DEMC_SIM_INSTANCES(DEMC_X_)
#undef DEMC_X_
#endif
}  // namespace demc
#endif
