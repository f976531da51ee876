// demc_bridge.cpp -- the kernels of demc_bridge (demc_bridge.hpp says what each does; DESIGN.md 5.10 is the definition) and the host
// code that strings them together, in a translation unit of their own: the other code objects of the library do not change when
// this one does.
#include "demc_bridge.hpp"

#include <vector>

#include "../../include/demc.h"
#include "demc_cov.hpp"     // cov_run (declaration only: the kernels stay in demc_cov.cpp)
#include "demc_devmem.hpp"  // Scratch, PassTrace, finish
#include "demc_philox.hpp"  // draw_block, u53

namespace demc {

namespace {

__device__ __forceinline__ unsigned long long bridge_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double bridge_unkey(unsigned long long k) {
    if (k == 0) return __longlong_as_double(0x7ff8000000000000LL);  // no l1 but NaNs
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(kBridgeWG) void k_bridge_transform(BridgeKParams p) {
    const long long e = (long long)blockIdx.x * kBridgeWG + threadIdx.x;
    if (e >= p.n_win) return;
    const double* src = p.hist + (size_t)e * p.ld;
    double* dst = p.xi + (size_t)e * p.D;
    double lj = 0.0;
    for (int k = 0; k < p.D; ++k) {
        const double lo = p.tab[k].lo, hi = p.tab[k].hi;
        const double th = src[k];
        const double x = bridge_forward(th, lo, hi);
        if (!isfinite(x)) {
            atomicAdd(&p.word[BW_BAD], 1ull);
            atomicMin(&p.word[BW_FIRST_BAD], (unsigned long long)(e * p.D + k));
        }
        dst[k] = x;
        lj += bridge_logjac(x, lo, hi);
        if (e >= p.n_fit) p.th1[(size_t)(e - p.n_fit) * p.D + k] = th;
    }
    p.lj1[e] = lj;
}

// One wave per workgroup, a draw per lane; zs[k][lane] in LDS is the lane's own column: no barrier.
__global__ __launch_bounds__(kBridgeLane) void k_bridge_draw(BridgeKParams p) {
    extern __shared__ double zs[];
    const int lane = threadIdx.x;
    const long long j = (long long)blockIdx.x * kBridgeLane + lane;
    const long long jj = j < p.N2 ? j : p.N2 - 1;  // (the rows that pad the last chunk, and the lanes past it, repeat the last draw)
    const int D = p.D;
    double q = 0.0;
    for (int k2 = 0; 2 * k2 < D; ++k2) {
        const U4 b = draw_block(p.seed, kBridgeStream, 0u, 0ull, (uint32_t)jj, (uint32_t)k2);
        const double u1 = u53(b.x, b.y), u2 = u53(b.z, b.w);
        const double rad = sqrt(-2.0 * log(1.0 - u1));
        double sn, cs;
        sincospi(2.0 * u2, &sn, &cs);
        const double za = rad * cs, zb = rad * sn;
        zs[(2 * k2) * kBridgeLane + lane] = za;
        q += za * za;
        if (2 * k2 + 1 < D) {
            zs[(2 * k2 + 1) * kBridgeLane + lane] = zb;
            q += zb * zb;
        }
    }
    const double* m = p.fit;
    const double* L = p.fit + D;
    double lj = 0.0;
    for (int i = 0; i < D; ++i) {
        double x = m[i];
        for (int k = 0; k <= i; ++k) x += L[(size_t)i * D + k] * zs[k * kBridgeLane + lane];
        const double lo = p.tab[i].lo, hi = p.tab[i].hi;
        lj += bridge_logjac(x, lo, hi);
        if (j < p.pad2) p.th2[(size_t)j * D + i] = bridge_inverse(x, lo, hi);
    }
    if (j < p.N2) {
        p.lj2[j] = lj;
        p.lg2[j] = -0.5 * q - p.fit[D + D * D];
    }
}

// log g of the estimate half: y = L^-1 (xi - m), a draw per lane, y[k][lane] in LDS
__global__ __launch_bounds__(kBridgeLane) void k_bridge_solve(BridgeKParams p) {
    extern __shared__ double ys[];
    const int lane = threadIdx.x;
    const long long i = (long long)blockIdx.x * kBridgeLane + lane;
    if (i >= p.N1) return;
    const int D = p.D;
    const double* x = p.xi + (size_t)(p.n_fit + i) * D;
    const double* m = p.fit;
    const double* L = p.fit + D;
    double q = 0.0;
    for (int k = 0; k < D; ++k) {
        double t = x[k] - m[k];
        for (int c = 0; c < k; ++c) t -= L[(size_t)k * D + c] * ys[c * kBridgeLane + lane];
        const double y = t / L[(size_t)k * D + k];
        ys[k * kBridgeLane + lane] = y;
        q += y * y;
    }
    p.lg1[i] = -0.5 * q - p.fit[D + D * D];
}

__global__ __launch_bounds__(kBridgeWG) void k_bridge_logs(BridgeKParams p) {
    const long long i = (long long)blockIdx.x * kBridgeWG + threadIdx.x;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    if (i < p.N1) {
        const double l = p.lp1[i] + p.lj1[p.n_fit + i] - p.lg1[i];
        p.l1[i] = l;
        if (l != l || l == inf) atomicAdd(&p.word[BW_NONFINITE], 1ull);
        if (l == l) atomicMax(&p.word[BW_LSTAR_KEY], bridge_key(l));
    }
    if (i < p.N2) {
        const double lp = p.lp2[i];
        const double l = lp + p.lj2[i] - p.lg2[i];
        p.l2[i] = l;
        if (lp == -inf) atomicAdd(&p.word[BW_ZERO], 1ull);
        if (l != l || l == inf) atomicAdd(&p.word[BW_NONFINITE], 1ull);
    }
}

__global__ __launch_bounds__(kBridgeWG) void k_bridge_exp(BridgeKParams p) {
    const long long i = (long long)blockIdx.x * kBridgeWG + threadIdx.x;
    const double lstar = bridge_unkey(p.word[BW_LSTAR_KEY]);
    if (i < p.N1) p.e1[i] = exp(p.l1[i] - lstar);
    if (i < p.N2) p.e2[i] = exp(lstar - p.l2[i]);
    if (i == 0) {
        p.val[BV_R] = 1.0;
        p.val[BV_LSTAR] = lstar;
        if (p.word[BW_NONFINITE] > 0 || !isfinite(lstar)) p.word[BW_FLAG] = BF_STOPPED;
    }
}

// the sum of v over the workgroup by a halving tree, in thread 0
__device__ __forceinline__ double bridge_tree(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int w = kBridgeWG / 2; w > 0; w >>= 1) {
        if (t < w) sh[t] += sh[t + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// a term of the proposal side (f1) and of the posterior side: MODE 0 the means of an iteration, 1 f1 / f2, 2 their squared deviations
template <int MODE>
__device__ __forceinline__ double bridge_term2(const BridgeKParams& p, double e2, double r) {
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const double f = e2 == inf ? 0.0 : 1.0 / (p.s1 + (p.s2 * r) * e2);
    if (MODE == 2) { const double d = f - p.val[BV_MEAN1]; return d * d; }
    return f;
}
template <int MODE>
__device__ __forceinline__ double bridge_term1(const BridgeKParams& p, double e1, double r) {
    if (MODE == 0) return 1.0 / (p.s1 * e1 + p.s2 * r);
    const double f = 1.0 / ((p.s1 * e1) / r + p.s2);
    if (MODE == 2) { const double d = f - p.val[BV_MEAN2]; return d * d; }
    return f;
}

template <int MODE>
__global__ __launch_bounds__(kBridgeWG) void k_bridge_part(BridgeKParams p) {
    __shared__ double sh[kBridgeWG];
    if (MODE == 0 && p.word[BW_FLAG] != BF_RUNNING) return;  // (uniform over the grid: the flag changes between launches only)
    const double r = p.val[BV_R];
    const int b = blockIdx.x;
    double s = 0.0;
    if (b < p.W2) {
        const long long stride = (long long)p.W2 * kBridgeWG;
        for (long long j = (long long)b * kBridgeWG + threadIdx.x; j < p.N2; j += stride) s += bridge_term2<MODE>(p, p.e2[j], r);
    } else {
        const long long stride = (long long)p.W1 * kBridgeWG;
        for (long long i = (long long)(b - p.W2) * kBridgeWG + threadIdx.x; i < p.N1; i += stride) s += bridge_term1<MODE>(p, p.e1[i], r);
    }
    s = bridge_tree(s, sh);
    if (threadIdx.x == 0) p.part[b] = s;
}

template <int MODE>
__global__ __launch_bounds__(kBridgeWG) void k_bridge_final(BridgeKParams p) {
    __shared__ double sh[kBridgeWG];
    if (MODE == 0 && p.word[BW_FLAG] != BF_RUNNING) return;
    const int t = threadIdx.x;
    const double a = bridge_tree(t < p.W2 ? p.part[t] : 0.0, sh);           // (W1, W2 <= kBridgeMaxW = kBridgeWG)
    const double c = bridge_tree(t < p.W1 ? p.part[p.W2 + t] : 0.0, sh);
    if (t != 0) return;
    if (MODE == 0) {
        const double r = p.val[BV_R];
        const double num = a / (double)p.N2, den = c / (double)p.N1;
        const double rn = num / den;
        const double change = fabs(rn - r);
        p.val[BV_R] = rn;
        p.val[BV_REL] = change / fabs(rn);
        p.word[BW_ITER] += 1;
        if (change <= kBridgeTol * fabs(rn)) p.word[BW_FLAG] = BF_CONVERGED;
        else if (!(isfinite(rn) && rn > 0.0)) p.word[BW_FLAG] = BF_STOPPED;
    } else if (MODE == 1) {
        p.val[BV_MEAN1] = a / (double)p.N2;
        p.val[BV_MEAN2] = c / (double)p.N1;
    } else {
        p.val[BV_SS1] = a;
        p.val[BV_SS2] = c;
    }
}

template <int MODE>
void launch_reduce(const BridgeKParams& p, hipStream_t st) {
    hipLaunchKernelGGL((k_bridge_part<MODE>), dim3((unsigned)(p.W1 + p.W2)), dim3(kBridgeWG), 0, st, p);
    hipLaunchKernelGGL((k_bridge_final<MODE>), dim3(1), dim3(kBridgeWG), 0, st, p);
}

unsigned blocks_of(long long n) { return (unsigned)((n + kBridgeWG - 1) / kBridgeWG); }

}  // namespace

static_assert(kBridgeMaxW <= kBridgeWG, "k_bridge_final reads one partial sum per thread");

int bridge_run(const HistView& v, const DimTab* tab, const BridgePlan& plan, const CovPlan& fitplan, unsigned long long seed, hipStream_t st, const BridgeEval& eval,
               double* out, double* prop_out, double* post_out, double* fit_out, std::string& err) {
    const char* who = "demc_bridge";
    const int D = v.D;
    const size_t n_fitbuf = (size_t)D + (size_t)D * D + 1;
    BridgeKParams p{};
    p.hist = v.hist + (size_t)v.row0 * v.P * v.ld;
    p.tab = tab; p.D = D; p.ld = v.ld;
    p.n_win = plan.n_win; p.n_fit = plan.n_fit; p.N1 = plan.N1; p.N2 = plan.N2; p.pad2 = plan.pad2;
    p.seed = seed; p.s1 = plan.s1; p.s2 = plan.s2; p.W1 = plan.W1; p.W2 = plan.W2;
    Scratch s;
    double* d_fit = nullptr;
    const size_t N1 = (size_t)plan.N1, N2 = (size_t)plan.N2, pad2 = (size_t)plan.pad2;
    if (!(s.get(&p.xi, (size_t)plan.n_win * D) && s.get(&p.lj1, (size_t)plan.n_win) && s.get(&p.th1, N1 * D) && s.get(&p.lp1, N1) && s.get(&p.lg1, N1) &&
          s.get(&p.th2, pad2 * D) && s.get(&p.lp2, pad2) && s.get(&p.lj2, N2) && s.get(&p.lg2, N2) && s.get(&p.l1, N1) && s.get(&p.l2, N2) &&
          s.get(&p.e1, N1) && s.get(&p.e2, N2) && s.get(&d_fit, n_fitbuf) && s.get(&p.part, (size_t)2 * kBridgeMaxW) && s.get(&p.val, (size_t)BV_COUNT) &&
          s.get(&p.word, (size_t)BW_COUNT))) {
        err = "demc_bridge: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    p.fit = d_fit;
    unsigned long long word[BW_COUNT] = {};
    double val[BV_COUNT] = {};
    word[BW_FIRST_BAD] = ~0ull;
    if (!hip_ok(who, hipMemcpyAsync(p.word, word, sizeof word, hipMemcpyHostToDevice, st), err)) return DEMC_EHIP;
    if (!hip_ok(who, hipMemcpyAsync(p.val, val, sizeof val, hipMemcpyHostToDevice, st), err)) return DEMC_EHIP;
    PassTrace tr;  // (the diagnostic variant: device time of the transform and fit, the draws, the evaluations, the iteration)
    bool ok = tr.mark(st);

    // 1. the window on the real line; a draw on a bound is the call's refusal
    hipLaunchKernelGGL(k_bridge_transform, dim3(blocks_of(plan.n_win)), dim3(kBridgeWG), 0, st, p);
    if (!finish(who, st, {{word, p.word, sizeof word}}, err)) return DEMC_EHIP;
    if (word[BW_BAD] > 0) {
        const Refusal r = bridge_bad_draws((long long)word[BW_BAD], (long long)word[BW_FIRST_BAD], v.row0, v.P, D);
        err = r.message;
        return r.code;
    }

    // 2. the proposal: mean and covariance of the fit half by demc_covariance's kernels, the factor on the host
    std::vector<double> fit(n_fitbuf), V((size_t)D * D);
    {
        // (a history of n_fit rows of one cell, D doubles apart; the kernels read acc and lp only for the series D and D + 1)
        const HistView xv{p.xi, (const unsigned char*)p.lj1, p.lj1, nullptr, 1, 0, plan.n_fit, 0, D, D};
        const int rc = cov_run(xv, fitplan, st, fit.data(), V.data(), nullptr, err);
        if (rc != DEMC_OK) return rc;
    }
    const int pivot = bridge_cholesky(V.data(), D, fit.data() + D);
    if (pivot >= 0) {
        const Refusal r = bridge_bad_pivot(pivot, D);
        err = r.message;
        return r.code;
    }
    fit[n_fitbuf - 1] = bridge_lognorm(fit.data() + D, D);
    if (!hip_ok(who, hipMemcpyAsync(d_fit, fit.data(), n_fitbuf * sizeof(double), hipMemcpyHostToDevice, st), err)) return DEMC_EHIP;
    ok = ok && tr.mark(st);

    // 3. the proposal draws, into the chunks the evaluation reads; log g of the estimate half
    hipLaunchKernelGGL(k_bridge_draw, dim3((unsigned)plan.draw_blocks), dim3(kBridgeLane), plan.lds_bytes, st, p);
    hipLaunchKernelGGL(k_bridge_solve, dim3((unsigned)plan.solve_blocks), dim3(kBridgeLane), plan.lds_bytes, st, p);
    ok = ok && tr.mark(st);

    // 4. the log posterior of both sets, P rows at a time, by the handle's own evaluate path
    for (long long c = 0; c < plan.chunks1; ++c)
        if (const int rc = eval(p.th1 + (size_t)c * v.P * D, p.lp1 + (size_t)c * v.P)) { err = "demc_bridge: the log posterior of the estimate half could not be evaluated"; return rc; }
    for (long long c = 0; c < plan.chunks2; ++c)
        if (const int rc = eval(p.th2 + (size_t)c * v.P * D, p.lp2 + (size_t)c * v.P)) { err = "demc_bridge: the log posterior of the proposal draws could not be evaluated"; return rc; }
    ok = ok && tr.mark(st);

    // 5. the log ratios, l*, the exponentials; the iteration in batches, the flag read between them; the error terms
    const unsigned both = blocks_of(std::max(plan.N1, plan.N2));
    hipLaunchKernelGGL(k_bridge_logs, dim3(both), dim3(kBridgeWG), 0, st, p);
    hipLaunchKernelGGL(k_bridge_exp, dim3(both), dim3(kBridgeWG), 0, st, p);
    for (int it = 0; it < kBridgeMaxIter;) {
        const int n = std::min(kBridgeBatch, kBridgeMaxIter - it);
        for (int k = 0; k < n; ++k) launch_reduce<0>(p, st);
        it += n;
        if (!finish(who, st, {{word, p.word, sizeof word}}, err)) return DEMC_EHIP;
        if (word[BW_FLAG] != BF_RUNNING) break;
    }
    launch_reduce<1>(p, st);
    launch_reduce<2>(p, st);
    ok = ok && tr.mark(st);
    if (!ok) { err = "demc_bridge: an event could not be recorded"; return DEMC_EHIP; }
    if (!finish(who, st, {{word, p.word, sizeof word}, {val, p.val, sizeof val}}, err)) return DEMC_EHIP;
    bridge_outputs(plan, val, word, out);
    tr.print(who, 4, 1);

    // the diagnostics: the device's own stages, for whoever checks them one by one
    if (fit_out) std::copy(fit.begin(), fit.begin() + (D + (size_t)D * D), fit_out);
    if (post_out) {
        std::vector<double> lp(N1), lj(N1), lg(N1);
        if (!finish(who, st, {{lp.data(), p.lp1, N1 * 8}, {lj.data(), p.lj1 + plan.n_fit, N1 * 8}, {lg.data(), p.lg1, N1 * 8}}, err)) return DEMC_EHIP;
        for (size_t i = 0; i < N1; ++i) { post_out[3 * i] = lp[i]; post_out[3 * i + 1] = lj[i]; post_out[3 * i + 2] = lg[i]; }
    }
    if (prop_out) {
        std::vector<double> th(N2 * D), lp(N2), lj(N2), lg(N2);
        if (!finish(who, st, {{th.data(), p.th2, N2 * D * 8}, {lp.data(), p.lp2, N2 * 8}, {lj.data(), p.lj2, N2 * 8}, {lg.data(), p.lg2, N2 * 8}}, err)) return DEMC_EHIP;
        const size_t w = (size_t)D + 3;
        for (size_t j = 0; j < N2; ++j) {
            std::copy(th.begin() + j * D, th.begin() + (j + 1) * D, prop_out + j * w);
            prop_out[j * w + D] = lp[j]; prop_out[j * w + D + 1] = lj[j]; prop_out[j * w + D + 2] = lg[j];
        }
    }
    return DEMC_OK;
}

}  // namespace demc
