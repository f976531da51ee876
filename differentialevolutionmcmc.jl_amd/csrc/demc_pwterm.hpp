// demc_pwterm.hpp -- the text of a per-observation term l_is = log p(y_i | theta_s), once: the constants a draw is turned into
// (pw_prepare_draw), what a lane keeps of its observation (PwObs, pw_load), the term itself (pw_term) and the family's table in LDS
// (pw_table).  Device functions only, no kernel: demc_pointwise.cpp (demc_pointwise_loglik, demc_waic) and demc_loo.cpp (demc_loo)
// wrap them in kernels of their own, so that a term of either call is the same bits (-ffp-contract=off in both units).
#pragma once
#include "demc_device.hpp"     // lba_trial, phiS_Phi_table, log_Phi_neg_table and their tables, kLog2Pi
#include "demc_pointwise.hpp"  // PwKParams, the kPw* constants, PwFamily

namespace demc {

constexpr bool pw_is_mvn(int F) { return F == PW_MVN_ISO || F == PW_MVN_FULL; }

__device__ __forceinline__ double pw_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the constants of draw s
__device__ __forceinline__ void pw_prepare_draw(const PwKParams& p, long long s) {
    const double* th = p.theta + (size_t)s * p.ld;
    double* c = p.cst + (size_t)s * p.K;
    bool flag = false;
    for (int j = 0; j < p.D; ++j) {
        const double v = th[j];
        flag |= v != v;
        if (p.bounds) flag |= !(v >= p.bounds[j].lo && v <= p.bounds[j].hi);  // in_bounds, as the proposal kernel decides it
    }
    switch (p.fam) {
        case PW_GAUSSIAN:
            c[0] = th[0]; c[1] = 1.0 / th[1]; c[2] = -log(th[1]) - 0.5 * kLog2Pi;
            break;
        case PW_BINOMIAL:
            c[0] = log(th[0]); c[1] = log1p(-th[0]);
            break;
        case PW_LNR:
            for (int a = 0; a <= p.n_acc; ++a) c[a] = th[a];
            break;
        case PW_LBA: {  // the operands of lba_trial, formed as lba_range_sum forms them
            const int na = p.n_acc;
            const double A = th[na], kk = th[na + 1], tau = th[na + 2], b = A + kk, inv_A = 1.0 / A;
            double pneg = 1.0;
            for (int a = 0; a < na; ++a) {
                const double nu = th[a], nuS = kPhiS * nu;
                double q, Ph;
                phiS_Phi_table(kPhiTable, -nuS, q, Ph);
                pneg *= Ph;
                c[a] = nu; c[na + a] = nuS;
            }
            c[2 * na] = kPhiS * kk; c[2 * na + 1] = kPhiS * b; c[2 * na + 2] = tau; c[2 * na + 3] = inv_A;
            c[2 * na + 4] = inv_A * (1.0 / kPhiS); c[2 * na + 5] = 1.0 / (1.0 - pneg);
        } break;
        case PW_MVN_ISO: {  // m = theta' - xbar; the sigma terms of loglike_from_stats for one row
            const int d = p.d;
            for (int k = 0; k < p.dp; ++k) c[k] = k < d ? th[k] - p.xbar[k] : 0.0;
            const double sg = th[d];
            c[p.dp] = -0.5 * (double)d * kLog2Pi - (double)d * log(sg);
            c[p.dp + 1] = 0.5 / (sg * sg);
        } break;
        case PW_MVN_FULL: {  // m_c = sum_k M[k][c] (theta' - xbar)_k with M = (L^-1)', the proposal kernel's preparation
            const int d = p.d;
            for (int cc = 0; cc < p.dp; ++cc) {
                double y = 0.0;
                if (cc < d)
                    for (int k = 0; k < d; ++k) y += p.M[(size_t)k * d + cc] * (th[k] - p.xbar[k]);
                c[cc] = y;
            }
        } break;
        default: break;
    }
    c[p.K - 1] = flag ? 1.0 : 0.0;
}

// what a lane keeps of its observation
template <int F, int X>
struct PwObs { double v[pw_is_mvn(F) ? X : 3]; };

template <int F, int X>
__device__ __forceinline__ void pw_load(const PwKParams& p, long long i, PwObs<F, X>& o) {
    if constexpr (F == PW_GAUSSIAN) {
        o.v[0] = p.data[i];
    } else if constexpr (F == PW_BINOMIAL) {  // data = [n], data2 = [k], then the log binomial coefficients
        o.v[0] = p.data[i]; o.v[1] = p.data2[i]; o.v[2] = p.data2[p.N + i];
    } else if constexpr (F == PW_LNR || F == PW_LBA) {  // choice, decision time
        o.v[0] = p.data[i]; o.v[1] = p.data2[i];
    } else {
#pragma unroll
        for (int k = 0; k < X; ++k) o.v[k] = p.data[(size_t)i * X + k];
    }
}

// l_is from the observation in registers and the draw's constants c (wave-uniform: scalar loads); tab: the family's table in LDS
template <int F, int X>
__device__ __forceinline__ double pw_term(const PwKParams& p, const double* __restrict__ c, const PwObs<F, X>& o, const double* tab, double lsg,
                                          double isg) {
    double l;
    if constexpr (F == PW_GAUSSIAN) {
        const double z = (o.v[0] - c[0]) * c[1];
        l = c[2] - 0.5 * (z * z);
    } else if constexpr (F == PW_BINOMIAL) {
        // obs_range_sum's FAM_BINOMIAL term (demc_kernels.hpp) on the two logs of the draw: that function sums inside its own loop and
        // forms the logs per call, so the term is written again here -- the two must change together (a comment there says so)
        const double n = o.v[0], k = o.v[1];
        const double t1 = (k == 0.0) ? 0.0 : k * c[0];
        const double t2 = (n - k == 0.0) ? 0.0 : (n - k) * c[1];
        l = o.v[2] + t1 + t2;
    } else if constexpr (F == PW_LNR) {
        // lnr_range_sum's trial (demc_kernels.hpp), term for term: written again for the same reason, and kept together the same way
        const int na = p.n_acc;
        const double t = o.v[1] - c[na];
        if (!(t > 0.0))
            l = -INFINITY;
        else {
            const double lt = log(t);
            l = 0.0;
            for (int a = 0; a < na; ++a) {
                const double z = (lt - c[a]) * isg;
                l += ((double)(a + 1) == o.v[0]) ? (-(z * z + kLog2Pi) / 2.0 - lsg - lt) : log_Phi_neg_table(tab, z);
            }
        }
    } else if constexpr (F == PW_LBA) {
        const int na = X > 0 ? X : p.n_acc;
        l = log(lba_trial<X, double>(tab, na, c, c + na, c[2 * na], c[2 * na + 1], c[2 * na + 2], c[2 * na + 3], c[2 * na + 4], c[2 * na + 5],
                                     o.v[0], o.v[1]));
    } else {  // |z_i - m|^2 over the padded row (the padding is zero on both sides)
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < X; ++k) {
            const double r = o.v[k] - c[k];
            q += r * r;
        }
        l = F == PW_MVN_FULL ? p.c0 - 0.5 * q : c[X] - q * c[X + 1];
    }
    return c[p.K - 1] != 0.0 ? pw_nan() : l;
}

// the family's table, copied into LDS by a workgroup of kPwWG threads
template <int F>
__device__ __forceinline__ const double* pw_table(double* s_tab) {
    if constexpr (F == PW_LBA) {
        for (int i = threadIdx.x; i < kPhiIntervals * kPhiRow; i += kPwWG) s_tab[i] = kPhiTable[i];
        __syncthreads();
    } else if constexpr (F == PW_LNR) {
        for (int i = threadIdx.x; i < kLogPhiRows * kLogPhiRow; i += kPwWG) s_tab[i] = kLogPhiTable[i];
        __syncthreads();
    }
    return s_tab;
}
template <int F>
constexpr int pw_table_len() { return F == PW_LBA ? kPhiIntervals * kPhiRow : F == PW_LNR ? kLogPhiRows * kLogPhiRow : 1; }

// the instances: <family, X>
#define DEMC_PW_INSTANCES(Y)                                                                                              \
    Y(PW_GAUSSIAN, 0) Y(PW_BINOMIAL, 0) Y(PW_LNR, 0) Y(PW_LBA, 2) Y(PW_LBA, 3) Y(PW_LBA, 0) Y(PW_MVN_ISO, 8) Y(PW_MVN_ISO, 16) \
    Y(PW_MVN_ISO, 32) Y(PW_MVN_ISO, 64) Y(PW_MVN_FULL, 8) Y(PW_MVN_FULL, 16) Y(PW_MVN_FULL, 32) Y(PW_MVN_FULL, 64)

inline int pw_instance_x(const PwKParams& p) {
    if (p.fam == PW_LBA) return p.n_acc == 2 || p.n_acc == 3 ? p.n_acc : 0;
    return pw_is_mvn(p.fam) ? p.dp : 0;
}

inline PwKParams pw_base_params(const PwModelView& mv, PwFamily fam) {
    PwKParams p{};
    p.fam = fam; p.n_acc = mv.m.n_acc; p.d = mv.m.d; p.dp = mv.m.dp; p.N = mv.m.N;
    p.data = mv.data; p.data2 = mv.data2; p.M = mv.M; p.xbar = mv.xbar; p.c0 = mv.c0; p.order = mv.order;
    return p;
}

}  // namespace demc
