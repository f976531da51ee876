// demc_pointwise.cpp -- the kernels of demc_pointwise_loglik and demc_waic (demc_pointwise.hpp says what each does) and the host
// code that strings them together, in a translation unit of their own: the other code objects of the library do not change when
// this one does.
#include "demc_pointwise.hpp"

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, PassTrace, finish
#include "demc_pwterm.hpp"  // the term itself: pw_prepare_draw, PwObs, pw_load, pw_term, pw_table (shared with demc_loo.cpp)

namespace demc {

namespace {

// a draw's constants, once per draw
__global__ __launch_bounds__(kPwPrepWG) void k_pw_prepare(PwKParams p) {
    for (long long s = (long long)blockIdx.x * kPwPrepWG + threadIdx.x; s < p.S; s += (long long)gridDim.x * kPwPrepWG) pw_prepare_draw(p, s);
}

// One pass over the chunk's draws.  `cst` is the kernel's own restrict-qualified argument (not a field of p): the loads of a draw's
// constants are then known not to alias the stores and stay scalar loads.
template <int F, int X>
__global__ __launch_bounds__(kPwWG) void k_pw_accumulate(PwKParams p, const double* __restrict__ cst) {
    __shared__ double s_tab[pw_table_len<F>()];
    const double* tab = pw_table<F>(s_tab);
    const long long i = (long long)blockIdx.x * kPwWG + threadIdx.x;
    const bool valid = i < p.N;
    PwObs<F, X> o;
    pw_load<F, X>(p, valid ? i : p.N - 1, o);  // (a lane past the end walks the last observation and writes nothing)
    const double lsg = F == PW_LNR ? log(p.c0) : 0.0, isg = F == PW_LNR ? 1.0 / p.c0 : 0.0;
    const long long s0 = (long long)blockIdx.y * p.chunk_len, s1 = s0 + p.chunk_len < p.S ? s0 + p.chunk_len : p.S;
    double M = -INFINITY, E = 0.0, l0 = 0.0, a1 = 0.0, a2 = 0.0;
    int flags = 0;
    for (long long s = s0; s < s1; ++s) {
        const double l = pw_term<F, X>(p, cst + (size_t)s * p.K, o, tab, lsg, isg);
        if (s == s0) l0 = l;
        const double dl = l - l0;
        a1 += dl;
        a2 += dl * dl;
        if (l != l)
            flags |= 3;
        else if (l == -INFINITY)
            flags |= 1;
        else if (l > M) {
            E = E * exp(M - l) + 1.0;
            M = l;
        } else
            E += exp(l - M);
    }
    if (!valid) return;
    const double n = (double)(s1 - s0);
    const size_t N = (size_t)p.N;
    double* out = p.part + (size_t)blockIdx.y * kPwPartial * N + (size_t)i;
    out[0] = M;
    out[N] = E;
    out[2 * N] = l0 + a1 / n;
    out[3 * N] = a2 - (a1 * a1) / n;
    out[4 * N] = (double)flags;
}

// the chunks of an observation in index order, then its four values (-ffp-contract=off: the expressions are the ones written)
__global__ __launch_bounds__(kPwWG) void k_pw_final(PwKParams p) {
    const long long i = (long long)blockIdx.x * kPwWG + threadIdx.x;
    if (i >= p.N) return;
    const size_t N = (size_t)p.N;
    const double* part = p.part + (size_t)i;
    double M = part[0];
    for (int c = 1; c < p.chunks; ++c) {
        const double m = part[(size_t)c * kPwPartial * N];
        M = m > M ? m : M;
    }
    double E = 0.0;
    for (int c = 0; c < p.chunks; ++c) {
        const double* pc = part + (size_t)c * kPwPartial * N;
        const double Ec = pc[N];
        if (Ec != 0.0) E += Ec * exp(pc[0] - M);  // (a chunk without a finite term has E_c = 0 and M_c = -Inf)
    }
    const double S = (double)p.S;
    double lppd = M + log(E) - log(S);
    double n = (double)(p.chunk_len < p.S ? p.chunk_len : p.S), mean = part[2 * N], M2 = part[3 * N];
    int flags = (int)part[4 * N];
    for (int c = 1; c < p.chunks; ++c) {  // Chan, Golub, LeVeque: the pairwise rule, chunk by chunk
        const double* pc = part + (size_t)c * kPwPartial * N;
        const long long s0 = (long long)c * p.chunk_len;
        const double nb = (double)((s0 + p.chunk_len < p.S ? s0 + p.chunk_len : p.S) - s0);
        const double tot = n + nb, delta = pc[2 * N] - mean;
        mean = mean + delta * (nb / tot);
        M2 = (M2 + pc[3 * N]) + (delta * delta) * (n * nb / tot);
        n = tot;
        flags |= (int)pc[4 * N];
    }
    double p_waic = M2 / (S - 1.0);  // (S = 1: 0 / 0)
    if (flags & 1) { mean = pw_nan(); p_waic = pw_nan(); }
    if (flags & 2) lppd = pw_nan();
    double* out = p.point + (size_t)(p.order ? p.order[i] : i) * DEMC_WAIC_NPOINT;
    out[0] = lppd;
    out[1] = p_waic;
    out[2] = mean;
    out[3] = lppd - p_waic;
}

// the eight totals of the table, rows in the caller's order
__global__ __launch_bounds__(kPwTotalsWG) void k_pw_totals(PwKParams p) {
    __shared__ double sh[kPwTotalsWG];
    const int t = threadIdx.x;
    auto block_sum = [&](double v) {  // a halving tree over the threads; every thread returns the sum
        sh[t] = v;
        __syncthreads();
        for (int w = kPwTotalsWG / 2; w > 0; w >>= 1) {
            if (t < w) sh[t] += sh[t + w];
            __syncthreads();
        }
        const double r = sh[0];
        __syncthreads();
        return r;
    };
    double lppd = 0.0, pw = 0.0, mean = 0.0, elpd = 0.0, high = 0.0, bad = 0.0;
    for (long long i = t; i < p.N; i += kPwTotalsWG) {
        const double* r = p.point + (size_t)i * DEMC_WAIC_NPOINT;
        lppd += r[0]; pw += r[1]; mean += r[2]; elpd += r[3];
        high += r[1] > 0.4 ? 1.0 : 0.0;
        bad += (isfinite(r[0]) && isfinite(r[1])) ? 0.0 : 1.0;
    }
    lppd = block_sum(lppd); pw = block_sum(pw); mean = block_sum(mean); elpd = block_sum(elpd); high = block_sum(high); bad = block_sum(bad);
    const double N = (double)p.N, ebar = elpd / N;
    double ss = 0.0;
    for (long long i = t; i < p.N; i += kPwTotalsWG) {
        const double dv = p.point[(size_t)i * DEMC_WAIC_NPOINT + 3] - ebar;
        ss += dv * dv;
    }
    ss = block_sum(ss);
    if (t == 0) {
        p.total[0] = elpd;
        p.total[1] = sqrt(N * (ss / (N - 1.0)));  // (N = 1: 0 / 0)
        p.total[2] = pw;
        p.total[3] = lppd;
        p.total[4] = -2.0 * elpd;
        p.total[5] = -2.0 * mean;
        p.total[6] = high;
        p.total[7] = bad;
    }
}

// the terms themselves: out[s][i], caller's order
template <int F, int X>
__global__ __launch_bounds__(kPwWG) void k_pw_matrix(PwKParams p, const double* __restrict__ cst, double* __restrict__ out) {
    __shared__ double s_tab[pw_table_len<F>()];
    const double* tab = pw_table<F>(s_tab);
    const long long i = (long long)blockIdx.x * kPwWG + threadIdx.x;
    const bool valid = i < p.N;
    PwObs<F, X> o;
    pw_load<F, X>(p, valid ? i : p.N - 1, o);
    const double lsg = F == PW_LNR ? log(p.c0) : 0.0, isg = F == PW_LNR ? 1.0 / p.c0 : 0.0;
    const long long s0 = (long long)blockIdx.y * p.chunk_len, s1 = s0 + p.chunk_len < p.S ? s0 + p.chunk_len : p.S;
    const size_t col = (size_t)(valid ? (p.order ? p.order[i] : i) : 0);
    for (long long s = s0; s < s1; ++s) {
        const double l = pw_term<F, X>(p, cst + (size_t)s * p.K, o, tab, lsg, isg);
        if (valid) out[(size_t)s * (size_t)p.N + col] = l;
    }
}

// false: no instance for (family, X) -- a missing kernel is an error, not a detour
bool launch_walk(bool matrix, const PwKParams& p, hipStream_t st) {
    const dim3 grid((unsigned)((p.N + kPwWG - 1) / kPwWG), (unsigned)p.chunks), wg(kPwWG);
    const int x = pw_instance_x(p);
#define DEMC_Y_(F, X)                                                                                      \
    if (p.fam == F && x == X) {                                                                            \
        if (matrix) hipLaunchKernelGGL((k_pw_matrix<F, X>), grid, wg, 0, st, p, (const double*)p.cst, p.matrix); \
        else hipLaunchKernelGGL((k_pw_accumulate<F, X>), grid, wg, 0, st, p, (const double*)p.cst);        \
        return true;                                                                                       \
    }
    DEMC_PW_INSTANCES(DEMC_Y_)
#undef DEMC_Y_
    return false;
}

PwKParams base_params(const PwModelView& mv, const PwPlan& plan) {
    PwKParams p = pw_base_params(mv, plan.fam);
    p.S = plan.S; p.K = plan.K; p.chunk_len = plan.chunk_len; p.chunks = plan.chunks;
    return p;
}

}  // namespace

int pw_waic_run(const PwModelView& mv, const HistView& v, const PwPlan& plan, hipStream_t st, double* total_out, double* point_out, std::string& err) {
    const char* who = "demc_waic";
    PwKParams p = base_params(mv, plan);
    p.theta = v.hist + (size_t)v.row0 * v.P * v.ld;
    p.ld = v.ld; p.D = v.D; p.bounds = nullptr;
    Scratch s;
    if (!(s.get(&p.cst, plan.n_cst) && s.get(&p.part, plan.n_part) && s.get(&p.point, plan.n_point) && s.get(&p.total, plan.n_total))) {
        err = "demc_waic: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    PassTrace tr;  // (the diagnostic variant: device time of the three passes)
    bool ok = tr.mark(st);
    hipLaunchKernelGGL(k_pw_prepare, dim3((unsigned)plan.prep_blocks), dim3(kPwPrepWG), 0, st, p);
    ok = ok && tr.mark(st);
    if (!launch_walk(false, p, st)) { err = "demc_waic: no k_pw_accumulate instance for this model"; return DEMC_EUNSUPPORTED; }
    ok = ok && tr.mark(st);
    hipLaunchKernelGGL(k_pw_final, dim3((unsigned)plan.final_blocks), dim3(kPwWG), 0, st, p);
    hipLaunchKernelGGL(k_pw_totals, dim3(1), dim3(kPwTotalsWG), 0, st, p);
    ok = ok && tr.mark(st);
    if (!ok) { err = "demc_waic: an event could not be recorded"; return DEMC_EHIP; }
    if (!finish(who, st, {{total_out, p.total, plan.n_total * sizeof(double)}, {point_out, p.point, plan.n_point * sizeof(double)}}, err)) return DEMC_EHIP;
    tr.print(who, 3, 1);
    return DEMC_OK;
}

int pw_matrix_run(const PwModelView& mv, const double* theta_host, int D, const DimTab* bounds_dev, const PwPlan& plan, hipStream_t st, double* out,
                  std::string& err) {
    const char* who = "demc_pointwise_loglik";
    PwKParams p = base_params(mv, plan);
    double* d_theta = nullptr;
    Scratch s;
    if (!(s.get(&d_theta, plan.n_theta) && s.get(&p.cst, plan.n_cst) && s.get(&p.matrix, plan.n_matrix))) {
        err = "demc_pointwise_loglik: out of device memory for the staging buffers";
        return DEMC_ENOMEM;
    }
    if (!hip_ok(who, hipMemcpyAsync(d_theta, theta_host, plan.n_theta * sizeof(double), hipMemcpyHostToDevice, st), err)) return DEMC_EHIP;
    p.theta = d_theta; p.ld = D; p.D = D; p.bounds = bounds_dev;
    hipLaunchKernelGGL(k_pw_prepare, dim3((unsigned)plan.prep_blocks), dim3(kPwPrepWG), 0, st, p);
    if (!launch_walk(true, p, st)) { err = "demc_pointwise_loglik: no k_pw_matrix instance for this model"; return DEMC_EUNSUPPORTED; }
    if (!finish(who, st, {{out, p.matrix, plan.n_matrix * sizeof(double)}}, err)) return DEMC_EHIP;
    return DEMC_OK;
}

}  // namespace demc
