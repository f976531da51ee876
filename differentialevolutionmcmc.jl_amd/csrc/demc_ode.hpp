// demc_ode.hpp -- ODE-trajectory likelihoods: k_ode_loglike<SYS>, the likelihood kernel (K2 slot) of models whose mean is the
// solution of an initial-value problem observed with Gaussian noise (include/demc.h: DEMC_FAM_ODE_LV,
// Examples/Predator_Prey_Example.jl:6-11,56-65).  K1 -> k_ode_loglike -> k_accept_store, partial[slot] the hand-over,
// n_partials = 1 -- the place k_sim_loglike has in the launch schedule; no resident, fused or lean form.
//
// SPECIFICATION.  Everything below is IEEE double, compiled with -ffp-contract=off: every line is ONE rounded operation unless it
// says otherwise, in this order, so that it can be restated operation for operation (tests/test_ode_host.py does, in numpy).
//   proposal row  theta = (p_0 .. p_{NPAR-1}, sigma); state u = (u_0 .. u_{DIM-1}); data Y[T][DIM]; from the host, once per model:
//   h = dt / substeps, h2 = 0.5 h (exact), h6 = h / 6 (the one division of the solver).
//   u <- u0.  ss <- 0.  For j = 0 .. T-1:
//     for c = 0 .. DIM-1:  r = Y[j][c] - u_c;  q = r r;  ss = ss + q                     (residuals in (j, c) order, one accumulator)
//     if j < T-1: `substeps` times the classical Runge-Kutta step
//       k1 = f(u)
//       for c: v_c = h2 k1_c;  w_c = u_c + v_c          k2 = f(w)
//       for c: v_c = h2 k2_c;  w_c = u_c + v_c          k3 = f(w)
//       for c: v_c = h  k3_c;  w_c = u_c + v_c          k4 = f(w)
//       for c: s = 2 k2_c (exact);  s = k1_c + s;  t = 2 k3_c (exact);  s = s + t;  s = s + k4_c;  s = h6 s;  u_c = u_c + s
//     (T = 1: no step at all, the residual is taken at u0 only)
//   Lotka-Volterra (SYS = lv: DIM = 2, NPAR = 4, p = (alpha, beta, gamma, delta), u = (x, y)):
//       f_0:  a = beta y;   a = alpha - a;  f_0 = a x            ( = (alpha - beta y) x )
//       f_1:  b = delta x;  b = b - gamma;  f_1 = b y            ( = (delta x - gamma) y )
//   loglike:  l = log(sigma);  l = 2 l (exact);  l = log(2 pi) + l;  l = T l;  v = sigma sigma;  v = 2 v (exact);  e = ss / v;
//             loglike = (-l) - e              ( = -T (log 2 pi + 2 log sigma) - ss / (2 sigma^2), T counted once per time point
//                                               because DIM = 2 halves of log(2 pi sigma^2) make one whole; general DIM: the
//                                               factor is T DIM / 2, exact for even DIM )
//   -Inf instead when sigma <= 0, sigma is not finite, ss is not finite (any non-finite state at an observation or residual ends
//   there: squares are never negative, so nothing cancels an Inf, and a NaN stays one), or the result is a NaN (sigma^2
//   underflowed under ss = 0).  Never a NaN into the accept step -- the simulation kernels' rule (demc_simlike.hpp).
// The only function call is the log of sigma; tests hold the kernel to the restatement at the project's 1e-9 relative bar and to
// the same model written as a user's whole-row source (demc_set_model_source_row) bit for bit in theta.
//
// The reference solves with the adaptive Tsit5(); this is a FIXED-step fourth-order method: DESIGN.md 5.4 has the measured global
// error against the step and the recommended default.
//
// Geometry: a trajectory is sequential in time, so the parallelism is across proposals -- one thread per proposal, 256-thread
// workgroups, grid (launch groups, ceil(n_act / 256)): every group's moving particles get workgroups of their own, so that a small
// population (the example: 3 groups x 6 moving particles) still lands on several CUs.  The 2 T data doubles are the same for every lane:
// staged in LDS once per workgroup (broadcast reads) rather than left to scalar loads, whose scalar form the compiler does not
// promise.  Parameters and the Runge-Kutta state stay in registers.  The kernel is a dependent chain of
// (T - 1) substeps steps: latency-bound at any population that does not fill the chip.
//
// A second system is a functor like OdeLV (DIM, NPAR, rhs), a line in DEMC_ODE_INSTANCES and in ode_system_name, and its family in
// demc_set_model.
#pragma once
#include "demc_kernels.hpp"

namespace demc {

constexpr int FAM_ODE_LV = 9;      // DEMC_FAM_ODE_LV
constexpr int kOdeMaxT = 4096;     // observation times: 2 T doubles = 64 KB of LDS at the cap
constexpr int kOdeMaxSubsteps = 1024;
enum OdeSys : int { ODE_LV = 0 };

// kernarg of k_ode_loglike
struct OdeKParams {
    int n_groups, Np, D, a_lo, n_act;
    int T, substeps, pad_;
    double u0[4];               // initial state (DIM <= 4)
    double h, h2, h6;           // dt / substeps, its half, its sixth: from the host, once per model
    const double* prop;         // [P][D]
    double* partial;            // [P]
    const double* obs;          // [T][DIM]
    const int* glist;
};

struct OdeLV {
    static constexpr int DIM = 2, NPAR = 4;
    __device__ static __forceinline__ void rhs(const double* u, const double* p, double* f) {
        double a = p[1] * u[1];
        a = p[0] - a;
        f[0] = a * u[0];
        double b = p[3] * u[0];
        b = b - p[2];
        f[1] = b * u[1];
    }
};
template <int SYS> struct OdeSystemOf;
template <> struct OdeSystemOf<ODE_LV> { using type = OdeLV; };

template <int SYS>
__global__ __launch_bounds__(256) void k_ode_loglike(OdeKParams p) {
    using S = typename OdeSystemOf<SYS>::type;
    constexpr int DIM = S::DIM, NPAR = S::NPAR;
    extern __shared__ double s_obs[];  // [T][DIM]
    const int tid = threadIdx.x;
    const int n_data = p.T * DIM;
    for (int i = tid; i < n_data; i += 256) s_obs[i] = p.obs[i];
    __syncthreads();
    const int a = blockIdx.y * 256 + tid;  // moving particle of the group
    if (a >= p.n_act) return;
    const int gq = blockIdx.x;
    const int g = p.glist ? p.glist[gq] : gq;
    const size_t slot = (size_t)g * p.Np + p.a_lo + a;
    const double* th = p.prop + slot * p.D;
    double par[NPAR], u[DIM];
#pragma unroll
    for (int i = 0; i < NPAR; ++i) par[i] = th[i];
    const double sigma = th[NPAR];
#pragma unroll
    for (int c = 0; c < DIM; ++c) u[c] = p.u0[c];
    const double h = p.h, h2 = p.h2, h6 = p.h6;
    double ss = 0.0;
    for (int j = 0; j < p.T; ++j) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) {
            const double r = s_obs[j * DIM + c] - u[c];
            const double q = r * r;
            ss = ss + q;
        }
        if (j + 1 < p.T)
            for (int s = 0; s < p.substeps; ++s) {
                double k1[DIM], k2[DIM], k3[DIM], k4[DIM], w[DIM];
                S::rhs(u, par, k1);
#pragma unroll
                for (int c = 0; c < DIM; ++c) { const double v = h2 * k1[c]; w[c] = u[c] + v; }
                S::rhs(w, par, k2);
#pragma unroll
                for (int c = 0; c < DIM; ++c) { const double v = h2 * k2[c]; w[c] = u[c] + v; }
                S::rhs(w, par, k3);
#pragma unroll
                for (int c = 0; c < DIM; ++c) { const double v = h * k3[c]; w[c] = u[c] + v; }
                S::rhs(w, par, k4);
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    double t = 2.0 * k2[c];
                    t = k1[c] + t;
                    const double t3 = 2.0 * k3[c];
                    t = t + t3;
                    t = t + k4[c];
                    t = h6 * t;
                    u[c] = u[c] + t;
                }
            }
    }
    double l = log(sigma);
    l = 2.0 * l;
    l = kLog2Pi + l;
    l = ((double)p.T * (0.5 * DIM)) * l;
    double v = sigma * sigma;
    v = 2.0 * v;
    const double e = ss / v;
    double ll = (-l) - e;
    const bool bad = !(sigma > 0.0) || !(sigma < INFINITY) || !(ss < INFINITY) || !(ll == ll);
    p.partial[slot] = bad ? -INFINITY : ll;
}

// X(SYS): the instances the library ships (demc_ode.cpp, demc_instances.hpp)
#define DEMC_ODE_INSTANCES(X) X(ODE_LV)
#ifdef DEMC_ODE_EXTERN
#define DEMC_X_(...) extern template __global__ void k_ode_loglike<__VA_ARGS__>(OdeKParams);
DEMC_ODE_INSTANCES(DEMC_X_)
#undef DEMC_X_
#endif

}  // namespace demc
