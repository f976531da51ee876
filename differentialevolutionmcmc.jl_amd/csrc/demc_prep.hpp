// demc_prep.hpp -- everything between a caller's arrays and the device that needs no device: the validation of a model's data and
// hyper-parameters, the data-only constants and the layouts the kernels read (prepare_model, prepare_sim), and the bounds / prior
// table with its run-length forms (prepare_priors, prepare_bounds, encode_segments, encode_mask).  Host only: plain C++17, no
// device header, no handle, no device memory -- the runtime calls these, reports a refusal through the handle and uploads what
// comes back.  tests/prep_host.cpp runs them on the CPU under the sanitizers.
//
// The order of the floating-point operations here is part of the results: what these functions return is what the kernels read.
#pragma once
#include "../../include/demc.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "demc_dimtab.hpp"
#include "demc_hostbase.hpp"  // Refusal, pow2_ceil

namespace demc {

// The caps the refusals quote.  The kernels' own constants (demc_ode.hpp, demc_simlike.hpp) sit behind the device headers;
// the runtime asserts that the two agree.
constexpr int kPrepOdeMaxT = 4096, kPrepOdeMaxSubsteps = 1024;
constexpr int kPrepSimMaxN = 16384, kPrepSimChoiceMaxN = 15000;

// Sigma = L L' (row-major, d x d): Ainv = Sigma^-1, logdet = log det Sigma, Linv = L^-1.  false: Sigma is not positive definite.
inline bool chol_inv(const double* S, int d, std::vector<double>& Ainv, double& logdet, std::vector<double>* Linv = nullptr) {
    std::vector<double> L((size_t)d * d, 0.0), Li((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = S[i * d + j];
            for (int k = 0; k < j; ++k) s -= L[i * d + k] * L[j * d + k];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[i * d + i] = std::sqrt(s);
            } else
                L[i * d + j] = s / L[j * d + j];
        }
    logdet = 0.0;
    for (int i = 0; i < d; ++i) logdet += 2.0 * std::log(L[i * d + i]);
    for (int c = 0; c < d; ++c)  // Li = L^-1 by forward substitution on unit vectors
        for (int i = 0; i < d; ++i) {
            double s = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= L[i * d + k] * Li[k * d + c];
            Li[i * d + c] = s / L[i * d + i];
        }
    Ainv.assign((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            double s = 0.0;
            for (int k = 0; k < d; ++k) s += Li[k * d + i] * Li[k * d + j];
            Ainv[i * d + j] = s;
        }
    if (Linv) *Linv = Li;
    return true;
}

// log C(n, k)
inline double log_binomial_coefficient(double n, double k) { return std::lgamma(n + 1.0) - std::lgamma(k + 1.0) - std::lgamma(n - k + 1.0); }

// ---- demc_set_model ----------------------------------------------------------------------------------------------------------

// The sizes and data-only constants of a model: what prepare_model works out and the handle's Model record keeps.
struct ModelShape {
    long long N = 0;
    int d = 0, n_acc = 0, dpad = 0;
    int n_tiles = 0;
    int ks_t = 0, n_kpass = 0;  // MFMA k-steps per pass (template) and passes over the dimensions
    int dp_direct = 0;          // DIRECT mode: padded length of a whitened observation row (8 / 16 / 32 / 64)
    size_t data2_off = 0;
    double c0 = 0, c1 = 0, c2 = 0;
    // ODE-trajectory likelihood (DEMC_FAM_ODE_LV, demc_ode.hpp): N = the observation times T, data = Y[T][DIM]
    int ode_substeps = 0;
    double ode_u0[4] = {0, 0, 0, 0}, ode_h = 0.0;
};

// ... and what goes to the device with them (an empty vector: that buffer is not part of the family).  A refused model carries
// nothing but the refusal.
struct PreparedModel : ModelShape {
    Refusal refused;
    std::vector<double> data;      // the observations as the family's kernels read them
    std::vector<double> M;         // MVN_FULL, the Ainv slot: Sigma^-1, or (L^-1)' in DIRECT mode
    std::vector<double> sx, xbar;  // MVN: sum of the centred observations, their mean
    std::vector<double> Xf;        // MVN: the centred observations in MFMA fragment order
    std::vector<int> order;        // LBA: the caller's index of sorted trial k (empty: the data keep the caller's order)
};

inline Refusal prep_gaussian(PreparedModel& m, int D, const double* data, const long long* dm) {
    if (D != 2 || dm[0] < 1) return {DEMC_EINVAL, "GAUSSIAN: theta=(mu,sigma), dims=[N]"};
    m.N = dm[0];
    m.data.assign(data, data + dm[0]);
    return {};
}

inline Refusal prep_binomial(PreparedModel& m, int D, const double* data, const long long* dm) {
    if (D != 1 || dm[0] < 1) return {DEMC_EINVAL, "BINOMIAL: theta=p, dims=[N], data=[n[N],k[N]]"};
    const long long N = dm[0];
    m.N = N;
    m.data.assign(data, data + 2 * N);
    m.data.resize(3 * N);
    for (long long i = 0; i < N; ++i) m.data[2 * N + i] = log_binomial_coefficient(data[i], data[N + i]);
    m.data2_off = (size_t)N;
    return {};
}

inline Refusal prep_hier_binomial(PreparedModel& m, int D, const double* data, const long long* dm, const double* hyper, int nhyper) {
    if (D != dm[0] + 2 || nhyper < 1) return {DEMC_EINVAL, "HIER_BINOMIAL: D=S+2, dims=[S], hyper=[n]"};
    const long long S = dm[0];
    m.N = S;
    m.c0 = hyper[0];
    m.data.assign(data, data + S);
    m.data.resize(2 * S);
    double lgc_sum = 0.0;
    for (long long s = 0; s < S; ++s) {
        m.data[S + s] = log_binomial_coefficient(hyper[0], data[s]);
        lgc_sum += m.data[S + s];
    }
    m.c2 = lgc_sum;  // the long-row kernel adds the coefficients as one data-only constant
    return {};
}

inline Refusal prep_hier_gaussian(PreparedModel& m, int D, const double* data, const long long* dm) {
    if (D != dm[0] + 3 || dm[1] < 1) return {DEMC_EINVAL, "HIER_GAUSSIAN: D=S+3, dims=[S,n]"};
    m.N = dm[0];
    m.d = (int)dm[1];
    m.data.assign(data, data + dm[0] * dm[1]);
    return {};
}

inline Refusal prep_race(PreparedModel& m, int family, int D, const double* data, const long long* dm, const double* hyper, int nhyper) {
    const int extra = (family == DEMC_FAM_LBA) ? 3 : 1;
    if (dm[1] < 1 || dm[1] > 8 || D != dm[1] + extra) return {DEMC_EINVAL, "LBA/LNR: dims=[N,n_acc<=8]"};
    // data = [choice[N] ; rt[N]]: the kernels pick the winning accumulator by comparing the choice code with 1..n_acc
    // (k_lba_wave: exact double equality) and the sort below compares decision times -- a non-integral or out-of-range
    // code would silently make every accumulator a loser, a NaN is no strict weak ordering: refused here
    for (long long i = 0; i < dm[0]; ++i) {
        const double ch = data[i], rt = data[dm[0] + i];
        if (!(ch >= 1.0 && ch <= (double)dm[1] && ch == std::floor(ch)))
            return {DEMC_EINVAL, "LBA/LNR: choice of trial " + std::to_string(i) + " is not an integer in [1, n_acc]"};
        if (!std::isfinite(rt)) return {DEMC_EINVAL, "LBA/LNR: decision time of trial " + std::to_string(i) + " is not finite"};
    }
    m.N = dm[0];
    m.n_acc = (int)dm[1];
    m.c0 = (family == DEMC_FAM_LNR) ? (nhyper > 0 ? hyper[0] : 1.0) : 0.0;
    m.data.assign(data, data + 2 * dm[0]);
    m.data2_off = (size_t)dm[0];
    if (family == DEMC_FAM_LBA) {
        // The log-likelihood is a sum over trials: their order is the library's to choose.  Sorted by (choice, decision time)
        // the 64 lanes of k_lba_wave -- 64 consecutive trials of one proposal -- read the same row or two of the Phi table and
        // share their winner (demc_kernels.hpp).
        const size_t N = (size_t)dm[0];
        std::vector<size_t> order(N);
        for (size_t i = 0; i < N; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b2) {
            return data[a] != data[b2] ? data[a] < data[b2] : data[N + a] < data[N + b2];
        });
        for (size_t i = 0; i < N; ++i) { m.data[i] = data[order[i]]; m.data[N + i] = data[N + order[i]]; }
        // ... and the per-observation calls answer in the caller's (demc_pointwise.hpp): the permutation is kept
        if (N > 0x7fffffffu) return {DEMC_EINVAL, "too many observations"};
        m.order.resize(N);
        for (size_t i = 0; i < N; ++i) m.order[i] = (int)order[i];
    }
    return {};
}

inline Refusal prep_ode_lv(PreparedModel& m, int D, const double* data, const long long* dm, int ndims, const double* hyper, int nhyper) {
    if (D != 5) return {DEMC_EINVAL, "ODE_LV: D = 5 required, theta=(alpha,beta,gamma,delta,sigma)"};
    if (ndims < 2 || dm[1] != 2) return {DEMC_EINVAL, "ODE_LV: dims[1] = 2 required, dims=[T,2] (the observed x and y per time)"};
    if (dm[0] < 1 || dm[0] > kPrepOdeMaxT)
        return {DEMC_EINVAL, "ODE_LV: T = dims[0] = " + std::to_string(dm[0]) + " is outside [1, " + std::to_string(kPrepOdeMaxT) + "]"};
    if (nhyper != 4 || !hyper) return {DEMC_EINVAL, "ODE_LV: hyper=[x0, y0, dt, substeps] (nhyper = 4)"};
    if (!(hyper[3] >= 1.0 && hyper[3] <= (double)kPrepOdeMaxSubsteps && hyper[3] == std::floor(hyper[3])))
        return {DEMC_EINVAL, "ODE_LV: substeps (hyper[3]) must be an integer in [1, " + std::to_string(kPrepOdeMaxSubsteps) + "]"};
    if (!(std::isfinite(hyper[2]) && hyper[2] > 0.0)) return {DEMC_EINVAL, "ODE_LV: dt (hyper[2]) must be finite and positive"};
    if (!std::isfinite(hyper[0]) || !std::isfinite(hyper[1])) return {DEMC_EINVAL, "ODE_LV: u0 = (x0, y0) (hyper[0], hyper[1]) must be finite"};
    if (!data) return {DEMC_EINVAL, "ODE_LV: data = Y[T][2] required"};
    for (long long i = 0; i < 2 * dm[0]; ++i)
        if (!std::isfinite(data[i]))
            return {DEMC_EINVAL, "ODE_LV: data value " + std::to_string(i) + " (time " + std::to_string(i / 2) + ") is not finite"};
    m.N = dm[0];
    m.ode_substeps = (int)hyper[3];
    m.ode_u0[0] = hyper[0]; m.ode_u0[1] = hyper[1]; m.ode_u0[2] = m.ode_u0[3] = 0.0;
    m.ode_h = hyper[2] / hyper[3];
    m.data.assign(data, data + 2 * dm[0]);
    return {};
}

inline Refusal prep_mvn(PreparedModel& m, int family, int D, bool direct, const double* data, const long long* dm, const double* hyper, int nhyper) {
    const long long N = dm[0];
    const int d = (int)dm[1];
    if (N < 1 || d < 1) return {DEMC_EINVAL, "MVN: dims=[N,d]"};
    if (d > 1024) return {DEMC_EUNSUPPORTED, "MVN families: data dimension d <= 1024"};
    if (family == DEMC_FAM_MVN_ISO && D != d + 1) return {DEMC_EINVAL, "MVN_ISO: D=d+1"};
    if (family == DEMC_FAM_MVN_FULL && (D != d || nhyper != d * d)) return {DEMC_EINVAL, "MVN_FULL: D=d, hyper=Sigma[d][d]"};
    m.N = N;
    m.d = d;
    // k-steps of 4 dims: one pass of KS in {1,2,4,8,16} steps for d <= 64, else passes of 16 steps
    if (d <= 64) { m.ks_t = pow2_ceil((d + 3) / 4); m.n_kpass = 1; }
    else { m.ks_t = 16; m.n_kpass = (d + 63) / 64; }
    m.dpad = 4 * m.ks_t * m.n_kpass;
    if ((N + 15) / 16 > 0x3fffffff) return {DEMC_EINVAL, "too many observations"};
    m.n_tiles = (int)((N + 15) / 16);
    if (direct && d > 64) return {DEMC_EUNSUPPORTED, "DIRECT likelihood: data dimension d <= 64 (the whitened proposal lives in registers)"};
    std::vector<double> Ainv, Linv;
    double logdet = 0.0;
    if (family == DEMC_FAM_MVN_FULL) {
        if (!chol_inv(hyper, d, Ainv, logdet, &Linv)) return {DEMC_EINVAL, "Sigma is not positive definite"};
        m.c0 = -0.5 * (double)N * (d * kLog2Pi + logdet);
        // K1's preparation forms y_c = sum_k M[k][c] (theta' - xbar)_k.  M = Sigma^-1 (symmetric) gives y = Sigma^-1 mu~;
        // in DIRECT mode M = (L^-1)' gives the whitened proposal m = L^-1 mu~ instead.
        m.M = Ainv;
        if (direct)
            for (int r = 0; r < d; ++r)
                for (int cc = 0; cc < d; ++cc) m.M[(size_t)r * d + cc] = Linv[(size_t)cc * d + r];
    }
    // The data are CENTRED once (x~_i = x_i - xbar) and proposals are shifted the same way in K1
    // (mu~ = theta' - xbar): (x_i - mu) = (x~_i - mu~), but every term of the expanded quadratic form
    //   sum_i x~_i' A^-1 x~_i  -  2 y . sum_i x~_i  +  N mu~' A^-1 mu~ ,   y = A^-1 mu~
    // is then O(N d) whatever the offset of the data, so the expansion loses no digits to cancellation.
    // data-only constants: c1 = sum_i x~_i' A^-1 x~_i (A = I for ISO), sx = sum_i x~_i (~ 0)
    m.xbar.assign(d, 0.0);
    for (long long i = 0; i < N; ++i)
        for (int k = 0; k < d; ++k) m.xbar[k] += data[i * d + k];
    for (int k = 0; k < d; ++k) m.xbar[k] /= (double)N;
    std::vector<double> xc((size_t)N * d);
    for (long long i = 0; i < N; ++i)
        for (int k = 0; k < d; ++k) xc[(size_t)i * d + k] = data[i * d + k] - m.xbar[k];
    data = xc.data();
    m.sx.assign(d, 0.0);
    double c1 = 0.0;
    for (long long i = 0; i < N; ++i) {
        const double* x = data + i * d;
        double q = 0.0;
        if (family == DEMC_FAM_MVN_FULL) {
            for (int r = 0; r < d; ++r) {
                double sr = 0.0;
                for (int k = 0; k < d; ++k) sr += Ainv[r * d + k] * x[k];
                q += x[r] * sr;
            }
        } else
            for (int k = 0; k < d; ++k) q += x[k] * x[k];
        c1 += q;
        for (int k = 0; k < d; ++k) m.sx[k] += x[k];
    }
    m.c1 = c1;
    // fragment-ordered copy of X for v_mfma_f64_16x16x4_f64's B operand:
    //   Xf[tile][kstep][lane] = X[16*tile + (lane&15)][4*kstep + (lane>>4)], zero padded
    const int ksx = m.dpad / 4;
    m.Xf.assign(((size_t)m.n_tiles + 1) * ksx * 64, 0.0);  // +1: the all-zero tail tile
    for (long long tI = 0; tI < m.n_tiles; ++tI)
        for (int ks = 0; ks < ksx; ++ks)
            for (int l = 0; l < 64; ++l) {
                const long long i = 16 * tI + (l & 15);
                const int k = 4 * ks + (l >> 4);
                if (i < N && k < d) m.Xf[((size_t)tI * ksx + ks) * 64 + l] = data[i * d + k];
            }
    if (direct) {
        // whitened, centred observations z_i = L^-1 x~_i (ISO: x~_i), rows padded with zeros to DP scalars
        m.dp_direct = d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64;
        const int DP = m.dp_direct;
        m.data.assign((size_t)N * DP, 0.0);
        for (long long i = 0; i < N; ++i) {
            const double* x = data + i * d;
            double* zr = m.data.data() + (size_t)i * DP;
            if (family == DEMC_FAM_MVN_FULL) {
                for (int r = 0; r < d; ++r) {
                    double sr = 0.0;
                    for (int k = 0; k <= r; ++k) sr += Linv[(size_t)r * d + k] * x[k];
                    zr[r] = sr;
                }
            } else
                for (int k = 0; k < d; ++k) zr[k] = x[k];
        }
    }
    return {};
}

// demc_set_model's arguments (ndims in [0, 4]: the entry point checks the call's shape) with the handle's D and likelihood mode.
inline PreparedModel prepare_model(int family, int D, int loglike_mode, const double* data, const int64_t* dims, int ndims,
                                   const double* hyper, int nhyper) {
    long long dm[4] = {0, 0, 0, 0};
    for (int i = 0; i < ndims && i < 4; ++i) dm[i] = dims[i];
    PreparedModel m;
    Refusal r;
    switch (family) {
        case DEMC_FAM_GAUSSIAN: r = prep_gaussian(m, D, data, dm); break;
        case DEMC_FAM_BINOMIAL: r = prep_binomial(m, D, data, dm); break;
        case DEMC_FAM_HIER_BINOMIAL: r = prep_hier_binomial(m, D, data, dm, hyper, nhyper); break;
        case DEMC_FAM_HIER_GAUSSIAN: r = prep_hier_gaussian(m, D, data, dm); break;
        case DEMC_FAM_LBA:
        case DEMC_FAM_LNR: r = prep_race(m, family, D, data, dm, hyper, nhyper); break;
        case DEMC_FAM_RASTRIGIN: m.N = 1; break;
        case DEMC_FAM_ODE_LV: r = prep_ode_lv(m, D, data, dm, ndims, hyper, nhyper); break;
        case DEMC_FAM_MVN_ISO:
        case DEMC_FAM_MVN_FULL: r = prep_mvn(m, family, D, loglike_mode == DEMC_LOGLIKE_DIRECT, data, dm, hyper, nhyper); break;
        default: r = {DEMC_EUNSUPPORTED, "model family is not registered; arbitrary closures cannot run on the device"};
    }
    if (r) {
        m = PreparedModel{};
        m.refused = r;
    }
    return m;
}

// ---- demc_set_model_sim ------------------------------------------------------------------------------------------------------

struct PreparedSim {
    Refusal refused;
    int kmax = 0;                // KDE_CHOICE: the largest observed choice
    std::vector<double> hyper;   // as the kernels see it: [bandwidth, the simulator's own ...], at least the bandwidth
    double sim_bw = 0.0;
    std::vector<double> logtab;  // FREQUENCY: [n_sim + 1] log(c / n_sim)
};

// demc_set_model_sim's arguments with the handle's D.  hyper[0] = the KDE bandwidth (<= 0 or absent: the rule of thumb), hyper[1..]
// the simulator's own hyper-parameters.  DEMC_SIMEST_KDE_CHOICE: data = the n_obs choices, then the n_obs response times.
inline PreparedSim prepare_sim(int D, int simulator, int estimator, int64_t n_sim, const char* source, const double* data,
                               int64_t n_obs, const double* hyper, int nhyper) {
    auto refuse = [](const std::string& msg) {
        PreparedSim r;
        r.refused = {DEMC_EINVAL, msg};
        return r;
    };
    if (simulator != DEMC_SIM_NORMAL && simulator != DEMC_SIM_BINOMIAL && simulator != DEMC_SIM_LNR && simulator != DEMC_SIM_USER)
        return refuse("demc_set_model_sim: unknown simulator");
    if (estimator != DEMC_SIMEST_KDE_EPANECHNIKOV && estimator != DEMC_SIMEST_FREQUENCY && estimator != DEMC_SIMEST_KDE_CHOICE)
        return refuse("demc_set_model_sim: unknown estimator");
    const bool pairs = estimator == DEMC_SIMEST_KDE_CHOICE;
    if (simulator == DEMC_SIM_LNR && !pairs)
        return refuse(std::string("demc_set_model_sim: DEMC_SIM_LNR simulates (choice, time) pairs and cannot be scored by the scalar estimator ") +
                      (estimator == DEMC_SIMEST_FREQUENCY ? "DEMC_SIMEST_FREQUENCY" : "DEMC_SIMEST_KDE_EPANECHNIKOV") + " (use DEMC_SIMEST_KDE_CHOICE)");
    if (pairs && (simulator == DEMC_SIM_NORMAL || simulator == DEMC_SIM_BINOMIAL))
        return refuse(std::string("demc_set_model_sim: ") + (simulator == DEMC_SIM_NORMAL ? "DEMC_SIM_NORMAL" : "DEMC_SIM_BINOMIAL") +
                      " simulates scalars and cannot be scored by DEMC_SIMEST_KDE_CHOICE (use DEMC_SIM_LNR or a user simulator of pairs)");
    if (n_sim < 2) return refuse("demc_set_model_sim: n_sim < 2 (a density estimate needs at least two simulated values)");
    const int64_t cap = pairs ? kPrepSimChoiceMaxN : kPrepSimMaxN;
    if (n_sim > cap)
        return refuse("demc_set_model_sim: n_sim = " + std::to_string(n_sim) + " is above the cap of " + std::to_string(cap) +
                      " simulated values (the sample of a proposal is held in LDS)");
    if (n_obs < 1 || !data) return refuse("demc_set_model_sim: n_obs >= 1 observations required");
    if (nhyper < 0 || (nhyper > 0 && !hyper)) return refuse("demc_set_model_sim: nhyper > 0 without hyper");
    if (simulator == DEMC_SIM_USER && (!source || !source[0]))
        return refuse("demc_set_model_sim: DEMC_SIM_USER needs hip_source (a definition of demc_user_sim; demc_user_sim_choice under DEMC_SIMEST_KDE_CHOICE)");
    if (simulator != DEMC_SIM_USER && source && source[0])
        return refuse("demc_set_model_sim: hip_source given with a registered simulator");
    if (simulator == DEMC_SIM_NORMAL && D != 2) return refuse("SIM_NORMAL: theta=(mu,sigma)");
    if (simulator == DEMC_SIM_BINOMIAL) {
        if (D != 1) return refuse("SIM_BINOMIAL: theta=p");
        if (nhyper < 2 || !(hyper[1] >= 1.0 && hyper[1] <= 1024.0 && hyper[1] == std::floor(hyper[1])))
            return refuse("SIM_BINOMIAL: hyper=[bandwidth, n_trials], n_trials an integer in [1, 1024]");
        if (n_sim * (((int64_t)hyper[1] + 3) / 4) > 0x7fffffffLL) return refuse("SIM_BINOMIAL: too many Philox blocks per proposal");
    }
    if (simulator == DEMC_SIM_LNR) {
        if (D < 3 || D > 9) return refuse("SIM_LNR: theta=(nu[K],tau), K = D - 1 in [2, 8]");
        if (nhyper < 2 || !(hyper[1] > 0.0)) return refuse("SIM_LNR: hyper=[bandwidth, sigma], sigma > 0");
    }
    PreparedSim s;
    if (pairs) {  // host_data = the n_obs choices, then the n_obs times
        const int hi = simulator == DEMC_SIM_LNR ? D - 1 : 255;
        for (int64_t j = 0; j < n_obs; ++j) {
            const double c = data[j];
            if (!(c >= 1.0 && c <= (double)hi && c == std::floor(c)))
                return refuse("demc_set_model_sim: the choice of observation " + std::to_string(j) + " is not an integer in [1, " + std::to_string(hi) + "]");
            if (!std::isfinite(data[n_obs + j]))
                return refuse("demc_set_model_sim: the response time of observation " + std::to_string(j) + " is not finite");
            s.kmax = std::max(s.kmax, (int)c);
        }
    }
    if (estimator == DEMC_SIMEST_FREQUENCY)
        for (int64_t j = 0; j < n_obs; ++j)
            if (!(data[j] == std::floor(data[j])))
                return refuse("demc_set_model_sim: the FREQUENCY estimator needs integer-valued data (observation " + std::to_string(j) + " is not)");
    s.hyper.assign((size_t)(nhyper > 0 ? nhyper : 1), 0.0);
    for (int i = 0; i < nhyper; ++i) s.hyper[(size_t)i] = hyper[i];
    s.sim_bw = s.hyper[0] > 0.0 ? s.hyper[0] : 0.0;
    if (estimator == DEMC_SIMEST_FREQUENCY) {
        s.logtab.resize((size_t)n_sim + 1);
        for (int64_t c = 0; c <= n_sim; ++c) s.logtab[(size_t)c] = std::log((double)c / (double)n_sim);  // (log 0 = -Inf: a count of zero)
    }
    return s;
}

// ---- demc_set_priors / demc_set_bounds / demc_set_blocks ---------------------------------------------------------------------

// DEMC_PRIOR_TRUNCNORMAL: log(Phi((hi - a) / b) - Phi((lo - a) / b)), the mass of Normal(a, b) between the bounds of scalar j, from
// erfc on the side of the mean where the difference does not cancel (both bounds above the mean: the upper tails).  DEMC_EINVAL
// when the bounds are empty or the mass is 0 or not finite -- the density would be a division by it.
inline Refusal truncnormal_log_mass(size_t j, double a, double b, double lo, double hi, double* out) {
    const std::string who = "DEMC_PRIOR_TRUNCNORMAL, scalar " + std::to_string(j) + ": ";
    if (!(std::isfinite(a) && std::isfinite(b) && b > 0.0)) return {DEMC_EINVAL, who + "Normal(a, b) needs a finite a and a finite b > 0"};
    if (!(lo < hi)) return {DEMC_EINVAL, who + "the bounds lo >= hi leave nothing to truncate to"};
    const double zl = (lo - a) / b, zh = (hi - a) / b, r = std::sqrt(0.5);
    // Phi(z) = erfc(-z / sqrt 2) / 2; 1 - Phi(z) = erfc(z / sqrt 2) / 2
    const double mass = zl > 0.0 ? 0.5 * (std::erfc(zl * r) - std::erfc(zh * r)) : 0.5 * (std::erfc(-zh * r) - std::erfc(-zl * r));
    if (!(mass > 0.0) || !std::isfinite(mass)) return {DEMC_EINVAL, who + "the mass of the Normal between the bounds is 0 or not finite"};
    *out = std::log(mass);
    return {};
}

// The table entry of scalar j: prior `kind`(a, b[, theta[ref]]) -- a DEMC_PRIOR_* kind of the C-ABI -- under the bounds in force.
// truncated(Normal(a, b), lo, hi) is the device's Normal entry, its constant lowered by the log of the mass between the bounds.
inline Refusal prior_entry(size_t j, int kind, double a, double b, int ref, double lo, double hi, DimTab* out) {
    const bool trunc = kind == DEMC_PRIOR_TRUNCNORMAL;
    const int kd = trunc ? (int)PR_NORMAL : kind;
    DimTab t;
    t.lo = lo;
    t.hi = hi;
    t.kind = kd;
    t.ref = ref;
    t.a = a;
    // reciprocal scale for the location-scale families: no FP64 division per scalar in the kernels
    const bool recip = kd == PR_NORMAL || kd == PR_HALFCAUCHY || kd == PR_GAMMA ||
                       kd == PR_EXPONENTIAL || kd == PR_LOGNORMAL || kd == PR_CAUCHY;
    t.b = recip ? 1.0 / b : b;
    t.c = prior_const(kd, a, b);
    if (trunc) {
        double lm = 0.0;
        if (Refusal r = truncnormal_log_mass(j, a, b, lo, hi, &lm)) return r;
        t.c -= lm;
    }
    *out = t;
    return {};
}

// demc_set_priors: every entry of `tab` (which holds the bounds in force) formed again from kind / a / b / ref (a, b, ref may be
// null: 0, 1, 0).  trunc_sd[j] keeps the scale of a truncated Normal (0: the scalar has none), for prepare_bounds.  A refused call
// leaves tab and trunc_sd as they were.
inline Refusal prepare_priors(std::vector<DimTab>& tab, std::vector<double>& trunc_sd, const int32_t* kind, const double* a,
                              const double* b, const int32_t* ref) {
    const size_t D = tab.size();
    for (size_t j = 0; j < D; ++j) {
        if (kind[j] < 0 || kind[j] > DEMC_PRIOR_TRUNCNORMAL) return {DEMC_EUNSUPPORTED, "prior kind not registered"};
        if (kind[j] == DEMC_PRIOR_NORMAL_REF && (!ref || ref[j] < 0 || ref[j] >= (int)D)) return {DEMC_EINVAL, "prior ref out of range"};
    }
    std::vector<DimTab> t(D);
    std::vector<double> sd(D, 0.0);
    for (size_t j = 0; j < D; ++j) {
        const double bj = b ? b[j] : 1.0;
        if (Refusal r = prior_entry(j, kind[j], a ? a[j] : 0.0, bj, ref ? ref[j] : 0, tab[j].lo, tab[j].hi, &t[j])) return r;
        if (kind[j] == DEMC_PRIOR_TRUNCNORMAL) sd[j] = bj;
    }
    tab.swap(t);
    trunc_sd.swap(sd);
    return {};
}

// demc_set_bounds: the bounds of every entry replaced; a truncated Normal's constant holds the mass between them, so that entry is
// formed again -- priors and bounds arrive in either order.  A refused call leaves tab as it was.
inline Refusal prepare_bounds(std::vector<DimTab>& tab, const std::vector<double>& trunc_sd, const double* lo, const double* hi) {
    std::vector<DimTab> t = tab;
    for (size_t j = 0; j < t.size(); ++j) {
        t[j].lo = lo[j];
        t[j].hi = hi[j];
        if (j < trunc_sd.size() && trunc_sd[j] != 0.0)
            if (Refusal r = prior_entry(j, DEMC_PRIOR_TRUNCNORMAL, t[j].a, trunc_sd[j], t[j].ref, lo[j], hi[j], &t[j])) return r;
    }
    tab.swap(t);
    return {};
}

// Run-length form of the table: consecutive scalars with byte-identical entries share a segment.  More than kMaxDimSeg segments:
// n_seg = 0, the kernels read the table itself.
struct SegTable {
    DimSeg segs[kMaxDimSeg];
    int n_seg = 0;
    int seg_start[kMaxDimSeg] = {0};
    unsigned seg_plain = 0;  // segments with a flat / Normal / Normal(a, theta[ref]) prior
};

inline SegTable encode_segments(const std::vector<DimTab>& tab) {
    SegTable s;
    std::memset(s.segs, 0, sizeof s.segs);
    int n = 0;
    for (size_t j = 0; j < tab.size(); ++j) {
        if (j == 0 || std::memcmp(&tab[j], &tab[j - 1], sizeof(DimTab)) != 0) {
            if (n == kMaxDimSeg) { n = -1; break; }
            s.segs[n].start = (int)j;
            s.segs[n].t = tab[j];
            ++n;
        }
    }
    s.n_seg = n > 0 ? n : 0;
    for (int q = 0; q < kMaxDimSeg; ++q) {
        s.seg_start[q] = q < s.n_seg ? s.segs[q].start : 0;
        const int kd = s.segs[q].t.kind;
        if (q < s.n_seg && (kd == PR_FLAT || kd == PR_NORMAL || kd == PR_NORMAL_REF)) s.seg_plain |= 1u << q;
    }
    return s;
}

// Run-length form of one block mask (kernarg table of the long-row kernel): the runs' first scalars, bit q of `in` set when run q
// lies inside the block.  n = 0: more runs than kMaxMaskRun.
struct MaskRuns { int n = 0; unsigned in = 0; int start[kMaxMaskRun] = {0}; };

inline MaskRuns encode_mask(const uint8_t* mk, int D) {
    MaskRuns mr;
    for (int j = 0; j < D; ++j)
        if (j == 0 || (mk[j] != 0) != (mk[j - 1] != 0)) {
            if (mr.n == kMaxMaskRun) return MaskRuns();
            mr.start[mr.n] = j;
            if (mk[j]) mr.in |= 1u << mr.n;
            ++mr.n;
        }
    return mr;
}

}  // namespace demc
