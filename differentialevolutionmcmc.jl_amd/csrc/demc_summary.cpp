// demc_summary.cpp -- the kernels of demc_summarize (demc_summary.hpp) and the host code that strings them together, in a
// translation unit of their own: the other code objects of the library do not change when this one does.
#define DEMC_SUMMARY_KERNELS
#include "demc_summary.hpp"

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, finish

namespace demc {

namespace {

template <bool LDS>
int launch_all(SumKParams& p, const SummaryPlan& plan, hipStream_t st, std::string& err) {
    const void* fns[3] = {(const void*)k_sum_moments<LDS, 0>, (const void*)k_sum_moments<LDS, 1>, (const void*)k_sum_acf<LDS>};
    for (const void* f : fns)  // (per function, not per call: always the same ceiling)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSumLdsMax) != hipSuccess) {
            err = "demc_summarize: the LDS limit of a kernel could not be raised";
            return DEMC_EHIP;
        }
    const int D2 = p.D + 2, workers = plan.workers;
    const size_t lds = plan.lds_bytes;
    const dim3 grid((unsigned)workers, (unsigned)plan.tiles);
    const long long cells = p.n * p.P;
    hipLaunchKernelGGL(k_sum_invmap, dim3((unsigned)std::min<long long>((cells + 255) / 256, 65536)), dim3(256), 0, st, p);
    hipLaunchKernelGGL((k_sum_moments<LDS, 0>), grid, dim3(kSumWG), lds, st, p);
    hipLaunchKernelGGL(k_sum_means, dim3((unsigned)D2), dim3(256), 0, st, p, workers);
    hipLaunchKernelGGL((k_sum_moments<LDS, 1>), grid, dim3(kSumWG), lds, st, p);
    for (int b = 0; b < plan.lag_blocks; ++b) {  // a block whose series have all ended costs two launches that return at once
        hipLaunchKernelGGL((k_sum_acf<LDS>), grid, dim3(kSumWG), lds, st, p, b * kSumLagBlock);
        hipLaunchKernelGGL(k_sum_geyer, dim3((unsigned)D2), dim3(kSumLagBlock), 0, st, p, b * kSumLagBlock, workers);
    }
    hipLaunchKernelGGL(k_sum_final, dim3((unsigned)((D2 + 63) / 64)), dim3(64), 0, st, p, workers);
    return DEMC_OK;
}

}  // namespace

int summary_enqueue(const char* who, const HistView& v, const SummaryPlan& plan, hipStream_t st, Scratch& s, SumKParams& p, std::string& err) {
    p = SumKParams{};
    p.hist = v.hist; p.acc = v.acc; p.lp = v.lp; p.idh = v.idh;
    p.P = v.P; p.row0 = v.row0; p.n = v.row1 - v.row0; p.h = plan.h; p.id0 = v.id0;
    p.D = v.D; p.ld = v.ld; p.JT = plan.JT; p.L = plan.L; p.rho_cols = plan.rho_cols;
    const int D2 = v.D + 2;

    double* small = nullptr;  // mean | bh | W | vplus | p_prev | p_sum | out[6]: one allocation, one fill
    int* flags = nullptr;     // K | stopped
    bool ok = s.get(&p.inv, plan.n_inv) && s.get(&p.mu, plan.n_mu) && s.get(&p.part_sum, plan.n_part) && s.get(&p.part_ss, plan.n_part) &&
              s.get(&p.part_g, plan.n_part_g) && s.get(&small, plan.n_small) && s.get(&flags, plan.n_flags);
    if (ok && !plan.lds) ok = s.get(&p.xg, plan.n_xg);
    if (ok && plan.rho_cols > 0) ok = s.get(&p.rho, plan.n_rho);
    if (!ok) { err = std::string(who) + ": out of device memory for the scratch buffers"; return DEMC_ENOMEM; }
    p.mean = small; p.bh = small + D2; p.W = small + 2 * D2; p.vplus = small + 3 * D2; p.p_prev = small + 4 * D2;
    p.p_sum = small + 5 * D2; p.out = small + 6 * D2;
    p.K = flags; p.stopped = flags + D2;
    hipError_t e = hipMemsetAsync(p.inv, 0, plan.n_inv * sizeof(int), st);  // (an id out of range leaves a valid slot behind)
    if (e == hipSuccess) e = hipMemsetAsync(small, 0, plan.n_small * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, plan.n_flags * sizeof(int), st);
    if (e == hipSuccess && p.rho) e = hipMemsetAsync(p.rho, 0xFF, plan.n_rho * sizeof(double), st);  // all ones: a NaN
    if (!hip_ok(who, e, err)) return DEMC_EHIP;
    return plan.lds ? launch_all<true>(p, plan, st, err) : launch_all<false>(p, plan, st, err);
}

int summary_run(const HistView& v, const SummaryPlan& plan, hipStream_t st, double* out, double* rho_out, long long rho_len, std::string& err) {
    const char* who = "demc_summarize";
    const int D2 = v.D + 2;
    Scratch s;
    SumKParams p;
    const int rc = summary_enqueue(who, v, plan, st, s, p, err);
    if (rc != DEMC_OK) return rc;
    std::vector<double> rho_host(p.rho ? plan.n_rho : 0);
    if (!finish(who, st, {{out, p.out, (size_t)D2 * 6 * sizeof(double)}, {p.rho ? rho_host.data() : nullptr, p.rho, plan.n_rho * sizeof(double)}}, err))
        return DEMC_EHIP;
    if (rho_out) {  // lags the call did not evaluate (past the lag cap, or the whole row when h < 2) are NaN
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int j = 0; j < D2; ++j)
            for (long long t = 0; t < rho_len; ++t)
                rho_out[(size_t)j * rho_len + t] = t < p.rho_cols ? rho_host[(size_t)j * p.rho_cols + t] : nan;
    }
    return DEMC_OK;
}

}  // namespace demc
