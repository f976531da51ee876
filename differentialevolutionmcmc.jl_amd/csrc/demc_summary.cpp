// demc_summary.cpp -- the kernels of demc_summarize (demc_summary.hpp) and the host code that strings them together, in a
// translation unit of their own: the other code objects of the library do not change when this one does.
#define DEMC_SUMMARY_KERNELS
#include "demc_summary.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch

namespace demc {

namespace {

template <bool LDS>
int launch_all(SumKParams& p, int workers, int n_jt, size_t lds, int n_blocks, hipStream_t st, std::string& err) {
    const void* fns[3] = {(const void*)k_sum_moments<LDS, 0>, (const void*)k_sum_moments<LDS, 1>, (const void*)k_sum_acf<LDS>};
    for (const void* f : fns)  // (per function, not per call: always the same ceiling)
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSumLdsMax) != hipSuccess) {
            err = "demc_summarize: the LDS limit of a kernel could not be raised";
            return DEMC_EHIP;
        }
    const int D2 = p.D + 2;
    const dim3 grid((unsigned)workers, (unsigned)n_jt);
    const long long cells = p.n * p.P;
    hipLaunchKernelGGL(k_sum_invmap, dim3((unsigned)std::min<long long>((cells + 255) / 256, 65536)), dim3(256), 0, st, p);
    hipLaunchKernelGGL((k_sum_moments<LDS, 0>), grid, dim3(kSumWG), lds, st, p);
    hipLaunchKernelGGL(k_sum_means, dim3((unsigned)D2), dim3(256), 0, st, p, workers);
    hipLaunchKernelGGL((k_sum_moments<LDS, 1>), grid, dim3(kSumWG), lds, st, p);
    for (int b = 0; b < n_blocks; ++b) {  // a block whose series have all ended costs two launches that return at once
        hipLaunchKernelGGL((k_sum_acf<LDS>), grid, dim3(kSumWG), lds, st, p, b * kSumLagBlock);
        hipLaunchKernelGGL(k_sum_geyer, dim3((unsigned)D2), dim3(kSumLagBlock), 0, st, p, b * kSumLagBlock, workers);
    }
    hipLaunchKernelGGL(k_sum_final, dim3((unsigned)((D2 + 63) / 64)), dim3(64), 0, st, p, workers);
    return DEMC_OK;
}

}  // namespace

int summary_run(const SumArgs& a, hipStream_t st, double* out, double* rho_out, long long rho_len, std::string& err) {
    SumKParams p{};
    p.hist = a.hist; p.acc = a.acc; p.lp = a.lp; p.idh = a.idh;
    p.P = a.P; p.row0 = a.row0; p.n = a.row1 - a.row0; p.h = p.n / 2; p.id0 = a.id0;
    p.D = a.D; p.ld = a.ld;
    const int D2 = a.D + 2;
    const long long n = p.n, h = p.h;
    if (h - 1 > (long long)std::numeric_limits<int>::max() / 2) { err = "demc_summarize: too many rows"; return DEMC_EINVAL; }
    p.L = h >= 2 ? (int)(a.max_lag > 0 ? std::min<long long>(h - 1, a.max_lag) : h - 1) : -1;
    const int n_blocks = h >= 2 ? p.L / kSumLagBlock + 1 : 0;
    // geometry: as many series per tile as kSumLdsSmall holds (<= kSumMaxJT), one series while it fits in kSumLdsMax, a global
    // tile per (worker, series) beyond that
    const size_t per_series = ((size_t)n + 2 * kSumLagBlock) * sizeof(double);
    int workers = (int)std::min<long long>(a.P, kSumMaxWorkers);
    bool lds_mode = true;
    if (per_series <= kSumLdsSmall) p.JT = (int)std::min<size_t>(std::min(D2, kSumMaxJT), kSumLdsSmall / per_series);
    else if (per_series <= kSumLdsMax) p.JT = 1;
    else {
        p.JT = 1;
        lds_mode = false;
        workers = (int)std::max<size_t>(1, std::min<size_t>((size_t)workers, kSumGlobalTile / ((size_t)n * D2 * sizeof(double))));
    }
    const int n_jt = (D2 + p.JT - 1) / p.JT;
    const size_t lds = lds_mode ? (size_t)p.JT * per_series : (size_t)2 * kSumLagBlock * sizeof(double);
    p.rho_cols = rho_out ? std::min<long long>(rho_len, (long long)p.L + 1) : 0;
    if (p.rho_cols < 0) p.rho_cols = 0;

    Scratch s;
    double* small = nullptr;  // mean | bh | W | vplus | p_prev | p_sum | out[6]: one allocation, one fill
    int* flags = nullptr;     // K | stopped
    bool ok = s.get(&p.inv, (size_t)n * a.P) && s.get(&p.mu, (size_t)D2 * 2 * a.P) && s.get(&p.part_sum, (size_t)workers * D2) &&
              s.get(&p.part_ss, (size_t)workers * D2) && s.get(&p.part_g, (size_t)workers * D2 * kSumLagBlock) &&
              s.get(&small, (size_t)D2 * 12) && s.get(&flags, (size_t)D2 * 2);
    if (ok && !lds_mode) ok = s.get(&p.xg, (size_t)workers * D2 * n);
    if (ok && p.rho_cols > 0) ok = s.get(&p.rho, (size_t)D2 * p.rho_cols);
    if (!ok) { err = "demc_summarize: out of device memory for the scratch buffers"; return DEMC_ENOMEM; }
    p.mean = small; p.bh = small + D2; p.W = small + 2 * D2; p.vplus = small + 3 * D2; p.p_prev = small + 4 * D2;
    p.p_sum = small + 5 * D2; p.out = small + 6 * D2;
    p.K = flags; p.stopped = flags + D2;
    hipError_t e = hipMemsetAsync(p.inv, 0, (size_t)n * a.P * sizeof(int), st);  // (an id out of range leaves a valid slot behind)
    if (e == hipSuccess) e = hipMemsetAsync(small, 0, (size_t)D2 * 12 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, (size_t)D2 * 2 * sizeof(int), st);
    if (e == hipSuccess && p.rho) e = hipMemsetAsync(p.rho, 0xFF, (size_t)D2 * p.rho_cols * sizeof(double), st);  // all ones: a NaN
    if (e != hipSuccess) { err = std::string("demc_summarize: ") + hipGetErrorString(e); return DEMC_EHIP; }
    const int rc = lds_mode ? launch_all<true>(p, workers, n_jt, lds, n_blocks, st, err) : launch_all<false>(p, workers, n_jt, lds, n_blocks, st, err);
    if (rc != DEMC_OK) return rc;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(out, p.out, (size_t)D2 * 6 * sizeof(double), hipMemcpyDeviceToHost);
    std::vector<double> rho_host;
    if (e == hipSuccess && p.rho) {
        rho_host.resize((size_t)D2 * p.rho_cols);
        e = hipMemcpy(rho_host.data(), p.rho, rho_host.size() * sizeof(double), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) { err = std::string("demc_summarize: ") + hipGetErrorString(e); return DEMC_EHIP; }
    if (rho_out) {  // lags the call did not evaluate (past the lag cap, or the whole row when h < 2) are NaN
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int j = 0; j < D2; ++j)
            for (long long t = 0; t < rho_len; ++t)
                rho_out[(size_t)j * rho_len + t] = t < p.rho_cols ? rho_host[(size_t)j * p.rho_cols + t] : nan;
    }
    return DEMC_OK;
}

}  // namespace demc
