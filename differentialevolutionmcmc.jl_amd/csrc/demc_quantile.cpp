// demc_quantile.cpp -- the kernels of demc_quantiles (demc_quantile.hpp) and the host code that strings them together, in a
// translation unit of their own: the other code objects of the library do not change when this one does.
#define DEMC_QUANTILE_KERNELS
#include "demc_quantile.hpp"

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, PassTrace, finish

namespace demc {

int quantile_run(const HistView& v, const QuantilePlan& plan, hipStream_t st, double* out, std::string& err) {
    const char* who = "demc_quantiles";
    const int D2 = v.D + 2, n_probs = plan.tg.n_probs;
    QKParams p{};
    p.hist = v.hist; p.acc = v.acc; p.lp = v.lp;
    p.P = v.P; p.row0 = v.row0; p.n = v.row1 - v.row0; p.D = v.D; p.ld = v.ld; p.T = plan.T;
    Scratch s;
    const size_t cells = plan.n_cells;
    if (!(s.get(&p.table, plan.n_table) && s.get(&p.gprefix, cells) && s.get(&p.trank, cells) && s.get(&p.tgrp, cells) && s.get(&p.ng, plan.n_series) &&
          s.get(&p.nanflag, plan.n_series) && s.get(&p.out, plan.n_out))) {
        err = "demc_quantiles: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    if (!hip_ok(who, hipMemsetAsync(p.table, 0, plan.n_table * sizeof(unsigned long long), st), err)) return DEMC_EHIP;
    PassTrace tr;  // (the diagnostic variant: device time of every histogram pass)
    hipLaunchKernelGGL(k_q_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p, plan.tg);
    for (const void* f : {(const void*)k_q_hist<true>, (const void*)k_q_hist<false>})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_max) != hipSuccess) {
            err = "demc_quantiles: the LDS limit of a kernel could not be raised";
            return DEMC_EHIP;
        }
    for (int i = 0; i < kQPasses; ++i) {
        const int shift = 64 - kQBits * (i + 1);
        p.slots = plan.slots[i];
        const size_t lds = plan.lds_bytes[i];
        if (!tr.mark(st)) { err = "demc_quantiles: an event could not be recorded"; return DEMC_EHIP; }
        if (i == 0) hipLaunchKernelGGL((k_q_hist<true>), dim3((unsigned)plan.W), dim3(kQWG), lds, st, p, shift);
        else hipLaunchKernelGGL((k_q_hist<false>), dim3((unsigned)plan.W), dim3(kQWG), lds, st, p, shift);
        if (!tr.mark(st)) { err = "demc_quantiles: an event could not be recorded"; return DEMC_EHIP; }
        hipLaunchKernelGGL(k_q_scan, dim3((unsigned)D2), dim3(256), 0, st, p, shift);
    }
    hipLaunchKernelGGL(k_q_final, dim3((unsigned)((plan.n_out + 255) / 256)), dim3(256), 0, st, p, plan.tg);
    if (!finish(who, st, {{out, p.out, plan.n_out * sizeof(double)}}, err)) return DEMC_EHIP;
    tr.print(who, kQPasses, 2);
    return DEMC_OK;
}

}  // namespace demc
