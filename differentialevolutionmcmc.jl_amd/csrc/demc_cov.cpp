// demc_cov.cpp -- the kernels of demc_covariance (demc_cov.hpp) and the host code that strings them together, in a translation
// unit of their own: the other code objects of the library do not change when this one does.
#define DEMC_COV_KERNELS
#include "demc_cov.hpp"

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, PassTrace, finish

namespace demc {

namespace {

template <int NB>
void launch_syrk(const CovKParams& p, hipStream_t st) {
    hipLaunchKernelGGL((k_cov_syrk<NB>), dim3((unsigned)p.W), dim3(kCovWG), 0, st, p);
}

}  // namespace

int cov_run(const HistView& v, const CovPlan& plan, hipStream_t st, double* mean_out, double* cov_out, double* cor_out, std::string& err) {
    const char* who = "demc_covariance";
    const int K = plan.K;
    CovKParams p{};
    p.hist = v.hist + (size_t)v.row0 * v.P * v.ld;
    p.acc = v.acc + (size_t)v.row0 * v.P;
    p.lp = v.lp + (size_t)v.row0 * v.P;
    p.N = (v.row1 - v.row0) * v.P; p.D = v.D; p.ld = v.ld; p.K = K;
    p.W = plan.W;
    Scratch s;
    int* d_cols = nullptr;
    if (!(s.get(&d_cols, plan.n_cols) && s.get(&p.part1, plan.n_part1) && s.get(&p.mhat, plan.n_mhat) && s.get(&p.part2, plan.n_part2) &&
          s.get(&p.mean, plan.n_mean) && s.get(&p.cov, plan.n_mat) && s.get(&p.cor, plan.n_mat))) {
        err = "demc_covariance: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    p.cols = d_cols;
    if (!hip_ok(who, hipMemcpyAsync(d_cols, plan.table, sizeof plan.table, hipMemcpyHostToDevice, st), err)) return DEMC_EHIP;
    PassTrace tr;  // (the diagnostic variant: device time of the three passes)
    bool ok = tr.mark(st);
    hipLaunchKernelGGL(k_cov_mean, dim3((unsigned)p.W), dim3(kCovWG), 0, st, p);
    hipLaunchKernelGGL(k_cov_mean_final, dim3(1), dim3(kCovMaxCols), 0, st, p);
    ok = ok && tr.mark(st);
    switch (plan.NB) {
        case 1: launch_syrk<1>(p, st); break;
        case 2: launch_syrk<2>(p, st); break;
        case 3: launch_syrk<3>(p, st); break;
        default: launch_syrk<4>(p, st); break;
    }
    ok = ok && tr.mark(st);
    hipLaunchKernelGGL(k_cov_final, dim3(1), dim3(kCovFinalWG), 0, st, p);
    ok = ok && tr.mark(st);
    if (!ok) { err = "demc_covariance: an event could not be recorded"; return DEMC_EHIP; }
    const size_t mat = plan.n_mat * sizeof(double);
    if (!finish(who, st, {{mean_out, p.mean, plan.n_mean * sizeof(double)}, {cov_out, p.cov, mat}, {cor_out, p.cor, mat}}, err)) return DEMC_EHIP;
    tr.print(who, 3, 1);
    return DEMC_OK;
}

}  // namespace demc
