// demc_cov.cpp -- the kernels of demc_covariance (demc_cov.hpp) and the host code that strings them together, in a translation
// unit of their own: the other code objects of the library do not change when this one does.
#define DEMC_COV_KERNELS
#include "demc_cov.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, Event

namespace demc {

namespace {

template <int NB>
void launch_syrk(const CovKParams& p, hipStream_t st) {
    hipLaunchKernelGGL((k_cov_syrk<NB>), dim3((unsigned)p.W), dim3(kCovWG), 0, st, p);
}

}  // namespace

int cov_run(const CovArgs& a, hipStream_t st, const int* cols, int K, double* mean_out, double* cov_out, double* cor_out, std::string& err) {
    const long long N = (a.row1 - a.row0) * a.P;
    // geometry (demc_cov.hpp): a chunk is kCovChunk cells, worker b takes the chunks b, b + W, ...
    const long long chunks = (N + kCovChunk - 1) / kCovChunk;
    const int NB = (K + 15) / 16;

    CovKParams p{};
    p.hist = a.hist + (size_t)a.row0 * a.P * a.ld;
    p.acc = a.acc + (size_t)a.row0 * a.P;
    p.lp = a.lp + (size_t)a.row0 * a.P;
    p.N = N; p.D = a.D; p.ld = a.ld; p.K = K;
    p.W = (int)std::min<long long>(chunks, kCovMaxWorkers);
    int table[kCovMaxCols];
    for (int k = 0; k < kCovMaxCols; ++k) table[k] = k < K ? cols[k] : -1;
    Scratch s;
    int* d_cols = nullptr;
    if (!(s.get(&d_cols, (size_t)kCovMaxCols) && s.get(&p.part1, (size_t)p.W * kCovMaxCols) && s.get(&p.mhat, (size_t)kCovMaxCols) &&
          s.get(&p.part2, (size_t)p.W * cov_partial(NB)) && s.get(&p.mean, (size_t)K) && s.get(&p.cov, (size_t)K * K) &&
          s.get(&p.cor, (size_t)K * K))) {
        err = "demc_covariance: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    p.cols = d_cols;
    hipError_t e = hipMemcpyAsync(d_cols, table, sizeof table, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { err = std::string("demc_covariance: ") + hipGetErrorString(e); return DEMC_EHIP; }
    const char* tr = std::getenv("DEMC_COV_TRACE");  // DEMC_COV_TRACE=1: device time of the passes, printed to stderr (tools/cov_bench.py)
    const bool trace = tr && tr[0] == '1';
    std::vector<Event> ev;
    auto mark = [&]() {
        if (!trace) return true;
        Event x;
        if (x.create(hipEventDefault) != hipSuccess) return false;
        ev.push_back(std::move(x));
        return hipEventRecord(ev.back(), st) == hipSuccess;
    };
    bool ok = mark();
    hipLaunchKernelGGL(k_cov_mean, dim3((unsigned)p.W), dim3(kCovWG), 0, st, p);
    hipLaunchKernelGGL(k_cov_mean_final, dim3(1), dim3(kCovMaxCols), 0, st, p);
    ok = ok && mark();
    switch (NB) {
        case 1: launch_syrk<1>(p, st); break;
        case 2: launch_syrk<2>(p, st); break;
        case 3: launch_syrk<3>(p, st); break;
        default: launch_syrk<4>(p, st); break;
    }
    ok = ok && mark();
    hipLaunchKernelGGL(k_cov_final, dim3(1), dim3(kCovFinalWG), 0, st, p);
    ok = ok && mark();
    if (!ok) { err = "demc_covariance: an event could not be recorded"; return DEMC_EHIP; }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && mean_out) e = hipMemcpy(mean_out, p.mean, (size_t)K * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && cov_out) e = hipMemcpy(cov_out, p.cov, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && cor_out) e = hipMemcpy(cor_out, p.cor, (size_t)K * K * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = std::string("demc_covariance: ") + hipGetErrorString(e); return DEMC_EHIP; }
    if (trace) {
        float ms[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        std::fprintf(stderr, "demc_covariance pass_ms %.4f %.4f %.4f\n", ms[0], ms[1], ms[2]);
    }
    return DEMC_OK;
}

}  // namespace demc
