// demc_quantile.cpp -- the kernels of demc_quantiles (demc_quantile.hpp) and the host code that strings them together, in a
// translation unit of their own: the other code objects of the library do not change when this one does.
#define DEMC_QUANTILE_KERNELS
#include "demc_quantile.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, Event

namespace demc {

namespace {

struct Events {  // DEMC_QUANTILE_TRACE=1: device time of every histogram pass, printed to stderr (tools/quantile_bench.py)
    std::vector<Event> ev;
    bool mark(hipStream_t st) {
        Event e;
        if (e.create(hipEventDefault) != hipSuccess) return false;
        ev.push_back(std::move(e));
        return hipEventRecord(ev.back(), st) == hipSuccess;
    }
};

}  // namespace

int quantile_run(const QArgs& a, hipStream_t st, const double* probs, int n_probs, double* out, std::string& err) {
    const long long n = a.row1 - a.row0, N = n * a.P;
    const int D2 = a.D + 2;
    // the targets: aleph = N p + (1 - p) as a rounded product and a rounded sum, j = clamp(trunc(aleph), 1, N - 1)
    QTargets tg{};
    tg.n_probs = n_probs;
    std::vector<unsigned long long> ranks;  // 0-based: x_(j) has rank j - 1
    std::vector<long long> js(n_probs);
    for (int k = 0; k < n_probs; ++k) {
        const double p = probs[k];
        const double prod = (double)N * p;
        const double aleph = prod + (1.0 - p);
        long long j = (long long)std::trunc(aleph);
        j = std::max<long long>(1, std::min<long long>(j, N - 1));
        if (N == 1) j = 1;
        tg.gamma[k] = N == 1 ? 0.0 : std::min(1.0, std::max(0.0, aleph - (double)j));
        js[k] = j;
        ranks.push_back((unsigned long long)(j - 1));
        if (N > 1) ranks.push_back((unsigned long long)j);
    }
    std::sort(ranks.begin(), ranks.end());
    ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
    const int T = (int)ranks.size();  // <= kQMaxTargets
    for (int t = 0; t < T; ++t) tg.rank[t] = ranks[t];
    for (int k = 0; k < n_probs; ++k) {
        tg.ia[k] = (int)(std::lower_bound(ranks.begin(), ranks.end(), (unsigned long long)(js[k] - 1)) - ranks.begin());
        tg.ib[k] = N == 1 ? tg.ia[k] : (int)(std::lower_bound(ranks.begin(), ranks.end(), (unsigned long long)js[k]) - ranks.begin());
    }

    // geometry (demc_quantile.hpp): a chunk is cpi whole cells, a workgroup takes every W-th chunk
    const int cpi = kQWG / std::min(a.ld, kQWG);
    const long long chunks = (N + cpi - 1) / cpi;
    const int W = (int)std::min<long long>(chunks, kQMaxWG);
    if ((chunks + W - 1) / W > kQMaxChunksPerWG) { err = "demc_quantiles: too many rows for the 32-bit counts of a workgroup"; return DEMC_EINVAL; }

    QKParams p{};
    p.hist = a.hist; p.acc = a.acc; p.lp = a.lp;
    p.P = a.P; p.row0 = a.row0; p.n = n; p.D = a.D; p.ld = a.ld; p.T = T;
    Scratch s;
    const size_t cells = (size_t)D2 * T;
    if (!(s.get(&p.table, cells * 256) && s.get(&p.gprefix, cells) && s.get(&p.trank, cells) && s.get(&p.tgrp, cells) && s.get(&p.ng, (size_t)D2) &&
          s.get(&p.nanflag, (size_t)D2) && s.get(&p.out, (size_t)D2 * n_probs))) {
        err = "demc_quantiles: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    hipError_t e = hipMemsetAsync(p.table, 0, cells * 256 * sizeof(unsigned long long), st);
    if (e != hipSuccess) { err = std::string("demc_quantiles: ") + hipGetErrorString(e); return DEMC_EHIP; }
    const char* tr = std::getenv("DEMC_QUANTILE_TRACE");
    const bool trace = tr && tr[0] == '1';
    Events ev;
    hipLaunchKernelGGL(k_q_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, p, tg);
    const int passes = 64 / kQBits;
    const size_t lds_max = (size_t)kQSlots * 257 * sizeof(unsigned int);  // tables and owner words
    for (const void* f : {(const void*)k_q_hist<true>, (const void*)k_q_hist<false>})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) {
            err = "demc_quantiles: the LDS limit of a kernel could not be raised";
            return DEMC_EHIP;
        }
    for (int i = 0; i < passes; ++i) {
        const int shift = 64 - kQBits * (i + 1);
        p.slots = 1;  // the power of two that holds the groups there can be, up to kQSlots
        while (p.slots < kQSlots && p.slots < (i == 0 ? (long long)D2 : (long long)D2 * T)) p.slots *= 2;
        const size_t lds = (size_t)p.slots * 257 * sizeof(unsigned int);
        if (trace && !ev.mark(st)) { err = "demc_quantiles: an event could not be recorded"; return DEMC_EHIP; }
        if (i == 0) hipLaunchKernelGGL((k_q_hist<true>), dim3((unsigned)W), dim3(kQWG), lds, st, p, shift);
        else hipLaunchKernelGGL((k_q_hist<false>), dim3((unsigned)W), dim3(kQWG), lds, st, p, shift);
        if (trace && !ev.mark(st)) { err = "demc_quantiles: an event could not be recorded"; return DEMC_EHIP; }
        hipLaunchKernelGGL(k_q_scan, dim3((unsigned)D2), dim3(256), 0, st, p, shift);
    }
    hipLaunchKernelGGL(k_q_final, dim3((unsigned)(((size_t)D2 * n_probs + 255) / 256)), dim3(256), 0, st, p, tg);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(out, p.out, (size_t)D2 * n_probs * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = std::string("demc_quantiles: ") + hipGetErrorString(e); return DEMC_EHIP; }
    if (trace) {
        std::string line = "demc_quantiles pass_ms";
        for (int i = 0; i < passes; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev.ev[2 * i], ev.ev[2 * i + 1]);
            char buf[32];
            std::snprintf(buf, sizeof buf, " %.4f", ms);
            line += buf;
        }
        std::fprintf(stderr, "%s\n", line.c_str());
    }
    return DEMC_OK;
}

}  // namespace demc
