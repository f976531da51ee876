// demc_rank.cpp -- the kernels of demc_rankstats and demc_rank_series (demc_rank.hpp says what each does; DESIGN.md 5.11 is the
// definition) and the host code that strings them together, in a translation unit of their own: the other code objects of the
// library do not change when this one does.  demc_hpd lives here too: it is the sort of round 0, whose kernels are
// local to this unit, followed by two kernels of its own.
#include "demc_rank.hpp"

#include <algorithm>
#include <vector>

#include "../../include/demc.h"
#include "demc_devmem.hpp"   // Scratch, PassTrace, finish
#include "demc_ppnd.hpp"     // ppnd16: the text the host test compiles too
#include "demc_summary.hpp"  // summary_enqueue, SumKParams (declarations only: the kernels are demc_summary.cpp's)

namespace demc {

namespace {

using u64 = unsigned long long;

struct RankKParams {
    const double* hist;          // [n_rows][P][ld]
    const unsigned char* acc;    // [n_rows][P]
    const double* lp;            // [n_rows][P]
    long long P, row0, N;        // N = n P values of a pool
    int D, ld;
    int j0, B;                   // the batch: series j0 .. j0 + B - 1
    u64* keys;                   // [2][B][N]
    unsigned* pos;               // [2][B][N]
    double* rk;                  // [B][N] average ranks by pool position (demc_rank_series: what is downloaded)
    double* der;                 // [N][ldd] the derived history: z | x <= q05 | x <= q95 | zeta -> z' of series b at 4 b
    int ldd;
    unsigned* cnt;               // [B][256][tiles] counts of a pass, then their exclusive prefix sums
    int tiles;
    long long scan_chunk;
    u64* word;                   // [2 rounds][B][3]: OR of the keys | OR of their complements | distinct keys
    int* flag;                   // [2 rounds][B] the pool holds a NaN
    double* q;                   // [B][3] med | q05 | q95
    double* out;                 // [series][8]
};

__device__ __forceinline__ u64 rank_key(double x) {  // the key order of DESIGN.md 5.6
    const u64 b = (u64)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}
__device__ __forceinline__ double rank_value(u64 k) { return __longlong_as_double((long long)(k ^ ((k >> 63) ? 1ull << 63 : ~0ull))); }
__device__ __forceinline__ double rank_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// bits in which the keys of (round, b) differ; a digit without one is shared by the whole pool and its pass is skipped
__device__ __forceinline__ u64 rank_diff(const RankKParams& p, int round, int b) {
    const u64* w = p.word + ((size_t)round * p.B + b) * 3;
    return w[0] & w[1];
}
__device__ __forceinline__ bool rank_skip(u64 diff, int d) { return ((diff >> (d * kRankBits)) & 255ull) == 0ull; }
// which of the two buffers holds the pairs before the pass of digit d (d = kRankPasses: after the last)
__device__ __forceinline__ int rank_src(u64 diff, int d) {
    int c = 0;
    for (int e = 0; e < d; ++e) c += rank_skip(diff, e) ? 0 : 1;
    return c & 1;
}

// every value of the batch, the history read straight through: f(b, t, x) for series j0 + b at pool position t
template <typename F>
__device__ __forceinline__ void rank_stream(const RankKParams& p, F f) {
    const long long stride = (long long)gridDim.x * kRankWG, t0 = (long long)blockIdx.x * kRankWG + threadIdx.x;
    const int c0 = p.j0, c1 = min(p.j0 + p.B, p.D);
    if (c0 < c1) {
        const double* base = p.hist + (size_t)p.row0 * p.P * p.ld;
        const long long total = p.N * p.ld;
        for (long long i = t0; i < total; i += stride) {  // consecutive lanes on consecutive doubles
            const long long cell = i / p.ld;
            const int col = (int)(i - cell * p.ld);
            if (col < c0 || col >= c1) continue;  // another batch's column, or the padding of a cell
            f(col - c0, cell, base[i]);
        }
    }
    if (p.D >= p.j0 && p.D < p.j0 + p.B) {
        const unsigned char* acc = p.acc + (size_t)p.row0 * p.P;
        for (long long t = t0; t < p.N; t += stride) f(p.D - p.j0, t, (double)acc[t]);
    }
    if (p.D + 1 >= p.j0 && p.D + 1 < p.j0 + p.B) {
        const double* lp = p.lp + (size_t)p.row0 * p.P;
        for (long long t = t0; t < p.N; t += stride) f(p.D + 1 - p.j0, t, lp[t]);
    }
}

__global__ __launch_bounds__(kRankWG) void k_rank_keys(RankKParams p) {
    rank_stream(p, [&](int b, long long t, double x) {
        p.keys[(size_t)b * p.N + t] = rank_key(x);
        p.pos[(size_t)b * p.N + t] = (unsigned)t;
    });
}

// the second round: the keys of zeta, from the derived history
__global__ __launch_bounds__(kRankWG) void k_rank_keys_folded(RankKParams p) {
    const int b = blockIdx.y;
    for (long long t = (long long)blockIdx.x * kRankWG + threadIdx.x; t < p.N; t += (long long)gridDim.x * kRankWG) {
        p.keys[(size_t)b * p.N + t] = rank_key(p.der[(size_t)t * p.ldd + kRankDerived * b + 3]);
        p.pos[(size_t)b * p.N + t] = (unsigned)t;
    }
}

__global__ __launch_bounds__(kRankWG) void k_rank_range(RankKParams p, int round) {
    const int b = blockIdx.y;
    const u64* ks = p.keys + (size_t)b * p.N;
    u64 o = 0ull, c = 0ull;
    int nan = 0;
    for (long long t = (long long)blockIdx.x * kRankWG + threadIdx.x; t < p.N; t += (long long)gridDim.x * kRankWG) {
        const u64 k = ks[t];
        o |= k;
        c |= ~k;
        if (k < kQKeyNegInf || k > kQKeyPosInf) nan = 1;
    }
    for (int m = 32; m > 0; m >>= 1) {
        o |= __shfl_xor(o, m, 64);
        c |= __shfl_xor(c, m, 64);
        nan |= __shfl_xor(nan, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {  // integer ORs: the words cannot depend on the order of arrival
        u64* w = p.word + ((size_t)round * p.B + b) * 3;
        atomicOr(&w[0], o);
        atomicOr(&w[1], c);
        if (nan) p.flag[round * p.B + b] = 1;  // (every writer writes the same word: no atomic)
    }
}

// one wave per tile: the counts of digit d
__global__ __launch_bounds__(kRankWave) void k_rank_hist(RankKParams p, int round, int d) {
    __shared__ unsigned cnt[256];
    const int b = blockIdx.y, lane = threadIdx.x;
    const u64 diff = rank_diff(p, round, b);
    if (rank_skip(diff, d)) return;  // (uniform over the workgroup)
    const u64* ks = p.keys + ((size_t)rank_src(diff, d) * p.B + b) * p.N;
    for (int i = lane; i < 256; i += kRankWave) cnt[i] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kRankTile;
    for (int r = 0; r < kRankTile / kRankWave; ++r) {
        const long long i = base + r * kRankWave + lane;
        if (i < p.N) atomicAdd(&cnt[(unsigned)(ks[i] >> (d * kRankBits)) & 255u], 1u);
    }
    __syncthreads();
    for (int i = lane; i < 256; i += kRankWave) p.cnt[((size_t)b * 256 + i) * p.tiles + blockIdx.x] = cnt[i];
}

// one workgroup per series: exclusive prefix sums over (digit, tile), digit-major, in index order
__global__ __launch_bounds__(kRankScanWG) void k_rank_scan(RankKParams p, int round, int d) {
    __shared__ unsigned part[kRankScanWG];
    const int b = blockIdx.x, t = threadIdx.x;
    if (rank_skip(rank_diff(p, round, b), d)) return;
    unsigned* h = p.cnt + (size_t)b * 256 * p.tiles;
    const long long total = (long long)256 * p.tiles;
    const long long want = (long long)t * p.scan_chunk, lo = want < total ? want : total, hi = lo + p.scan_chunk < total ? lo + p.scan_chunk : total;
    unsigned s = 0u;
    for (long long i = lo; i < hi; ++i) s += h[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned run = 0u;
        for (int i = 0; i < kRankScanWG; ++i) {
            const unsigned v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    unsigned run = part[t];
    for (long long i = lo; i < hi; ++i) {
        const unsigned v = h[i];
        h[i] = run;
        run += v;
    }
}

// one wave per tile, rounds of 64 pairs in position order: stable within the round, across rounds and across tiles
__global__ __launch_bounds__(kRankWave) void k_rank_scatter(RankKParams p, int round, int d) {
    __shared__ unsigned cnt[256];
    const int b = blockIdx.y, lane = threadIdx.x;
    const u64 diff = rank_diff(p, round, b);
    if (rank_skip(diff, d)) return;  // (uniform over the workgroup)
    const int src = rank_src(diff, d);
    const u64* ks = p.keys + ((size_t)src * p.B + b) * p.N;
    const unsigned* ps = p.pos + ((size_t)src * p.B + b) * p.N;
    u64* kd = p.keys + ((size_t)(1 - src) * p.B + b) * p.N;
    unsigned* pd = p.pos + ((size_t)(1 - src) * p.B + b) * p.N;
    for (int i = lane; i < 256; i += kRankWave) cnt[i] = p.cnt[((size_t)b * 256 + i) * p.tiles + blockIdx.x];
    __syncthreads();
    const long long base = (long long)blockIdx.x * kRankTile;
    const u64 below_me = (1ull << lane) - 1ull;
    for (int r = 0; r < kRankTile / kRankWave; ++r) {
        if (base + r * kRankWave >= p.N) break;  // (uniform)
        const long long i = base + r * kRankWave + lane;
        const bool valid = i < p.N;
        const u64 k = valid ? ks[i] : 0ull;
        const unsigned ps_i = valid ? ps[i] : 0u;
        const unsigned dg = (unsigned)(k >> (d * kRankBits)) & 255u;
        u64 peers = __ballot(valid);  // the valid lanes that hold the same digit
#pragma unroll
        for (int bit = 0; bit < kRankBits; ++bit) {
            const bool one = (dg >> bit) & 1u;
            const u64 bal = __ballot(valid && one);
            peers &= one ? bal : ~bal;
        }
        const unsigned below = (unsigned)__popcll(peers & below_me), all = (unsigned)__popcll(peers);
        const unsigned start = valid ? cnt[dg] : 0u;
        __syncthreads();
        if (valid && below == 0u) cnt[dg] = start + all;  // the lowest lane of every digit moves the tile's running count
        __syncthreads();
        const long long dst = (long long)start + below;
        if (valid && dst < p.N) {
            kd[dst] = k;
            pd[dst] = ps_i;
        }
    }
}

// r = L + (E + 1) / 2 of every sorted position, to the draw's own position; the run heads; med, q05, q95 (round 0)
__global__ __launch_bounds__(kRankWG) void k_rank_ties(RankKParams p, int round, RankTargets tg) {
    __shared__ unsigned heads;
    const int b = blockIdx.y;
    const int src = rank_src(rank_diff(p, round, b), kRankPasses);
    const u64* ks = p.keys + ((size_t)src * p.B + b) * p.N;
    const unsigned* ps = p.pos + ((size_t)src * p.B + b) * p.N;
    double* rk = p.rk + (size_t)b * p.N;
    if (threadIdx.x == 0) heads = 0u;
    __syncthreads();
    unsigned mine = 0u;
    for (long long i = (long long)blockIdx.x * kRankWG + threadIdx.x; i < p.N; i += (long long)gridDim.x * kRankWG) {
        const u64 k = ks[i];
        const bool head = i == 0 || ks[i - 1] != k, tail = i == p.N - 1 || ks[i + 1] != k;
        long long first = i, last = i;
        if (!head) {  // the first position whose key is not below k
            long long lo = 0, hi = i;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (ks[mid] < k) lo = mid + 1; else hi = mid;
            }
            first = lo;
        }
        if (!tail) {  // the first position whose key is above k
            long long lo = i + 1, hi = p.N;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (ks[mid] <= k) lo = mid + 1; else hi = mid;
            }
            last = lo - 1;
        }
        mine += head ? 1u : 0u;
        const unsigned at = ps[i];
        if ((long long)at < p.N) rk[at] = (double)first + ((double)(last - first + 1) + 1.0) / 2.0;
    }
    if (mine) atomicAdd(&heads, mine);
    __syncthreads();
    if (threadIdx.x == 0 && heads) atomicAdd(&p.word[((size_t)round * p.B + b) * 3 + 2], (u64)heads);  // (an integer sum)
    if (round == 0 && blockIdx.x == 0 && threadIdx.x < 3) {  // DESIGN.md 5.6, to the operation
        const int k = threadIdx.x;
        const long long j = tg.j[k];
        const double a = rank_value(ks[j - 1]), c = rank_value(ks[p.N == 1 ? 0 : j]), gm = tg.gamma[k];
        double r;
        if (p.N == 1) r = a;
        else if (isfinite(a) && isfinite(c)) r = a + gm * (c - a);
        else if (gm == 0.0) r = a;
        else if (gm == 1.0) r = c;
        else r = (1.0 - gm) * a + gm * c;
        p.q[b * 3 + k] = r;
    }
}

__device__ __forceinline__ double rank_score(double r, long long N) { return ppnd16((r - 0.375) / ((double)N + 0.25)); }

// the four derived series of every value of the batch
__global__ __launch_bounds__(kRankWG) void k_rank_derive(RankKParams p) {
    rank_stream(p, [&](int b, long long t, double x) {
        const double* q = p.q + b * 3;
        double* o = p.der + (size_t)t * p.ldd + kRankDerived * b;
        o[0] = rank_score(p.rk[(size_t)b * p.N + t], p.N);
        o[1] = x <= q[1] ? 1.0 : 0.0;
        o[2] = x <= q[2] ? 1.0 : 0.0;
        o[3] = fabs(x - q[0]);
    });
}

// ranks -> normal scores: into slot 3 of the derived history (z' over zeta), or in place (demc_rank_series, kind 1)
__global__ __launch_bounds__(kRankWG) void k_rank_score(RankKParams p, int in_place) {
    const int b = blockIdx.y;
    for (long long t = (long long)blockIdx.x * kRankWG + threadIdx.x; t < p.N; t += (long long)gridDim.x * kRankWG) {
        const double z = rank_score(p.rk[(size_t)b * p.N + t], p.N);
        if (in_place) p.rk[(size_t)b * p.N + t] = z;
        else p.der[(size_t)t * p.ldd + kRankDerived * b + 3] = z;
    }
}

// a thread per series of the batch: the eight columns from the summary table [4 B + 2][6] of the derived history
__global__ __launch_bounds__(64) void k_rank_final(RankKParams p, const double* tab) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const double nan = rank_nan();
    const double* r = tab + (size_t)kRankDerived * b * 6;
    const double rb = r[2], eb = r[3], e05 = r[6 + 3], e95 = r[12 + 3];
    const double rf = p.flag[p.B + b] ? nan : r[18 + 2];  // a NaN among zeta: no folded R-hat
    double* o = p.out + (size_t)(p.j0 + b) * DEMC_RANK_COLS;
    if (p.flag[b]) {
        for (int c = 0; c < DEMC_RANK_COLS; ++c) o[c] = nan;
        return;
    }
    o[0] = (rb != rb || rf != rf) ? nan : (rb > rf ? rb : rf);
    o[1] = eb;
    o[2] = (e05 != e05 || e95 != e95) ? nan : (e05 < e95 ? e05 : e95);
    o[3] = rb; o[4] = rf; o[5] = e05; o[6] = e95;
    o[7] = (double)p.word[(size_t)b * 3 + 2];
}

// ---- demc_hpd: the sorted keys of round 0, then one pass over the window widths ---------------------------------------

struct HpdBest {  // a candidate and its width; i < 0: none yet
    double w;
    long long i;
};

// the one of two candidates that Julia's findmin meets first: a NaN width ranks below every number, other widths compare by value,
// equal widths (two NaNs among them) by position.  A total order over distinct i: the minimum does not depend on how it is grouped.
__device__ __forceinline__ HpdBest hpd_min(HpdBest a, HpdBest b) {
    const bool an = a.w != a.w, bn = b.w != b.w;
    bool a_first;
    if (a.i < 0 || b.i < 0) a_first = b.i < 0;
    else if (an != bn) a_first = an;
    else if (!an && a.w != b.w) a_first = a.w < b.w;
    else a_first = a.i < b.i;
    return HpdBest{a_first ? a.w : b.w, a_first ? a.i : b.i};  // (field by field: the two records stay in registers)
}
__device__ __forceinline__ HpdBest hpd_wave_min(HpdBest best) {
    for (int s = 32; s > 0; s >>= 1) {
        const HpdBest o{__shfl_xor(best.w, s, 64), __shfl_xor(best.i, s, 64)};
        best = hpd_min(best, o);
    }
    return best;
}
// the sorted keys of series b of the batch: the buffer the passes that ran left them in
__device__ __forceinline__ const u64* hpd_sorted(const RankKParams& p, int b) {
    return p.keys + ((size_t)rank_src(rank_diff(p, 0, b), kRankPasses) * p.B + b) * p.N;
}

// blockIdx.y the series of the batch, blockIdx.z the alpha; lanes on consecutive candidates i: two coalesced loads, y[i] and
// y[N - m + i], one subtraction; the best of a thread, of its wave (shuffles), of the workgroup (LDS) -> one partial per workgroup
__global__ __launch_bounds__(kHpdWG) void k_hpd_window(RankKParams p, HpdGrid g, double* part_w, long long* part_i) {
    __shared__ double sw[kHpdWG / 64];
    __shared__ long long si[kHpdWG / 64];
    const int b = blockIdx.y, k = blockIdx.z, wgs = g.wgs[k];
    if ((int)blockIdx.x >= wgs) return;  // (uniform over the workgroup: an alpha with fewer candidates than the largest)
    const long long m = g.m[k], top = p.N - m, stride = (long long)wgs * kHpdWG;
    const u64* ks = hpd_sorted(p, b);
    HpdBest best{0.0, -1};
    for (long long i = (long long)blockIdx.x * kHpdWG + threadIdx.x; i < m; i += stride) {
        const HpdBest c{rank_value(ks[top + i]) - rank_value(ks[i]), i};
        best = hpd_min(best, c);
    }
    best = hpd_wave_min(best);
    if ((threadIdx.x & 63) == 0) {
        sw[threadIdx.x >> 6] = best.w;
        si[threadIdx.x >> 6] = best.i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < kHpdWG / 64; ++v) best = hpd_min(best, HpdBest{sw[v], si[v]});
        const size_t at = ((size_t)b * g.n_alphas + k) * g.slots + blockIdx.x;
        part_w[at] = best.w;
        part_i[at] = best.i;
    }
}

// one wave per (series of the batch, alpha): the partials in index order, the NaN flag of the pool, keys back to values
__global__ __launch_bounds__(kHpdFinalWG) void k_hpd_final(RankKParams p, HpdGrid g, const double* part_w, const long long* part_i) {
    const int b = blockIdx.x, k = blockIdx.y;
    const size_t base = ((size_t)b * g.n_alphas + k) * g.slots;
    const long long m = g.m[k];
    HpdBest best{0.0, -1};
    for (int x = threadIdx.x; x < g.wgs[k]; x += kHpdFinalWG) best = hpd_min(best, HpdBest{part_w[base + x], part_i[base + x]});
    best = hpd_wave_min(best);
    if (threadIdx.x != 0) return;
    double* o = p.out + ((size_t)(p.j0 + b) * g.n_alphas + k) * DEMC_HPD_COLS;
    if (p.flag[b] || best.i < 0 || best.i >= m) {
        o[0] = o[1] = o[2] = rank_nan();
    } else {
        const u64* ks = hpd_sorted(p, b);
        o[0] = rank_value(ks[best.i]);
        o[1] = rank_value(ks[p.N - m + best.i]);
        o[2] = (double)best.i;
    }
    o[3] = (double)m;
}

// keys in buffer 0 -> sorted pairs in the buffer rank_src(diff, kRankPasses) names
void sort_round(const RankKParams& p, int blocks, int tiles, int passes, int round, hipStream_t st) {
    const dim3 stream_grid((unsigned)blocks, (unsigned)p.B), tile_grid((unsigned)tiles, (unsigned)p.B);
    hipLaunchKernelGGL(k_rank_range, stream_grid, dim3(kRankWG), 0, st, p, round);
    for (int d = 0; d < passes; ++d) {  // a pass whose digit the pool shares costs three launches that return at once
        hipLaunchKernelGGL(k_rank_hist, tile_grid, dim3(kRankWave), 0, st, p, round, d);
        hipLaunchKernelGGL(k_rank_scan, dim3((unsigned)p.B), dim3(kRankScanWG), 0, st, p, round, d);
        hipLaunchKernelGGL(k_rank_scatter, tile_grid, dim3(kRankWave), 0, st, p, round, d);
    }
}

}  // namespace

int rank_run(const HistView& v, const RankPlan& plan, const SummaryPlan& full, const SummaryPlan& last, int series, int kind, hipStream_t st,
             double* out, std::string& err) {
    const bool single = series >= 0;
    const char* who = single ? "demc_rank_series" : "demc_rankstats";
    RankKParams p{};
    p.hist = v.hist; p.acc = v.acc; p.lp = v.lp;
    p.P = v.P; p.row0 = v.row0; p.N = plan.N;
    p.D = v.D; p.ld = v.ld; p.tiles = plan.tiles; p.scan_chunk = plan.scan_chunk;
    Scratch s;
    double* zero_lp = nullptr;
    unsigned char* zero_acc = nullptr;
    bool ok = s.get(&p.keys, plan.n_keys) && s.get(&p.pos, plan.n_pos) && s.get(&p.rk, plan.n_rk) && s.get(&p.cnt, plan.n_hist) &&
              s.get(&p.word, plan.n_word) && s.get(&p.flag, plan.n_flag) && s.get(&p.q, plan.n_q);
    if (ok && !(single && kind != DEMC_RANK_KIND_FOLDED)) ok = s.get(&p.der, plan.n_der);
    if (ok && !single) ok = s.get(&p.out, plan.n_out) && s.get(&zero_lp, plan.n_zero) && s.get(&zero_acc, plan.n_zero);
    if (!ok) { err = std::string(who) + ": out of device memory for the scratch buffers"; return DEMC_ENOMEM; }
    if (!single) {  // the two internal series of the derived history: constant, so the summary kernels stop on them at once
        hipError_t e = hipMemsetAsync(zero_lp, 0, plan.n_zero * sizeof(double), st);
        if (e == hipSuccess) e = hipMemsetAsync(zero_acc, 0, plan.n_zero, st);
        if (!hip_ok(who, e, err)) return DEMC_EHIP;
    }
    std::vector<Scratch> sums;  // the summary runs' buffers live until the stream has drained
    sums.reserve((size_t)plan.batches);
    PassTrace tr;  // (the diagnostic variant: per batch keys | sort | ties, derive, keys | sort | ties, scores, summary, final)
    bool marks = tr.mark(st);
    for (int bi = 0; bi < plan.batches; ++bi) {
        p.j0 = single ? series : bi * plan.batch;
        p.B = bi == plan.batches - 1 ? plan.last_batch : plan.batch;
        p.ldd = kRankDerived * p.B;
        const dim3 stream_grid((unsigned)plan.blocks, (unsigned)p.B), flat_grid((unsigned)plan.blocks);
        hipError_t e = hipMemsetAsync(p.word, 0, plan.n_word * sizeof(u64), st);
        if (e == hipSuccess) e = hipMemsetAsync(p.flag, 0, plan.n_flag * sizeof(int), st);
        if (!hip_ok(who, e, err)) return DEMC_EHIP;
        hipLaunchKernelGGL(k_rank_keys, flat_grid, dim3(kRankWG), 0, st, p);
        marks = marks && tr.mark(st);
        sort_round(p, plan.blocks, plan.tiles, plan.passes, 0, st);
        marks = marks && tr.mark(st);
        hipLaunchKernelGGL(k_rank_ties, stream_grid, dim3(kRankWG), 0, st, p, 0, plan.tg);
        if (single && kind == DEMC_RANK_KIND_RANK) break;
        if (single && kind == DEMC_RANK_KIND_SCORE) {
            hipLaunchKernelGGL(k_rank_score, stream_grid, dim3(kRankWG), 0, st, p, 1);
            break;
        }
        hipLaunchKernelGGL(k_rank_derive, flat_grid, dim3(kRankWG), 0, st, p);
        hipLaunchKernelGGL(k_rank_keys_folded, stream_grid, dim3(kRankWG), 0, st, p);
        marks = marks && tr.mark(st);
        sort_round(p, plan.blocks, plan.tiles, plan.passes, 1, st);
        marks = marks && tr.mark(st);
        hipLaunchKernelGGL(k_rank_ties, stream_grid, dim3(kRankWG), 0, st, p, 1, plan.tg);
        if (single) break;
        hipLaunchKernelGGL(k_rank_score, stream_grid, dim3(kRankWG), 0, st, p, 0);
        const HistView dv{p.der, zero_acc, zero_lp, v.idh + (size_t)v.row0 * v.P, v.P, 0, plan.n, v.id0, p.ldd, p.ldd};
        sums.emplace_back();
        SumKParams sp;
        const int rc = summary_enqueue(who, dv, p.B == plan.batch ? full : last, st, sums.back(), sp, err);
        if (rc != DEMC_OK) return rc;
        hipLaunchKernelGGL(k_rank_final, dim3((unsigned)((p.B + 63) / 64)), dim3(64), 0, st, p, (const double*)sp.out);
        marks = marks && tr.mark(st);
    }
    if (!marks) { err = std::string(who) + ": an event could not be recorded"; return DEMC_EHIP; }
    if (!finish(who, st, {{out, single ? p.rk : p.out, (single ? (size_t)plan.N : plan.n_out) * sizeof(double)}}, err)) return DEMC_EHIP;
    if (!single) tr.print(who, 5 * plan.batches, 1);
    return DEMC_OK;
}

int hpd_run(const HistView& v, const HpdPlan& plan, hipStream_t st, double* out, std::string& err) {
    const char* name = "demc_hpd";
    RankKParams p{};
    p.hist = v.hist; p.acc = v.acc; p.lp = v.lp;
    p.P = v.P; p.row0 = v.row0; p.N = plan.N;
    p.D = v.D; p.ld = v.ld; p.tiles = plan.tiles; p.scan_chunk = plan.scan_chunk;
    Scratch s;
    double* part_w = nullptr;
    long long* part_i = nullptr;
    if (!(s.get(&p.keys, plan.n_keys) && s.get(&p.pos, plan.n_pos) && s.get(&p.cnt, plan.n_hist) && s.get(&p.word, plan.n_word) &&
          s.get(&p.flag, plan.n_flag) && s.get(&part_w, plan.n_part) && s.get(&part_i, plan.n_part) && s.get(&p.out, plan.n_out))) {
        err = std::string(name) + ": out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    const HpdGrid& g = plan.grid;
    PassTrace tr;  // (the diagnostic variant: per batch keys | sort | window and final)
    bool marks = tr.mark(st);
    for (int bi = 0; bi < plan.batches; ++bi) {
        p.j0 = bi * plan.batch;
        p.B = bi == plan.batches - 1 ? plan.last_batch : plan.batch;
        hipError_t e = hipMemsetAsync(p.word, 0, plan.n_word * sizeof(u64), st);
        if (e == hipSuccess) e = hipMemsetAsync(p.flag, 0, plan.n_flag * sizeof(int), st);
        if (!hip_ok(name, e, err)) return DEMC_EHIP;
        hipLaunchKernelGGL(k_rank_keys, dim3((unsigned)plan.blocks), dim3(kRankWG), 0, st, p);
        marks = marks && tr.mark(st);
        sort_round(p, plan.blocks, plan.tiles, plan.passes, 0, st);
        marks = marks && tr.mark(st);
        hipLaunchKernelGGL(k_hpd_window, dim3((unsigned)g.slots, (unsigned)p.B, (unsigned)g.n_alphas), dim3(kHpdWG), 0, st, p, g, part_w, part_i);
        hipLaunchKernelGGL(k_hpd_final, dim3((unsigned)p.B, (unsigned)g.n_alphas), dim3(kHpdFinalWG), 0, st, p, g, (const double*)part_w,
                           (const long long*)part_i);
        marks = marks && tr.mark(st);
    }
    if (!marks) { err = std::string(name) + ": an event could not be recorded"; return DEMC_EHIP; }
    if (!finish(name, st, {{out, p.out, plan.n_out * sizeof(double)}}, err)) return DEMC_EHIP;
    tr.print(name, 3 * plan.batches, 1);
    return DEMC_OK;
}

}  // namespace demc
