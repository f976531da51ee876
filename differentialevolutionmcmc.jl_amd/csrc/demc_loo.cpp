// demc_loo.cpp -- the kernels of demc_loo (demc_loo.hpp says what each does; DESIGN.md 5.9 is the definition) and the host code
// that strings them together, in a translation unit of their own: the other code objects of the library do not change when this
// one does.
#include "demc_loo.hpp"

#include "../../include/demc.h"
#include "demc_devmem.hpp"  // Scratch, PassTrace, finish
#include "demc_pwterm.hpp"  // the term itself, shared with demc_pointwise.cpp

namespace demc {

namespace {

using u64 = unsigned long long;

constexpr double kLooLogMin = -708.3964185322641;  // log(DBL_MIN), rounded to FP64: the floor of a shifted log ratio
constexpr int kLooDigits = 6;

__device__ __forceinline__ u64 loo_key(double x) {  // the key order of DESIGN.md 5.6
    const u64 b = (u64)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}
__device__ __forceinline__ double loo_value(u64 k) { return __longlong_as_double((long long)(k ^ ((k >> 63) ? 1ull << 63 : ~0ull))); }

// a draw's constants, once per call
__global__ __launch_bounds__(kPwPrepWG) void k_loo_prepare(PwKParams p) {
    for (long long s = (long long)blockIdx.x * kPwPrepWG + threadIdx.x; s < p.S; s += (long long)gridDim.x * kPwPrepWG) pw_prepare_draw(p, s);
}

// the terms of observations [obs0, obs0 + nb) in the library's own order, column-major: out[c][s]
template <int F, int X>
__global__ __launch_bounds__(kPwWG) void k_loo_terms(PwKParams p, const double* __restrict__ cst, double* __restrict__ out, long long obs0, int nb) {
    __shared__ double s_tab[pw_table_len<F>()];
    __shared__ double s_tile[kLooObs][kLooTile + 1];
    const double* tab = pw_table<F>(s_tab);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c0 = (int)blockIdx.x * kLooObs;
    const int col = c0 + lane < nb ? c0 + lane : nb - 1;  // (a lane past the end walks the block's last observation and stores nothing)
    PwObs<F, X> o;
    pw_load<F, X>(p, obs0 + col, o);
    const double lsg = F == PW_LNR ? log(p.c0) : 0.0, isg = F == PW_LNR ? 1.0 / p.c0 : 0.0;
    const long long s0 = (long long)blockIdx.y * p.chunk_len, s1 = s0 + p.chunk_len < p.S ? s0 + p.chunk_len : p.S;
    const int sd = threadIdx.x & (kLooTile - 1), so = threadIdx.x >> 4;  // the store: 16 lanes write one line of one column
    for (long long sb = s0; sb < s1; sb += kLooTile) {
#pragma unroll
        for (int q = 0; q < kLooTile / 4; ++q) {
            const long long s = sb + wave * (kLooTile / 4) + q;
            if (s < s1) s_tile[lane][wave * (kLooTile / 4) + q] = pw_term<F, X>(p, cst + (size_t)s * p.K, o, tab, lsg, isg);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLooObs / 16; ++j) {
            const int oc = so + 16 * j;
            if (c0 + oc < nb && sb + sd < s1) out[(size_t)(c0 + oc) * (size_t)p.S + (size_t)(sb + sd)] = s_tile[oc][sd];
        }
        __syncthreads();
    }
}

struct LooLds {
    u64* keys;       // [kLooCap]
    double* tail;    // [kLooMaxTail] the excesses of the tail, then its smoothed log weights
    unsigned* hist;  // [2048]
    double* red;     // [kLooWG]
    u64* redk;       // [kLooWG] (the fit: b [128] | L [128] | b w [128] as doubles)
    unsigned* part;  // [256]
    u64* word;       // [16]
};

template <typename T, typename Op>
__device__ __forceinline__ T loo_reduce(T* row, T v, Op op) {  // a halving tree over the threads; every thread returns the result
    const int t = threadIdx.x;
    row[t] = v;
    __syncthreads();
    for (int w = kLooWG / 2; w > 0; w >>= 1) {
        if (t < w) row[t] = op(row[t], row[t + w]);
        __syncthreads();
    }
    const T r = row[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double loo_sum(const LooLds& L, double v) { return loo_reduce(L.red, v, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ double loo_max(const LooLds& L, double v) { return loo_reduce(L.red, v, [](double a, double b) { return a > b ? a : b; }); }

// One observation: the column col[S] of its terms -> the row of six.  M: the tail length, 0: no tail is formed.
__global__ __launch_bounds__(kLooWG) void k_loo_column(PwKParams p, const double* __restrict__ terms, long long obs0, int M) {
    extern __shared__ __align__(16) unsigned char loo_lds[];
    LooLds L;
    L.keys = (u64*)loo_lds;
    L.tail = (double*)(L.keys + kLooCap);
    L.hist = (unsigned*)(L.tail + kLooMaxTail);
    L.red = (double*)(L.hist + (1 << kLooBits));
    L.redk = (u64*)(L.red + kLooWG);
    L.part = (unsigned*)(L.redk + kLooWG);
    L.word = (u64*)(L.part + 256);
    const int t = threadIdx.x;
    const long long S = p.S;
    const double* __restrict__ col = terms + (size_t)blockIdx.x * (size_t)S;
    const double inf = INFINITY;

    // (1) the keys' range, the flags, lppd
    u64 kmin = ~0ull, kmax = 0ull;
    int flags = 0;
    double Mx = -inf, E = 0.0;
    for (long long s = t; s < S; s += kLooWG) {
        const double l = col[s];
        const u64 k = loo_key(l);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
        if (l != l || l == inf)
            flags |= 2;
        else if (l == -inf)
            flags |= 1;
        else if (l > Mx) {
            E = E * exp(Mx - l) + 1.0;
            Mx = l;
        } else
            E += exp(l - Mx);
    }
    kmin = loo_reduce(L.redk, kmin, [](u64 a, u64 b) { return a < b ? a : b; });
    kmax = loo_reduce(L.redk, kmax, [](u64 a, u64 b) { return a > b ? a : b; });
    flags = (int)loo_reduce(L.redk, (u64)flags, [](u64 a, u64 b) { return a | b; });
    const double Mall = loo_max(L, Mx);
    const double Eall = loo_sum(L, E != 0.0 ? E * exp(Mx - Mall) : 0.0);
    const double lppd = Mall + (log(Eall) - log((double)S));  // (a constant column: Eall == S, lppd is the term itself and p_loo is 0)
    double* out = p.point + (size_t)(p.order ? p.order[obs0 + blockIdx.x] : obs0 + blockIdx.x) * DEMC_LOO_NPOINT;
    if (flags) {
        if (t == 0) {
            if (flags & 2) {
                for (int c = 0; c < DEMC_LOO_NPOINT; ++c) out[c] = pw_nan();
            } else {
                out[0] = -inf; out[1] = lppd - (-inf); out[2] = inf; out[3] = lppd; out[4] = 0.0; out[5] = -inf;
            }
        }
        return;
    }
    const double lmin = loo_value(kmin);

    // (2) the (M + 1)-th smallest key, or a bin that holds it with few enough keys up to it.  Afterwards a key k belongs to the
    // compacted set iff (k >> sh) <= lim.
    int sh = 0;
    u64 lim = 0, key_c = 0;
    bool early = false;
    if (M > 0) {
        u64 prefix = 0;
        unsigned rank = (unsigned)M, below = 0;
        for (int d = 0; d < kLooDigits && !early; ++d) {
            const int dsh = d < kLooDigits - 1 ? 64 - kLooBits * (d + 1) : 0, top = 64 - kLooBits * d;  // the digit is bits [dsh, top)
            if ((kmin >> dsh) == (kmax >> dsh)) {  // every key agrees down to here: no read
                prefix = (kmin >> dsh) << dsh;
                continue;
            }
            const unsigned mask = (1u << (top - dsh)) - 1u;
            for (int b = t; b < (1 << kLooBits); b += kLooWG) L.hist[b] = 0u;
            __syncthreads();
            for (long long s = t; s < S; s += kLooWG) {
                const u64 k = loo_key(col[s]);
                if (d == 0 || (k >> top) == (prefix >> top)) atomicAdd(&L.hist[(unsigned)(k >> dsh) & mask], 1u);
            }
            __syncthreads();
            if (t < 256) {
                unsigned a = 0;
                for (int b = 0; b < 8; ++b) a += L.hist[8 * t + b];
                L.part[t] = a;
            }
            __syncthreads();
            if (t == 0) {  // the bin of the rank: eight bins at a time, then bin by bin
                unsigned acc = 0;
                int g = 0;
                while (g < 255 && rank >= acc + L.part[g]) acc += L.part[g++];
                int b = 8 * g;
                while (b < 8 * g + 7 && rank >= acc + L.hist[b]) acc += L.hist[b++];
                L.word[0] = (u64)b; L.word[1] = (u64)acc; L.word[2] = (u64)L.hist[b];
            }
            __syncthreads();
            const unsigned bin = (unsigned)L.word[0], acc = (unsigned)L.word[1], cnt = (unsigned)L.word[2];
            __syncthreads();
            below += acc;
            rank -= acc;
            prefix |= (u64)bin << dsh;
            if (below + cnt <= (unsigned)kLooCap) {
                early = true;
                sh = dsh;
                lim = prefix >> dsh;
            }
        }
        if (!early) {  // resolved to the last bit (ties by the thousand): the keys below it are at most M
            key_c = prefix;
            sh = 0;
            lim = key_c - 1ull;
        }
    }

    // (3) compact, and add what stays outside to the two sums: A = sum exp((x + l) - lmin), B = sum exp(x), x = lmin - l
    if (t == 0) L.word[3] = 0ull;
    __syncthreads();
    unsigned* n_keys = (unsigned*)&L.word[3];
    double A = 0.0, B = 0.0;
    for (long long s = t; s < S; s += kLooWG) {
        const double l = col[s];
        const u64 k = loo_key(l);
        if (M > 0 && (k >> sh) <= lim) {
            const unsigned pos = atomicAdd(n_keys, 1u);
            if (pos < (unsigned)kLooCap) L.keys[pos] = k;
        } else {
            const double x = lmin - l;
            A += exp((x + l) - lmin);
            B += exp(x);
        }
    }
    __syncthreads();
    const int nc = (int)(*n_keys < (unsigned)kLooCap ? *n_keys : (unsigned)kLooCap);

    // (4) sort, cutoff, floor, tail
    int P2 = 1;
    while (P2 < nc) P2 <<= 1;
    for (int i = nc + t; i < P2; i += kLooWG) L.keys[i] = ~0ull;
    __syncthreads();
    for (int k2 = 2; k2 <= P2; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P2; i += kLooWG) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const u64 a = L.keys[i], b = L.keys[ixj];
                    if ((a > b) == ((i & k2) == 0)) { L.keys[i] = b; L.keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    double l_cut = pw_nan(), x_cut = inf;
    if (M > 0) {
        l_cut = early ? loo_value(L.keys[M < nc ? M : nc - 1]) : loo_value(key_c);  // (early: the compacted keys are the below + cnt > M smallest)
        const double xc = lmin - l_cut;
        x_cut = xc > kLooLogMin ? xc : kLooLogMin;
    }
    if (t == 0) L.word[4] = 0ull;
    __syncthreads();
    unsigned* n_tail = (unsigned*)&L.word[4];
    {
        unsigned mine = 0;
        for (int j = t; j < nc; j += kLooWG) mine += (lmin - loo_value(L.keys[j])) > x_cut ? 1u : 0u;
        if (mine) atomicAdd(n_tail, mine);
    }
    __syncthreads();
    const int n2 = (int)(*n_tail < (unsigned)kLooMaxTail ? *n_tail : (unsigned)kLooMaxTail);  // the tail is keys[0 .. n2): x descends with the key; n2 <= M
    for (int j = n2 + t; j < nc; j += kLooWG) {  // compacted, but outside the tail
        const double l = loo_value(L.keys[j]), x = lmin - l;
        A += exp((x + l) - lmin);
        B += exp(x);
    }
    A = loo_sum(L, A);
    B = loo_sum(L, B);

    // (5) the fit over e_(1) <= ... <= e_(n): tail[u] = e_(u + 1), from keys[n2 - 1 - u]
    const double exc = exp(x_cut), nd = (double)n2;
    double khat = inf;
    bool fitted = false;
    if (n2 > 4) {
        for (int u = t; u < n2; u += kLooWG) L.tail[u] = exp(lmin - loo_value(L.keys[n2 - 1 - u])) - exc;
        __syncthreads();
        const int q = (int)floor(nd / 4.0 + 0.5);
        const double eq = L.tail[q - 1], en = L.tail[n2 - 1];
        fitted = eq > 0.0;
        if (fitted) {
            double* fb = (double*)L.redk;
            double* fL = fb + kLooFitMax;
            double* fw = fL + kLooFitMax;
            const int m = 30 + (int)floor(sqrt(nd));
            const double md = (double)m;
            const int lane = t & 63, wave = t >> 6;
            for (int j = wave; j < m; j += kLooWG / 64) {
                const double bj = (1.0 - sqrt(md / ((double)(j + 1) - 0.5))) / (3.0 * eq) + 1.0 / en;
                double a = 0.0;
                for (int u = lane; u < n2; u += 64) a += log1p(-bj * L.tail[u]);
                for (int w = 32; w > 0; w >>= 1) a += __shfl_xor(a, w, 64);
                if (lane == 0) {
                    const double kj = a / nd;
                    fb[j] = bj;
                    fL[j] = nd * (log(-bj / kj) - kj - 1.0);
                }
            }
            __syncthreads();
            if (t < m) {
                double den = 0.0;
                for (int i = 0; i < m; ++i) den += exp(fL[i] - fL[t]);
                fw[t] = fb[t] * (1.0 / den);
            }
            __syncthreads();
            double bhat = 0.0;
            for (int j = 0; j < m; ++j) bhat += fw[j];  // (every thread the same sum, in index order)
            __syncthreads();
            double a = 0.0;
            for (int u = t; u < n2; u += kLooWG) a += log1p(-bhat * L.tail[u]);
            const double k = loo_sum(L, a) / nd, sigma = -k / bhat;
            khat = (nd * k + 5.0) / (nd + 10.0);
            // (6) the smoothed log weights, over the excesses
            for (int u = t; u < n2; u += kLooWG) {
                const double pt = ((double)(u + 1) - 0.5) / nd, lq = log1p(-pt);
                const double g = khat == 0.0 ? -sigma * lq : sigma * expm1(-khat * lq) / khat;
                const double xs = log(g + exc);
                L.tail[u] = xs < 0.0 ? xs : 0.0;
            }
        }
    }
    __syncthreads();
    if (!fitted) {
        for (int u = t; u < n2; u += kLooWG) L.tail[u] = lmin - loo_value(L.keys[n2 - 1 - u]);  // plain weights
        khat = inf;
    }
    __syncthreads();
    double vmax = -inf;
    for (int u = t; u < n2; u += kLooWG) {
        const double v = L.tail[u] + loo_value(L.keys[n2 - 1 - u]);
        vmax = v > vmax ? v : vmax;
    }
    vmax = loo_max(L, vmax);
    const double shift = vmax > lmin ? vmax : lmin;
    double Ta = 0.0, Tb = 0.0;
    for (int u = t; u < n2; u += kLooWG) {
        const double xs = L.tail[u];
        Ta += exp((xs + loo_value(L.keys[n2 - 1 - u])) - shift);
        Tb += exp(xs);
    }
    Ta = loo_sum(L, Ta);
    Tb = loo_sum(L, Tb);
    if (t == 0) {
        const double num = A * exp(lmin - shift) + Ta, den = B + Tb;
        const double elpd = shift + (log(num) - log(den));
        out[0] = elpd; out[1] = lppd - elpd; out[2] = khat; out[3] = lppd; out[4] = (double)n2; out[5] = l_cut;
    }
}

// the eight totals of the table, rows in the caller's order
__global__ __launch_bounds__(kLooTotalsWG) void k_loo_totals(PwKParams p) {
    __shared__ double sh[kLooTotalsWG];
    const int t = threadIdx.x;
    auto block_sum = [&](double v) {  // a halving tree over the threads; every thread returns the sum
        sh[t] = v;
        __syncthreads();
        for (int w = kLooTotalsWG / 2; w > 0; w >>= 1) {
            if (t < w) sh[t] += sh[t + w];
            __syncthreads();
        }
        const double r = sh[0];
        __syncthreads();
        return r;
    };
    double elpd = 0.0, ploo = 0.0, lppd = 0.0, high = 0.0, bad = 0.0, nonf = 0.0;
    for (long long i = t; i < p.N; i += kLooTotalsWG) {
        const double* r = p.point + (size_t)i * DEMC_LOO_NPOINT;
        elpd += r[0]; ploo += r[1]; lppd += r[3];
        high += r[2] > 0.7 ? 1.0 : 0.0;
        bad += r[2] > 1.0 ? 1.0 : 0.0;
        nonf += (isfinite(r[0]) && isfinite(r[3])) ? 0.0 : 1.0;
    }
    elpd = block_sum(elpd); ploo = block_sum(ploo); lppd = block_sum(lppd); high = block_sum(high); bad = block_sum(bad); nonf = block_sum(nonf);
    const double N = (double)p.N, ebar = elpd / N;
    double ss = 0.0;
    for (long long i = t; i < p.N; i += kLooTotalsWG) {
        const double dv = p.point[(size_t)i * DEMC_LOO_NPOINT] - ebar;
        ss += dv * dv;
    }
    ss = block_sum(ss);
    if (t == 0) {
        p.total[0] = elpd;
        p.total[1] = sqrt(N * (ss / (N - 1.0)));  // (N = 1: 0 / 0)
        p.total[2] = ploo;
        p.total[3] = lppd;
        p.total[4] = -2.0 * elpd;
        p.total[5] = high;
        p.total[6] = bad;
        p.total[7] = nonf;
    }
}

// false: no instance for (family, X) -- a missing kernel is an error, not a detour
bool launch_terms(const PwKParams& p, const dim3& grid, hipStream_t st, long long obs0, int nb) {
    const int x = pw_instance_x(p);
#define DEMC_Y_(F, X)                                                                                                            \
    if (p.fam == F && x == X) {                                                                                                  \
        hipLaunchKernelGGL((k_loo_terms<F, X>), grid, dim3(kPwWG), 0, st, p, (const double*)p.cst, p.matrix, obs0, nb);         \
        return true;                                                                                                             \
    }
    DEMC_PW_INSTANCES(DEMC_Y_)
#undef DEMC_Y_
    return false;
}

}  // namespace

int loo_run(const PwModelView& mv, const HistView& v, const LooPlan& plan, hipStream_t st, double* total_out, double* point_out, std::string& err) {
    const char* who = "demc_loo";
    PwKParams p = pw_base_params(mv, plan.fam);
    p.S = plan.S; p.K = plan.K; p.chunk_len = plan.chunk_len; p.chunks = plan.chunks;
    p.theta = v.hist + (size_t)v.row0 * v.P * v.ld;
    p.ld = v.ld; p.D = v.D; p.bounds = nullptr;
    Scratch s;
    if (!(s.get(&p.cst, plan.n_cst) && s.get(&p.matrix, plan.n_terms) && s.get(&p.point, plan.n_point) && s.get(&p.total, plan.n_total))) {
        err = "demc_loo: out of device memory for the scratch buffers";
        return DEMC_ENOMEM;
    }
    if (hipFuncSetAttribute((const void*)k_loo_column, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes) != hipSuccess) {
        err = "demc_loo: the LDS limit of a kernel could not be raised";
        return DEMC_EHIP;
    }
    PassTrace tr;  // (the diagnostic variant: device time of the preparation, then of the two passes of every block, then the totals)
    bool ok = tr.mark(st);
    hipLaunchKernelGGL(k_loo_prepare, dim3((unsigned)plan.prep_blocks), dim3(kPwPrepWG), 0, st, p);
    ok = ok && tr.mark(st);
    for (int b = 0; b < plan.blocks; ++b) {
        const long long obs0 = (long long)b * plan.Nb;
        const int nb = (int)std::min<long long>(plan.Nb, p.N - obs0);
        const dim3 grid((unsigned)((nb + kLooObs - 1) / kLooObs), (unsigned)plan.chunks);
        if (!launch_terms(p, grid, st, obs0, nb)) { err = "demc_loo: no k_loo_terms instance for this model"; return DEMC_EUNSUPPORTED; }
        ok = ok && tr.mark(st);
        hipLaunchKernelGGL(k_loo_column, dim3((unsigned)nb), dim3(kLooWG), plan.lds_bytes, st, p, (const double*)p.matrix, obs0, plan.M);
        ok = ok && tr.mark(st);
    }
    hipLaunchKernelGGL(k_loo_totals, dim3(1), dim3(kLooTotalsWG), 0, st, p);
    ok = ok && tr.mark(st);
    if (!ok) { err = "demc_loo: an event could not be recorded"; return DEMC_EHIP; }
    if (!finish(who, st, {{total_out, p.total, plan.n_total * sizeof(double)}, {point_out, p.point, plan.n_point * sizeof(double)}}, err)) return DEMC_EHIP;
    tr.print(who, 2 + 2 * plan.blocks, 1);
    return DEMC_OK;
}

}  // namespace demc
