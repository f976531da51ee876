// demc_quantile.hpp -- posterior quantiles on the device (include/demc_quantile.h: demc_quantiles; the definition is DESIGN.md 5.6):
// an exact MSD radix select over the slot-keyed history.  Quantiles pool the chains, so no inverse id map is needed and the history
// is read straight through.  Nothing but the (D+2) x n_probs results goes to the host, and nothing is read back between the passes.
//
// Keys: k(x) = bits(x) ^ (sign ? ~0 : 1 << 63), compared unsigned: the IEEE order with -0.0 before +0.0, NaNs beyond the infinities.
// Targets: every prob needs the order statistics x_(j) and x_(j+1); the host turns the probs into T <= 32 distinct 0-based ranks,
// ascending, the same for every series (all pools have N = n P values).  Target t of series s carries, on the device, the high
// bits of its key found so far and its remaining rank inside the bucket of that prefix.  Targets with the same prefix form a GROUP
// (gprefix[s][g], ascending in g; tgrp[s][t]): histograms are per group, not per target -- in the first pass every series has
// one group, and adjacent ranks stay in one group until the digit at which they part.
//
// One pass per digit of kQBits = 8 bits, most significant first (8 passes):
//   k_q_hist   streams hist rows [row0,row1) -- consecutive lanes on consecutive doubles, columns >= D of a padded cell skipped --
//              then acc_hist and lp_hist.  A value whose high bits match a group of its series counts its next digit into that
//              group's histogram.
//   k_q_scan   a workgroup per series, a wave per target in turn: prefix sum of the group's 256 counts, the bin the remaining rank
//              falls into extends the prefix and reduces the rank; the series' groups are formed again and its table is cleared.
// k_q_final flags series that hold a NaN (seen by the first pass), turns keys back into values and interpolates.
//
// Geometry of k_q_hist: kQWG = 512 threads.  A CHUNK is cpi = kQWG / min(ld, kQWG) whole cells (cpi * ld <= kQWG lanes are busy):
// lane l works on column l % ld of cell l / ld of the chunk, and a workgroup takes the chunks b, b + W, b + 2W, ... of its W =
// min(chunks, kQMaxWG) fellows -- so a lane stays on ONE series for all its iterations.  (Cells wider than kQWG are walked in
// column blocks of kQWG.)  acc and lp are streamed kQWG values per iteration.  Because the top digits of a parameter are nearly
// constant, a lane keeps (bin, run length) in registers and touches a histogram only when the bin changes or at its end: a pass
// over a constant digit costs one atomic per lane, not one per value.  In the later passes few values match any group: a lane
// holds a 64-bit filter over the six key bits just above the digit (set for the prefixes of its series' groups) and searches the
// ascending prefixes only for the values that pass it.
// Histograms: up to kQSlots tables of 256 32-bit counts in LDS (64 KiB), CLAIMED by the groups a workgroup meets: group g of series
// s has the id g (D+2) + s, looks at the kQProbes slots from id % slots on and takes the first that is free or already its own
// (a compare-and-swap on the slot's owner word).  The groups that are counted often claim early, whichever series they belong to --
// acceptance is two values, so its second group holds a quarter of the pool in EVERY pass --, and a group that finds no slot is
// counted in the global table directly (few values by then, or more series than tables).  At its end a workgroup adds its non-zero
// LDS counts into the global 64-bit table.  All adds are integer atomics, hence exact: neither the result nor any count depends
// on arrival order or on which group won a slot.
// Counters: LDS counts and run lengths are 32-bit.  One workgroup counts at most ceil(chunks / W) * kQWG values of a series per pass;
// the host refuses a call in which that reaches 2^32 (kQMaxChunksPerWG = 2^22 chunks, i.e. a history of 2^40 doubles and more:
// beyond any device's memory).  Global counts and ranks are 64-bit: N = n P may exceed 2^32.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "demc_postplan.hpp"  // host-only: the kQ* constants, QTargets, HistView, QuantilePlan

namespace demc {

struct QKParams {
    const double* hist;          // [n_rows][P][ld]
    const unsigned char* acc;    // [n_rows][P]
    const double* lp;            // [n_rows][P]
    long long P, row0, n;
    int D, ld, T, slots;         // T targets per series; slots: LDS tables of this launch (a power of two)
    unsigned long long* table;   // [D+2][T][256] counts of the pass (group-major within a series)
    unsigned long long* gprefix; // [D+2][T] the distinct prefixes of a series, ascending (low bits zero)
    unsigned long long* trank;   // [D+2][T] remaining 0-based rank of a target inside its group's bucket
    int* tgrp;                   // [D+2][T] group of a target
    int* ng;                     // [D+2] groups of a series
    int* nanflag;                // [D+2] the pool holds a NaN
    double* out;                 // [D+2][n_probs]
};

// host: what plan_quantiles planned for the rows of `v`, on `stream`; 0 or a DEMC_* code with a message
int quantile_run(const HistView& v, const QuantilePlan& plan, hipStream_t stream, double* out, std::string& err);

#ifdef DEMC_QUANTILE_KERNELS  // (demc_quantile.cpp only: the runtime's unit sees the declarations above and no device code)
__device__ __forceinline__ unsigned long long q_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : 1ull << 63);
}

__device__ __forceinline__ double q_value(unsigned long long k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 1ull << 63 : ~0ull)));
}

__global__ __launch_bounds__(256) void k_q_init(QKParams p, QTargets tg) {
    const int D2 = p.D + 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)D2 * p.T) return;
    const int t = (int)(i % p.T);
    p.gprefix[i] = 0;
    p.tgrp[i] = 0;
    p.trank[i] = tg.rank[t];
    if (t == 0) { p.ng[i / p.T] = 1; p.nanflag[i / p.T] = 0; }
}

struct QLane {  // what a lane keeps while it stays on series s
    const unsigned long long* gp;  // the prefixes of the series' groups
    unsigned long long lo, hi;     // ... the first and the last of them
    unsigned long long bm;         // bit d: some group's prefix has d in the six bits above the digit (a filter before the search)
    int s, ngs;
    int bin;                       // the run: g * 256 + digit, -1: none
    unsigned int cnt;
    int slot_g, slot;              // the LDS table of group slot_g (-1: it has none), looked up once per change of group
};

// the slot of group id: the first of kQProbes that is free (claimed here) or already this group's; -1: none
__device__ __forceinline__ int q_claim(int* owner, int slots, int id) {
    for (int k = 0; k < kQProbes; ++k) {
        const int h = (id + k) & (slots - 1);
        int o = owner[h];
        if (o == 0) {
            o = atomicCAS(&owner[h], 0, id + 1);
            if (o == 0) return h;
        }
        if (o == id + 1) return h;
    }
    return -1;
}

__device__ __forceinline__ void q_flush(const QKParams& p, unsigned int* lds, QLane& l) {
    if (l.bin < 0) return;
    const int g = l.bin >> kQBits, d = l.bin & 255;
    if (g != l.slot_g) {
        l.slot_g = g;
        l.slot = q_claim((int*)(lds + p.slots * 256), p.slots, g * (p.D + 2) + l.s);
    }
    if (l.slot >= 0) atomicAdd(&lds[l.slot * 256 + d], l.cnt);
    else atomicAdd(&p.table[((size_t)l.s * p.T + g) * 256 + d], (unsigned long long)l.cnt);
}

template <bool FIRST>
__device__ __forceinline__ void q_begin(const QKParams& p, int s, int shift, QLane& l) {
    l.s = s; l.bin = -1; l.cnt = 0; l.slot_g = -1; l.slot = -1;
    l.gp = p.gprefix + (size_t)s * p.T;
    l.ngs = FIRST ? 1 : p.ng[s];
    l.lo = FIRST ? 0 : l.gp[0];
    l.hi = FIRST ? 0 : l.gp[l.ngs - 1];
    l.bm = 0;
    if (!FIRST)
        for (int g = 0; g < l.ngs; ++g) l.bm |= 1ull << ((l.gp[g] >> (shift + kQBits)) & 63);
}

template <bool FIRST>
__device__ __forceinline__ void q_count(const QKParams& p, unsigned int* lds, QLane& l, double x, int shift, unsigned long long mask) {
    const unsigned long long k = q_key(x);
    int g = 0;
    if (FIRST) {
        if (k < kQKeyNegInf || k > kQKeyPosInf) p.nanflag[l.s] = 1;  // (every writer writes the same word: no atomic)
    } else {
        if (!((l.bm >> ((k >> (shift + kQBits)) & 63)) & 1)) return;  // most values of the later passes leave here
        const unsigned long long kp = k & mask;
        if (kp < l.lo || kp > l.hi) return;
        for (;; ++g) {  // ascending prefixes
            if (g == l.ngs) return;
            const unsigned long long q = l.gp[g];
            if (q == kp) break;
            if (q > kp) return;
        }
    }
    const int bin = g * 256 + (int)((k >> shift) & 255);
    if (bin == l.bin) { ++l.cnt; return; }
    q_flush(p, lds, l);
    l.bin = bin;
    l.cnt = 1;
}

// one digit: bits [shift, shift + 8) of the keys whose higher bits are a group's prefix
template <bool FIRST>
__global__ __launch_bounds__(kQWG) void k_q_hist(QKParams p, int shift) {
    extern __shared__ unsigned int q_lds[];  // [slots][256] counts | [slots] owner: group id + 1, 0: free
    const int D2 = p.D + 2;
    for (int i = threadIdx.x; i < p.slots * 257; i += kQWG) q_lds[i] = 0;
    __syncthreads();
    const unsigned long long mask = FIRST ? 0ull : ~0ull << (shift + kQBits);  // (shift <= 48 here)
    const long long cells = p.n * p.P;
    const double* base = p.hist + (size_t)p.row0 * p.P * p.ld;
    QLane l;
    for (int cb = 0; cb < p.D; cb += kQWG) {  // a single block of columns unless cells are wider than the workgroup
        const int lc = min(p.ld - cb, kQWG), cpi = kQWG / lc;
        const int off = (int)threadIdx.x / lc, col = cb + (int)threadIdx.x - off * lc;
        if (off >= cpi || col >= p.D) continue;  // idle lanes of the chunk; padding columns of a cell
        q_begin<FIRST>(p, col, shift, l);
        for (long long c = (long long)blockIdx.x * cpi + off; c < cells; c += (long long)gridDim.x * cpi)
            q_count<FIRST>(p, q_lds, l, base[(size_t)c * p.ld + col], shift, mask);
        q_flush(p, q_lds, l);
    }
    const unsigned char* acc = p.acc + (size_t)p.row0 * p.P;
    const double* lp = p.lp + (size_t)p.row0 * p.P;
    q_begin<FIRST>(p, p.D, shift, l);
    for (long long c = (long long)blockIdx.x * kQWG + threadIdx.x; c < cells; c += (long long)gridDim.x * kQWG)
        q_count<FIRST>(p, q_lds, l, (double)acc[c], shift, mask);
    q_flush(p, q_lds, l);
    q_begin<FIRST>(p, p.D + 1, shift, l);
    for (long long c = (long long)blockIdx.x * kQWG + threadIdx.x; c < cells; c += (long long)gridDim.x * kQWG)
        q_count<FIRST>(p, q_lds, l, lp[c], shift, mask);
    q_flush(p, q_lds, l);
    __syncthreads();
    for (int i = threadIdx.x; i < p.slots * 256; i += kQWG) {
        const unsigned int v = q_lds[i];
        if (v == 0) continue;
        const int id = (int)q_lds[p.slots * 256 + (i >> 8)] - 1, s = id % D2, g = id / D2;
        atomicAdd(&p.table[((size_t)s * p.T + g) * 256 + (i & 255)], (unsigned long long)v);
    }
}

// a workgroup per series, a wave per target in turn
__global__ __launch_bounds__(256) void k_q_scan(QKParams p, int shift) {
    __shared__ unsigned long long np[kQMaxTargets];
    const int s = blockIdx.x, T = p.T, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ng_old = p.ng[s];
    for (int t = wave; t < T; t += 4) {
        const int g = p.tgrp[(size_t)s * T + t];
        const unsigned long long r = p.trank[(size_t)s * T + t], pre = p.gprefix[(size_t)s * T + g];
        const unsigned long long* h = p.table + ((size_t)s * T + g) * 256 + lane * 4;
        const unsigned long long c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
        unsigned long long incl = c0 + c1 + c2 + c3;
        const unsigned long long own = incl;
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long up = __shfl_up(incl, m, 64);
            if (lane >= m) incl += up;
        }
        unsigned long long before = incl - own;
        if (lane == 0) np[t] = pre;  // (counts that do not cover the rank cannot occur; the prefix would stay)
        if (r >= before && r < incl) {
            int d = 0;
            if (r >= before + c0) { before += c0; d = 1;
                if (r >= before + c1) { before += c1; d = 2;
                    if (r >= before + c2) { before += c2; d = 3; } } }
            np[t] = pre | ((unsigned long long)(lane * 4 + d) << shift);
            p.trank[(size_t)s * T + t] = r - before;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ng_old * 256; i += 256) p.table[(size_t)s * T * 256 + i] = 0;
    if (threadIdx.x == 0) {  // ranks ascend, so prefixes do: a group is a run of equal prefixes
        int g = -1;
        for (int t = 0; t < T; ++t) {
            if (t == 0 || np[t] != np[t - 1]) p.gprefix[(size_t)s * T + ++g] = np[t];
            p.tgrp[(size_t)s * T + t] = g;
        }
        p.ng[s] = g + 1;
    }
}

// a thread per (series, prob): DESIGN.md 5.6, to the operation (-ffp-contract=off: the expressions are the ones written)
__global__ __launch_bounds__(256) void k_q_final(QKParams p, QTargets tg) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)(p.D + 2) * tg.n_probs) return;
    const int s = (int)(i / tg.n_probs), k = (int)(i % tg.n_probs), T = p.T;
    const unsigned long long* gp = p.gprefix + (size_t)s * T;
    const int* tgp = p.tgrp + (size_t)s * T;
    const double a = q_value(gp[tgp[tg.ia[k]]]), b = q_value(gp[tgp[tg.ib[k]]]), gm = tg.gamma[k];
    double r;
    if (p.nanflag[s]) r = __longlong_as_double(0x7ff8000000000000LL);
    else if (tg.ia[k] == tg.ib[k]) r = a;
    else if (isfinite(a) && isfinite(b)) r = a + gm * (b - a);
    else if (gm == 0.0) r = a;
    else if (gm == 1.0) r = b;
    else r = (1.0 - gm) * a + gm * b;
    p.out[i] = r;
}
#endif  // DEMC_QUANTILE_KERNELS

}  // namespace demc
