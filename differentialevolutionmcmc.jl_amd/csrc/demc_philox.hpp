// demc_philox.hpp -- the counter-based RNG of the path: Philox4x32-10, the draw addressing and the integer picks built on its words.
// One text for the kernels (demc_device.hpp includes it) and for the host-only code that re-draws the device's coins
// (demc_schedule.hpp): plain C++ apart from the one macro below, no header but <stdint.h>.
//
// RNG contract (DESIGN.md "Randomness"): the reference consumes Julia's task-local Xoshiro
// stream in a fixed order.  A fused kernel cannot share one sequential
// stream, so every draw is addressed instead:
//     Philox4x32-10( key = seed,
//                    ctr = (block, entity, iteration, stream<<24 | sweep) )
// entity = global group index or global slot index, so results do not depend on how groups
// are sharded over GPUs.  One block = 4 x u32 = two 53-bit uniforms.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DEMC_HD __host__ __device__
#else
#define DEMC_HD
#endif

namespace demc {

enum Stream : uint32_t { S_STEP = 1, S_GROUP = 2, S_PART = 3, S_NOISE = 4, S_RECOMB = 5, S_MIG = 6 };

struct U4 {
    uint32_t x, y, z, w;
};

DEMC_HD inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

DEMC_HD inline U4 draw_block(uint64_t seed, uint32_t stream, uint32_t sweep, uint64_t iter, uint32_t entity,
                             uint32_t block) {
    U4 c;
    c.x = block;
    c.y = entity;
    c.z = (uint32_t)iter;
    c.w = (stream << 24) | (sweep & 0xFFFFu);
    return philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 53-bit uniform in [0,1), the resolution of Julia's rand(Float64)
DEMC_HD inline double u53(uint32_t lo, uint32_t hi) {
    const uint64_t x = ((uint64_t)hi << 32) | lo;
    return (double)(x >> 11) * (1.0 / 9007199254740992.0);
}
// 32-bit uniform in (0,1) from ONE word: the per-scalar draws (crossover noise b ~ U(-eps, eps), recombination coins, the
// Box-Muller inputs of the mutation noise) -- four scalars per Philox block: block m of the NOISE / RECOMB streams covers
// scalars 4m..4m+3 (word 2(k&1)+e for scalar e of dim pair k).  2^-32 resolution is ample for a jitter of scale eps.
DEMC_HD inline double u32unit(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }
DEMC_HD inline uint32_t mulhi32(uint32_t x, uint32_t m) { return (uint32_t)(((uint64_t)x * m) >> 32); }

// StatsBase.samplepair: i1 = rand(1:m); i2 = rand(1:m-1); i2 == i1 ? m : i2
DEMC_HD inline void pick_pair(uint32_t r0, uint32_t r1, uint32_t m, uint32_t& i1, uint32_t& i2) {
    i1 = mulhi32(r0, m);
    uint32_t b = mulhi32(r1, m - 1);
    if (b == i1) b = m - 1;
    i2 = b;
}
// ordered 3-of-m without replacement (rank shift)
DEMC_HD inline void pick_triple(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t m, uint32_t& i1, uint32_t& i2,
                                uint32_t& i3) {
    const uint32_t a = mulhi32(r0, m);
    uint32_t b = mulhi32(r1, m - 1);
    if (b >= a) ++b;
    uint32_t c = mulhi32(r2, m - 2);
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    if (c >= lo) ++c;
    if (c >= hi) ++c;
    i1 = a;
    i2 = b;
    i3 = c;
}

}  // namespace demc
