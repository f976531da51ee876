// direct_four_plan.cpp -- plan_loglike's choice between k_direct_mvn<32> (two proposals per lane, blocks of 256) and
// k_direct_mvn<32>x4 (four per lane, blocks of 512) on the CPU (csrc/demc_geometry.hpp): the chunk count is the two-per-lane
// rule's at every shape, whichever body runs; the four-per-lane body is taken exactly where ceil(n_prop / 512) * n_chunks
// workgroups reach its resident count on the chip.  Built with the sanitizers by tests/test_direct_four_plan.py; no GPU.
#include "demc_geometry.hpp"

#include <cstdio>

namespace {
using namespace demc;

int failures = 0, checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++checks;                                                                    \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

// MvNormal full-Sigma in DIRECT mode, d = D, on 256 CUs with a 64-plane partial workspace
struct Case {
    demc_config c{};
    ModelShape m;
    Setup s;
    Case(int d, long long N) {
        c.loglike_mode = DEMC_LOGLIKE_DIRECT; c.D = d;
        m.N = N; m.d = d; m.dpad = d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : 32; m.dp_direct = m.dpad < 8 ? 8 : m.dpad;
        s.c = &c; s.m = &m; s.family = FAM_MVN_FULL; s.partial_cap = 64; s.n_cus = 256;
    }
};

// the chunk rule as the two-per-lane kernel alone had it: blocks of 256, its own occupancy
int parent_chunks(long long n_prop, long long N, int occ2) {
    long long cap = N / 64;
    if (cap > 64) cap = 64;
    if (cap < 1) cap = 1;
    return chunks_filling_rounds((n_prop + 255) / 256, cap, (double)occ2 * 256);
}

void check_shape(long long n_prop, long long N, unsigned want_x, int want_chunks, int want_body) {
    Occupancy occ;
    occ.direct = 6; occ.direct4 = 3;
    Case k(32, N);
    const LoglikePlan p = plan_loglike(k.s, n_prop, occ);
    CHECK(p.kind == K2_DIRECT_MVN && !p.refused && p.key[0] == 32);
    if (p.grid_x != want_x || p.n_chunks != want_chunks || p.key[1] != want_body)
        std::fprintf(stderr, "n_prop %lld N %lld: (%u, %d, %d)\n", n_prop, N, p.grid_x, p.n_chunks, p.key[1]);
    CHECK(p.grid_x == want_x && p.n_chunks == want_chunks && p.grid_y == (unsigned)want_chunks && p.n_partials == want_chunks);
    CHECK(p.key[1] == want_body);
    CHECK(p.n_chunks == parent_chunks(n_prop, N, 6));
}

void check_rule() {
    // the headline: 256 x 128 moving particles, N = 1e5 -> 64 blocks of 512 x 48 chunks = 4 x 768
    check_shape(32768, 100000, 64, 48, 4);
    // a population that cannot fill the chip with fat workgroups keeps the thin ones
    check_shape(2048, 2048, 8, 32, 0);
    check_shape(6300, 4000, 13, 61, 4);
    // the shapes of tests/test_gpu_direct_four.py: 12 x 64 = 768 is the first count that qualifies, 11 x 64 does not
    check_shape(6144, 4096, 12, 64, 4);
    check_shape(6144, 4161, 12, 64, 4);
    check_shape(6144, 4159, 12, 64, 4);
    check_shape(6145, 4096, 13, 61, 4);
    check_shape(6143, 4096, 12, 64, 4);
    check_shape(5632, 4096, 22, 64, 0);
    // every shape: the parent's chunk count; the body by the stated inequality; the grid covers the proposals exactly once
    Occupancy occ;
    occ.direct = 6; occ.direct4 = 3;
    for (long long N : {64LL, 1000LL, 4096LL, 100000LL})
        for (long long n_prop = 1; n_prop <= 40000; n_prop += (n_prop < 600 ? 1 : 97)) {
            Case k(32, N);
            const LoglikePlan p = plan_loglike(k.s, n_prop, occ);
            const int nc = parent_chunks(n_prop, N, 6);
            const bool four = ((n_prop + 511) / 512) * nc >= 3 * 256;
            CHECK(p.n_chunks == nc && p.n_partials == nc && p.grid_y == (unsigned)nc);
            CHECK(p.key[1] == (four ? 4 : 0));
            const long long per_block = four ? 512 : 256;
            CHECK((long long)p.grid_x * per_block >= n_prop && ((long long)p.grid_x - 1) * per_block < n_prop);
        }
    // no such instance in the library (occupancy not set), or another row length: the two-per-lane plan, untouched
    occ.direct4 = 0;
    {
        Case k(32, 100000);
        const LoglikePlan p = plan_loglike(k.s, 32768, occ);
        CHECK(p.key[1] == 0 && p.grid_x == 128 && p.n_chunks == 48);
    }
    occ.direct4 = 3;
    for (int d : {8, 16}) {
        Case k(d, 100000);
        const LoglikePlan p = plan_loglike(k.s, 32768, occ);
        CHECK(p.key[0] == d && p.key[1] == 0 && p.grid_x == 128 && p.n_chunks == parent_chunks(32768, 100000, 6));
    }
}
}  // namespace

int main() {
    check_rule();
    std::printf("%d checks, %d failures\n", checks, failures);
    if (failures) return 1;
    std::printf("direct four plan ok\n");
    return 0;
}
