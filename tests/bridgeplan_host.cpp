// bridgeplan_host.cpp -- csrc/demc_bridgeplan.hpp on the CPU: every refusal of demc_bridge with its code and text held literally and
// in the order they rank, the split of the window at R = 2, 3 and odd R, the chunks of P rows at N2 = 1, P - 1, P and P + 1 (every
// proposal draw in exactly one row, the padding counted), the transform against its own inverse, the Cholesky factorisation against a
// long double reference, the non-positive pivot, and the assembly of the outputs.  Built with the address and undefined-behaviour
// sanitizers by tests/test_bridge_host.py; no GPU, no HIP runtime, no ROCm header.
//
// bridgeplan_host --dump reads one request per line from stdin and prints what the header answers:
//   T theta lo hi        -> xi logJ theta_back (%.17g; inf / -inf / nan as printf writes them)
//   G R P D n_prop       -> plan_bridge's geometry for rows [0, R) of P draws: n_fit= N1= N2= W1= W2= chunks1= chunks2= pad2= last2= draw_blocks=
//                           solve_blocks= lds_bytes=, or refused=<code> message=<text>
#include "demc_bridgeplan.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

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

bool refused_with(const Refusal& r, int code, const std::string& text) { return r.code == code && r.message == text; }

BridgeCall good() {
    BridgeCall c;
    c.stored = true; c.row0 = 0; c.row1 = 10; c.n_rows = 10; c.family = DEMC_FAM_GAUSSIAN; c.has_out = true; c.sharded = false; c.n_prop = 0; c.D = 2; c.P = 13;
    return c;
}

void refusals() {
    CHECK(!plan_bridge(good()).refused);
    // each refusal alone, then with everything that ranks behind it wrong as well: the earlier one answers
    BridgeCall all = good();
    all.stored = false; all.row1 = 11; all.family = -1; all.has_out = false; all.sharded = true; all.n_prop = -1; all.D = 65; all.P = 1;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "history is not stored on this handle"));
    all.stored = true;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "bad rows: demc_bridge needs at least two rows of the history"));
    for (auto rows : {std::pair<long long, long long>{-1, 3}, {2, 2}, {2, 3}, {3, 2}, {0, 11}, {9, 10}}) {
        BridgeCall c = good();
        c.row0 = rows.first; c.row1 = rows.second;
        CHECK(refused_with(plan_bridge(c).refused, DEMC_EINVAL, kBridgeBadRows));
    }
    all.row1 = 10;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "demc_bridge: no model is set on this handle"));
    all.family = kBridgeFamSim;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EUNSUPPORTED,
                       "demc_bridge: a simulation likelihood (demc_set_model_sim) gives a noisy log posterior; bridge sampling needs an exact one"));
    all.family = DEMC_FAM_HIER_GAUSSIAN;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "demc_bridge: out is NULL"));
    all.has_out = true;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "sharded handle: demc_bridge reads the whole history of one handle"));
    all.sharded = false;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "demc_bridge: n_prop must be >= 0 (0: as many proposal draws as the estimate half holds)"));
    all.n_prop = (long long)DEMC_BRIDGE_MAX_DRAWS + 1;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL, "demc_bridge: D = 65 is above the cap of 64 (DEMC_BRIDGE_MAX_D: the covariance of the proposal)"));
    all.D = 5;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL,
                       "demc_bridge: the fit half holds N_fit = 5 draws, the covariance of the proposal needs more than D = 5; pass a wider window"));
    all.D = 4;
    CHECK(refused_with(plan_bridge(all).refused, DEMC_EINVAL,
                       "demc_bridge: N1 = 5 and N2 = 4194305 draws: one is above the cap of 4194304 (DEMC_BRIDGE_MAX_DRAWS); pass a narrower window or a smaller n_prop"));
    all.n_prop = DEMC_BRIDGE_MAX_DRAWS;
    CHECK(!plan_bridge(all).refused);
    BridgeCall wide = good();
    wide.P = 1 << 20; wide.n_rows = wide.row1 = 10;  // N1 = 5 * 2^20 > 2^22
    CHECK(plan_bridge(wide).refused.code == DEMC_EINVAL && plan_bridge(wide).refused.message.find("N1 = 5242880") != std::string::npos);
    // every served family, the user-source model (DEMC_FAM_USER) and the ODE family among them
    for (int fam : {DEMC_FAM_GAUSSIAN, DEMC_FAM_MVN_ISO, DEMC_FAM_MVN_FULL, DEMC_FAM_BINOMIAL, DEMC_FAM_HIER_BINOMIAL, DEMC_FAM_HIER_GAUSSIAN, DEMC_FAM_LBA, DEMC_FAM_LNR,
                    DEMC_FAM_RASTRIGIN, DEMC_FAM_USER, DEMC_FAM_ODE_LV}) {
        BridgeCall c = good();
        c.family = fam;
        CHECK(!plan_bridge(c).refused);
    }
    // the run-time refusals
    CHECK(refused_with(bridge_bad_draws(3, (1 * 4 + 2) * 2 + 1, 0, 4, 2), DEMC_EINVAL,
                       "demc_bridge: 3 scalar(s) of the window lie on or outside a finite bound or are NaN (the first: row 1, slot 2, scalar 1); the transform to "
                       "the real line needs every draw strictly inside the bounds"));
    CHECK(bridge_bad_draws(1, 0, 7, 4, 2).message.find("(the first: row 7, slot 0, scalar 0)") != std::string::npos);
    CHECK(refused_with(bridge_bad_pivot(0, 2), DEMC_EINVAL,
                       "demc_bridge: the covariance of the fit half is not positive definite (pivot 0 of 2 is not positive): a scalar is constant or the draws are "
                       "collinear"));
    CHECK(DEMC_BRIDGE_NOUT == 12 && DEMC_BRIDGE_MAX_D == 64 && DEMC_BRIDGE_MAX_DRAWS == 4194304 && kBridgeStream == 7 && kBridgeMaxIter == 1000);
}

void split_and_chunks() {
    struct { long long row0, row1, rmid; } cases[] = {{0, 2, 1}, {0, 3, 1}, {5, 8, 6}, {0, 7, 3}, {3, 12, 7}, {0, 10, 5}, {2, 103, 52}};
    for (const auto& k : cases) {
        BridgeCall c = good();
        c.P = 3; c.D = 1; c.n_rows = 200; c.row0 = k.row0; c.row1 = k.row1;
        if (k.rmid - k.row0 == 0) continue;
        const BridgePlan p = plan_bridge(c);
        if ((k.rmid - k.row0) * c.P <= c.D) { CHECK((bool)p.refused); continue; }
        CHECK(!p.refused && p.rmid == k.rmid && p.R == k.row1 - k.row0 && p.n_fit == (k.rmid - k.row0) * 3 && p.N1 == (k.row1 - k.rmid) * 3);
        CHECK(p.n_fit + p.N1 == p.n_win && p.N1 >= p.n_fit && p.N1 - p.n_fit <= 3 && p.N2 == p.N1 && p.chunks1 * 3 == p.N1);
        CHECK(p.s1 == 0.5 && p.s2 == 0.5);
    }
    {  // R = 2 at Np = 3: one row each
        BridgeCall c = good();
        c.P = 3; c.D = 2; c.row1 = 2;
        const BridgePlan p = plan_bridge(c);
        CHECK(!p.refused && p.n_fit == 3 && p.N1 == 3 && p.rmid == 1);
    }
    const long long P = 13;
    for (long long n2 : {1LL, P - 1, P, P + 1, 2 * P, 1000LL, (long long)DEMC_BRIDGE_MAX_DRAWS}) {
        BridgeCall c = good();
        c.P = P; c.n_prop = n2;
        const BridgePlan p = plan_bridge(c);
        CHECK(!p.refused && p.N2 == n2 && p.chunks2 == (n2 + P - 1) / P && p.pad2 == p.chunks2 * P && p.pad2 >= n2 && p.pad2 - n2 < P);
        CHECK(p.last2 >= 1 && p.last2 <= P && (p.chunks2 - 1) * P + p.last2 == n2);
        CHECK(p.draw_blocks * (long long)kBridgeLane >= p.pad2 && (p.draw_blocks - 1) * (long long)kBridgeLane < p.pad2);
        CHECK(p.solve_blocks * (long long)kBridgeLane >= p.N1 && p.W1 >= 1 && p.W2 >= 1 && p.W1 <= kBridgeMaxW && p.W2 <= kBridgeMaxW);
        CHECK(p.s1 + p.s2 == 1.0 || std::fabs(p.s1 + p.s2 - 1.0) < 1e-15);
        CHECK(p.lds_bytes == (size_t)c.D * kBridgeLane * 8 && p.lds_bytes <= 32768);
    }
    CHECK(plan_bridge(good()).chunks2 == 5 && plan_bridge(good()).pad2 == 65 && plan_bridge(good()).last2 == 13);
    CHECK(bridge_workers(1) == 1 && bridge_workers(1024) == 1 && bridge_workers(1025) == 2 && bridge_workers(DEMC_BRIDGE_MAX_DRAWS) == kBridgeMaxW);
}

void transform() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(bridge_kind(-inf, inf) == BK_NONE && bridge_kind(0, inf) == BK_LOWER && bridge_kind(-inf, 1) == BK_UPPER && bridge_kind(0, 1) == BK_BOTH);
    CHECK(bridge_kind(nan, nan) == BK_NONE);
    const double bounds[][2] = {{-inf, inf}, {0.0, inf}, {-2.5, inf}, {-inf, 6.0}, {0.0, 1.0}, {-3.0, 0.25}};
    for (const auto& b : bounds)
        for (double xi : {-700.0, -40.0, -3.0, -1e-9, 0.0, 0.5, 2.0, 30.0}) {
            const int kind = bridge_kind(b[0], b[1]);
            if (kind != BK_BOTH && kind != BK_NONE && xi > 300) continue;
            const double th = bridge_inverse(xi, b[0], b[1]);
            CHECK(std::isfinite(th) && th >= b[0] && th <= b[1]);
            const double back = bridge_forward(th, b[0], b[1]);
            const bool at_bound = th == b[0] || th == b[1];
            if (!at_bound && std::fabs(xi) <= 3.0) CHECK(std::fabs(back - xi) <= 1e-9 * std::max(1.0, std::fabs(xi)));
            if (at_bound) CHECK(!std::isfinite(back));
            const double lj = bridge_logjac(xi, b[0], b[1]);
            CHECK(std::isfinite(lj));
            if (kind == BK_NONE) CHECK(lj == 0.0 && th == xi);
            if (kind == BK_LOWER || kind == BK_UPPER) CHECK(lj == xi);
            if (kind == BK_BOTH) CHECK(lj <= std::log(b[1] - b[0]) - std::log(4.0) + 1e-15);
        }
    CHECK(bridge_forward(0.0, 0.0, inf) == -inf && std::isnan(bridge_forward(-1.0, 0.0, inf)) && std::isnan(bridge_forward(nan, -inf, inf)));
    CHECK(bridge_forward(1.0, 0.0, 1.0) == inf && bridge_forward(0.0, 0.0, 1.0) == -inf && std::isnan(bridge_forward(1.5, 0.0, 1.0)));
    CHECK(bridge_forward(6.0, -inf, 6.0) == -inf && std::isnan(bridge_forward(7.0, -inf, 6.0)));
}

void cholesky() {
    // V = A A' / n + 0.1 I from a fixed linear congruential sequence, against the same recurrence in long double
    unsigned long long s = 12345;
    auto next = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) / 9007199254740992.0 - 0.5; };
    for (int D : {1, 2, 3, 7, 8, 33, 64}) {
        std::vector<double> A((size_t)D * D), V((size_t)D * D), L((size_t)D * D, -1.0);
        for (double& a : A) a = next();
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                long double t = i == j ? 0.1L : 0.0L;
                for (int k = 0; k < D; ++k) t += (long double)A[(size_t)i * D + k] * A[(size_t)j * D + k] / D;
                V[(size_t)i * D + j] = (double)t;
            }
        CHECK(bridge_cholesky(V.data(), D, L.data()) == -1);
        std::vector<long double> R((size_t)D * D, 0.0L);
        for (int j = 0; j < D; ++j) {
            long double d = V[(size_t)j * D + j];
            for (int k = 0; k < j; ++k) d -= R[(size_t)j * D + k] * R[(size_t)j * D + k];
            R[(size_t)j * D + j] = std::sqrt(d);
            for (int i = j + 1; i < D; ++i) {
                long double t = V[(size_t)i * D + j];
                for (int k = 0; k < j; ++k) t -= R[(size_t)i * D + k] * R[(size_t)j * D + k];
                R[(size_t)i * D + j] = t / R[(size_t)j * D + j];
            }
        }
        double worst = 0.0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                if (j > i) CHECK(L[(size_t)i * D + j] == 0.0);
                worst = std::max(worst, (double)std::fabs((long double)L[(size_t)i * D + j] - R[(size_t)i * D + j]));
            }
        CHECK(worst <= 1e-13);
        // L L' gives V back
        double back = 0.0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j <= i; ++j) {
                long double t = 0.0L;
                for (int k = 0; k <= j; ++k) t += (long double)L[(size_t)i * D + k] * L[(size_t)j * D + k];
                back = std::max(back, (double)std::fabs(t - (long double)V[(size_t)i * D + j]));
            }
        CHECK(back <= 1e-14);
        long double ln = 0.5L * D * std::log(2.0L * 3.14159265358979323846264338327950288L);
        for (int k = 0; k < D; ++k) ln += std::log(R[(size_t)k * D + k]);
        CHECK(std::fabs(bridge_lognorm(L.data(), D) - (double)ln) <= 1e-12 * std::max(1.0, (double)std::fabs(ln)));
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double L4[4];
    const double zero[4] = {0.0, 0.0, 0.0, 1.0}, second[4] = {1.0, 1.0, 1.0, 1.0}, neg[4] = {1.0, 2.0, 2.0, 1.0}, bad[4] = {nan, 0.0, 0.0, 1.0};
    CHECK(bridge_cholesky(zero, 2, L4) == 0 && bridge_cholesky(second, 2, L4) == 1 && bridge_cholesky(neg, 2, L4) == 1 && bridge_cholesky(bad, 2, L4) == 0);
    const double infm[4] = {std::numeric_limits<double>::infinity(), 0.0, 0.0, 1.0};
    CHECK(bridge_cholesky(infm, 2, L4) == 0);
}

void outputs() {
    BridgeCall c = good();
    const BridgePlan p = plan_bridge(c);
    double val[BV_COUNT] = {};
    unsigned long long word[BW_COUNT] = {};
    val[BV_R] = 2.0; val[BV_LSTAR] = -10.0; val[BV_MEAN1] = 0.5; val[BV_MEAN2] = 0.25; val[BV_SS1] = 6.4; val[BV_SS2] = 1.6; val[BV_REL] = 1e-12;
    word[BW_FLAG] = BF_CONVERGED; word[BW_ITER] = 7; word[BW_ZERO] = 3;
    double out[DEMC_BRIDGE_NOUT];
    bridge_outputs(p, val, word, out);
    CHECK(out[0] == std::log(2.0) - 10.0 && out[3] == 7 && out[4] == 1 && out[5] == 65 && out[6] == 65 && out[7] == 65 && out[8] == -10.0 && out[9] == 3 && out[10] == 0);
    CHECK(out[1] == 6.4 / 64.0 / 0.25 / 65.0 && out[2] == 1.6 / 64.0 / 0.0625 / 65.0 && out[11] == 1e-12);
    word[BW_NONFINITE] = 1; word[BW_FLAG] = BF_STOPPED; word[BW_ITER] = 0;
    bridge_outputs(p, val, word, out);
    CHECK(std::isnan(out[0]) && std::isnan(out[1]) && std::isnan(out[2]) && std::isnan(out[11]) && out[3] == 0 && out[4] == 0 && out[10] == 1 && out[8] == -10.0);
    // an iterate that is not a positive finite number: the iteration stopped there and is counted, nothing converged whatever the flag
    // says (the kernel's test holds at +Inf), logml, the error terms and the last change are NaN, the counts and l* stay
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double r : {0.0, -0.0, inf, nan, -1.0, -inf})
        for (unsigned long long flag : {(unsigned long long)BF_STOPPED, (unsigned long long)BF_CONVERGED, (unsigned long long)BF_RUNNING}) {
            word[BW_NONFINITE] = 0; word[BW_FLAG] = flag; word[BW_ITER] = 23; word[BW_ZERO] = 3;
            val[BV_R] = r; val[BV_REL] = r == 0.0 ? inf : nan;
            bridge_outputs(p, val, word, out);
            CHECK(std::isnan(out[0]) && std::isnan(out[1]) && std::isnan(out[2]) && std::isnan(out[11]));
            CHECK(out[3] == 23 && out[4] == 0 && out[5] == 65 && out[6] == 65 && out[7] == 65 && out[8] == -10.0 && out[9] == 3 && out[10] == 0);
        }
    // ... and the smallest positive r is a result like any other
    word[BW_FLAG] = BF_CONVERGED; val[BV_R] = std::numeric_limits<double>::denorm_min(); val[BV_REL] = 0.0;
    bridge_outputs(p, val, word, out);
    CHECK(out[0] == std::log(val[BV_R]) - 10.0 && out[4] == 1 && std::isfinite(out[1]) && std::isfinite(out[2]) && out[11] == 0.0);
}

int dump() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, a, b, c;
        in >> what;
        if (what == "G") {
            BridgeCall k = good();
            long long R = 0, P = 0, D = 0, n_prop = 0;
            in >> R >> P >> D >> n_prop;
            k.row0 = 0; k.row1 = k.n_rows = R; k.P = P; k.D = (int)D; k.n_prop = n_prop;
            const BridgePlan g = plan_bridge(k);
            if (g.refused) { std::printf("refused=%d message=%s\n", g.refused.code, g.refused.message.c_str()); continue; }
            std::vector<int32_t> cols((size_t)D);  // the fit as the runtime plans it: every scalar of xi
            for (long long j = 0; j < D; ++j) cols[(size_t)j] = (int32_t)j;
            const CovPlan f = plan_cov(g.n_fit, (int)D, cols.data(), (int)D);
            std::printf("n_fit=%lld N1=%lld N2=%lld W1=%d W2=%d chunks1=%lld chunks2=%lld pad2=%lld last2=%lld draw_blocks=%d solve_blocks=%d lds_bytes=%zu "
                        "cov_chunks=%lld cov_workers=%d\n",
                        g.n_fit, g.N1, g.N2, g.W1, g.W2, g.chunks1, g.chunks2, g.pad2, g.last2, g.draw_blocks, g.solve_blocks, g.lds_bytes, f.chunks, f.W);
            continue;
        }
        in >> a >> b >> c;
        if (what != "T") { std::printf("?\n"); continue; }
        const double th = std::strtod(a.c_str(), nullptr), lo = std::strtod(b.c_str(), nullptr), hi = std::strtod(c.c_str(), nullptr);
        const double xi = bridge_forward(th, lo, hi);
        std::printf("%.17g %.17g %.17g\n", xi, bridge_logjac(xi, lo, hi), bridge_inverse(xi, lo, hi));
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--dump") == 0) return dump();
    refusals();
    split_and_chunks();
    transform();
    cholesky();
    outputs();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
