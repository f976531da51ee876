// prep_host.cpp -- csrc/demc_prep.hpp on the CPU: what demc_set_model, demc_set_model_sim, demc_set_priors, demc_set_bounds and
// demc_set_blocks work out before anything is uploaded, against values formed here by other means (integer and rational
// arithmetic, restated definitions, long double), and every refusal with its code and its exact text.  Built with the address and
// undefined-behaviour sanitizers by tests/test_prep_host.py; no GPU, no HIP runtime, no ROCm header.
#include "demc_prep.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <limits>

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

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kLog2PiHere = 1.8378770664093454835606594728112, kLogPiHere = 1.1447298858494001741434273513531;

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

bool is_refusal(const Refusal& r, int code, const std::string& text, int line) {
    if (r.code == code && r.message == text) return true;
    std::fprintf(stderr, "line %d: refusal is (%d, \"%s\"), expected (%d, \"%s\")\n", line, r.code, r.message.c_str(), code, text.c_str());
    return false;
}
#define REFUSED(r, code, text) CHECK(is_refusal((r), (code), (text), __LINE__))

// a refused model carries nothing
bool empty_model(const PreparedModel& m) {
    return m.N == 0 && m.d == 0 && m.dpad == 0 && m.n_tiles == 0 && m.ks_t == 0 && m.c0 == 0.0 && m.c1 == 0.0 && m.data.empty() &&
           m.M.empty() && m.sx.empty() && m.xbar.empty() && m.Xf.empty();
}

// ---- MvNormal: Sigma = L L', L unit lower bidiagonal; x[i][k] = (7 i + 3 k) mod 5 -- every intermediate is exactly representable

struct Ladder { int d, ks_t, n_kpass, dpad, dp_direct; };  // written out, not computed
const Ladder kLadder[] = {{1, 1, 1, 4, 8},    {5, 2, 1, 8, 8},     {8, 2, 1, 8, 8},    {9, 4, 1, 16, 16},  {16, 4, 1, 16, 16},
                          {17, 8, 1, 32, 32}, {32, 8, 1, 32, 32},  {33, 16, 1, 64, 64}, {64, 16, 1, 64, 64}, {65, 16, 2, 128, 0}};

std::vector<double> bidiagonal_sigma(int d) {
    std::vector<long long> L((size_t)d * d, 0);
    for (int i = 0; i < d; ++i) {
        L[(size_t)i * d + i] = 1;
        if (i) L[(size_t)i * d + i - 1] = 1;
    }
    std::vector<double> S((size_t)d * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            long long s = 0;
            for (int k = 0; k < d; ++k) s += L[(size_t)i * d + k] * L[(size_t)j * d + k];
            S[(size_t)i * d + j] = (double)s;
        }
    return S;
}

void mvn_case(int family, const Ladder& ld, long long N, int mode) {
    const int d = ld.d, D = family == DEMC_FAM_MVN_ISO ? d + 1 : d;
    const bool direct = mode == DEMC_LOGLIKE_DIRECT, full = family == DEMC_FAM_MVN_FULL;
    std::vector<double> x((size_t)N * d);
    for (long long i = 0; i < N; ++i)
        for (int k = 0; k < d; ++k) x[(size_t)i * d + k] = (double)((7 * i + 3 * k) % 5);
    const std::vector<double> S = bidiagonal_sigma(d);
    const int64_t dims[2] = {N, d};
    const PreparedModel m = prepare_model(family, D, mode, x.data(), dims, 2, full ? S.data() : nullptr, full ? d * d : 0);
    CHECK(m.refused.code == DEMC_OK && m.refused.message.empty());
    if (m.refused) return;
    // the ladders
    CHECK(m.N == N && m.d == d && m.ks_t == ld.ks_t && m.n_kpass == ld.n_kpass && m.dpad == ld.dpad && m.n_tiles == (int)((N + 15) / 16));
    CHECK(m.dp_direct == (direct ? ld.dp_direct : 0) && m.n_acc == 0 && m.data2_off == 0 && m.c2 == 0.0);
    // integer arithmetic: column sums, the centred data times N, the whitened rows times N
    std::vector<long long> colsum(d, 0), xt((size_t)N * d), z((size_t)N * d);
    for (long long i = 0; i < N; ++i)
        for (int k = 0; k < d; ++k) colsum[k] += (7 * i + 3 * k) % 5;
    for (long long i = 0; i < N; ++i)
        for (int k = 0; k < d; ++k) xt[(size_t)i * d + k] = N * ((7 * i + 3 * k) % 5) - colsum[k];
    for (long long i = 0; i < N; ++i)
        for (int r = 0; r < d; ++r) {  // L^-1[r][k] = (-1)^(r - k), k <= r
            long long s = 0;
            for (int k = 0; k <= r; ++k) s += ((r - k) & 1 ? -1 : 1) * xt[(size_t)i * d + k];
            z[(size_t)i * d + r] = full ? s : xt[(size_t)i * d + r];
        }
    CHECK((int)m.xbar.size() == d && (int)m.sx.size() == d);
    for (int k = 0; k < d; ++k) {
        CHECK(m.xbar[k] == (double)colsum[k] / (double)N);  // a multiple of 1/32
        CHECK(m.xbar[k] * 32.0 == std::floor(m.xbar[k] * 32.0));
        CHECK(m.sx[k] == 0.0);
    }
    long long zz = 0;
    for (size_t e = 0; e < z.size(); ++e) zz += z[e] * z[e];
    CHECK(m.c1 == (double)zz / (double)(N * N));  // sum_i |z_i|^2
    CHECK(m.c0 == (full ? -0.5 * (double)N * (d * kLog2PiHere + 0.0) : 0.0));
    // the matrix slot: Sigma^-1[i][j] = (-1)^(i + j) (d - max(i, j)); DIRECT: (L^-1)'[r][c] = L^-1[c][r]
    if (!full)
        CHECK(m.M.empty());
    else {
        CHECK(m.M.size() == (size_t)d * d);
        int bad = 0;
        for (int r = 0; r < d && m.M.size() == (size_t)d * d; ++r)
            for (int c = 0; c < d; ++c) {
                const long long want = direct ? (r <= c ? ((c - r) & 1 ? -1 : 1) : 0) : (((r + c) & 1) ? -1 : 1) * (long long)(d - std::max(r, c));
                bad += !(m.M[(size_t)r * d + c] == (double)want);
            }
        CHECK(bad == 0);
    }
    // Xf[tile][kstep][lane] = x~[16 tile + (lane & 15)][4 kstep + (lane >> 4)], zero padded, one all-zero tile behind the last
    const int ksx = ld.dpad / 4, n_tiles = (int)((N + 15) / 16);
    CHECK(m.Xf.size() == ((size_t)n_tiles + 1) * ksx * 64);
    if (m.Xf.size() == ((size_t)n_tiles + 1) * ksx * 64) {
        int bad = 0;
        for (int t = 0; t <= n_tiles; ++t)
            for (int ks = 0; ks < ksx; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const long long i = 16LL * t + (l & 15);
                    const int k = 4 * ks + (l >> 4);
                    const double want = (t < n_tiles && i < N && k < d) ? (double)xt[(size_t)i * d + k] / (double)N : 0.0;
                    bad += !(m.Xf[((size_t)t * ksx + ks) * 64 + l] == want);
                }
        CHECK(bad == 0);
    }
    // the DIRECT rows: z_i (ISO: x~_i), padded with zeros to dp_direct; otherwise no data buffer
    if (!direct)
        CHECK(m.data.empty());
    else {
        const int DP = ld.dp_direct;
        CHECK(m.data.size() == (size_t)N * DP);
        if (m.data.size() == (size_t)N * DP) {
            int bad = 0;
            for (long long i = 0; i < N; ++i)
                for (int r = 0; r < DP; ++r) bad += !(m.data[(size_t)i * DP + r] == (r < d ? (double)z[(size_t)i * d + r] / (double)N : 0.0));
            CHECK(bad == 0);
        }
    }
}

void mvn_exact() {
    for (const Ladder& ld : kLadder) {
        const bool issue_d = ld.d == 1 || ld.d == 5 || ld.d == 8 || ld.d == 33 || ld.d == 65;
        for (long long N : {1LL, 16LL, 32LL}) {
            if (!issue_d && N != 16) continue;  // the lengths in between: the DIRECT row ladder alone
            if (issue_d) mvn_case(DEMC_FAM_MVN_FULL, ld, N, DEMC_LOGLIKE_STREAMING);
            if (issue_d && N == 32) mvn_case(DEMC_FAM_MVN_FULL, ld, N, DEMC_LOGLIKE_SUFFSTAT);
            if (ld.d <= 64) mvn_case(DEMC_FAM_MVN_FULL, ld, N, DEMC_LOGLIKE_DIRECT);
        }
    }
    for (int mode : {DEMC_LOGLIKE_STREAMING, DEMC_LOGLIKE_DIRECT})
        for (long long N : {1LL, 16LL, 32LL}) mvn_case(DEMC_FAM_MVN_ISO, kLadder[1], N, mode);  // d = 5, D = 6
    // logdet of the bidiagonal Sigma is exactly 0, its factor's inverse exactly +-1
    std::vector<double> Ainv, Linv;
    double logdet = 1.0;
    const std::vector<double> S = bidiagonal_sigma(33);
    CHECK(chol_inv(S.data(), 33, Ainv, logdet, &Linv) && same_bits(logdet, 0.0));
    int bad = 0;
    for (int i = 0; i < 33; ++i)
        for (int c = 0; c < 33; ++c) bad += !(Linv[(size_t)i * 33 + c] == (c <= i ? ((i - c) & 1 ? -1.0 : 1.0) : 0.0));
    CHECK(bad == 0);
}

void mvn_refusals() {
    const double x[4] = {1, 2, 3, 4}, eye[4] = {1, 0, 0, 1}, indefinite[4] = {1, 2, 2, 1}, semidefinite[4] = {1, 1, 1, 1};
    const int64_t d22[2] = {2, 2};
    PreparedModel m = prepare_model(DEMC_FAM_MVN_FULL, 2, DEMC_LOGLIKE_STREAMING, x, d22, 2, indefinite, 4);
    REFUSED(m.refused, DEMC_EINVAL, "Sigma is not positive definite");
    CHECK(empty_model(m));
    REFUSED(prepare_model(DEMC_FAM_MVN_FULL, 2, DEMC_LOGLIKE_DIRECT, x, d22, 2, semidefinite, 4).refused, DEMC_EINVAL, "Sigma is not positive definite");
    REFUSED(prepare_model(DEMC_FAM_MVN_FULL, 2, DEMC_LOGLIKE_STREAMING, x, d22, 2, eye, 3).refused, DEMC_EINVAL, "MVN_FULL: D=d, hyper=Sigma[d][d]");
    REFUSED(prepare_model(DEMC_FAM_MVN_FULL, 3, DEMC_LOGLIKE_STREAMING, x, d22, 2, eye, 4).refused, DEMC_EINVAL, "MVN_FULL: D=d, hyper=Sigma[d][d]");
    REFUSED(prepare_model(DEMC_FAM_MVN_ISO, 2, DEMC_LOGLIKE_STREAMING, x, d22, 2, nullptr, 0).refused, DEMC_EINVAL, "MVN_ISO: D=d+1");
    const int64_t d02[2] = {0, 2}, d20[2] = {2, 0};
    REFUSED(prepare_model(DEMC_FAM_MVN_FULL, 2, DEMC_LOGLIKE_STREAMING, x, d02, 2, eye, 4).refused, DEMC_EINVAL, "MVN: dims=[N,d]");
    REFUSED(prepare_model(DEMC_FAM_MVN_ISO, 1, DEMC_LOGLIKE_STREAMING, x, d20, 2, nullptr, 0).refused, DEMC_EINVAL, "MVN: dims=[N,d]");
    REFUSED(prepare_model(DEMC_FAM_MVN_ISO, 3, DEMC_LOGLIKE_STREAMING, x, d22, 1, nullptr, 0).refused, DEMC_EINVAL, "MVN: dims=[N,d]");  // ndims = 1: d = 0
    // d = 1025 is refused before D, hyper or the DIRECT limit are looked at, and before the data are read
    const int64_t d1025[2] = {1, 1025};
    for (int mode : {DEMC_LOGLIKE_STREAMING, DEMC_LOGLIKE_DIRECT}) {
        REFUSED(prepare_model(DEMC_FAM_MVN_FULL, 1025, mode, x, d1025, 2, eye, 4).refused, DEMC_EUNSUPPORTED, "MVN families: data dimension d <= 1024");
        REFUSED(prepare_model(DEMC_FAM_MVN_ISO, 7, mode, x, d1025, 2, nullptr, 0).refused, DEMC_EUNSUPPORTED, "MVN families: data dimension d <= 1024");
    }
    // DIRECT with d = 65 (the streaming modes take it: mvn_exact)
    std::vector<double> x65(65, 1.0);
    const std::vector<double> S65 = bidiagonal_sigma(65);
    const int64_t d65[2] = {1, 65};
    m = prepare_model(DEMC_FAM_MVN_FULL, 65, DEMC_LOGLIKE_DIRECT, x65.data(), d65, 2, S65.data(), 65 * 65);
    REFUSED(m.refused, DEMC_EUNSUPPORTED, "DIRECT likelihood: data dimension d <= 64 (the whitened proposal lives in registers)");
    CHECK(empty_model(m));
    REFUSED(prepare_model(DEMC_FAM_MVN_ISO, 66, DEMC_LOGLIKE_DIRECT, x65.data(), d65, 2, nullptr, 0).refused, DEMC_EUNSUPPORTED,
            "DIRECT likelihood: data dimension d <= 64 (the whitened proposal lives in registers)");
    const int64_t dhuge[2] = {(int64_t)1 << 34, 1};  // 2^30 tiles of 16: refused before a datum is read
    REFUSED(prepare_model(DEMC_FAM_MVN_ISO, 2, DEMC_LOGLIKE_STREAMING, x, dhuge, 2, nullptr, 0).refused, DEMC_EINVAL, "too many observations");
    REFUSED(prepare_model(77, 2, DEMC_LOGLIKE_STREAMING, x, d22, 2, nullptr, 0).refused, DEMC_EUNSUPPORTED,
            "model family is not registered; arbitrary closures cannot run on the device");
    REFUSED(prepare_model(DEMC_FAM_USER, 2, DEMC_LOGLIKE_STREAMING, x, d22, 2, nullptr, 0).refused, DEMC_EUNSUPPORTED,
            "model family is not registered; arbitrary closures cannot run on the device");
}

// ---- the per-observation families

double lgamma_expression(double n, double k) { return std::lgamma(n + 1.0) - std::lgamma(k + 1.0) - std::lgamma(n - k + 1.0); }

void gaussian_binomial_hierarchical() {
    const double x[3] = {0.5, -1.25, 3.0};
    const int64_t d3[1] = {3}, d0[1] = {0};
    PreparedModel m = prepare_model(DEMC_FAM_GAUSSIAN, 2, DEMC_LOGLIKE_STREAMING, x, d3, 1, nullptr, 0);
    CHECK(!m.refused && m.N == 3 && m.data == std::vector<double>(x, x + 3) && m.M.empty() && m.Xf.empty() && m.data2_off == 0);
    REFUSED(prepare_model(DEMC_FAM_GAUSSIAN, 3, DEMC_LOGLIKE_STREAMING, x, d3, 1, nullptr, 0).refused, DEMC_EINVAL, "GAUSSIAN: theta=(mu,sigma), dims=[N]");
    REFUSED(prepare_model(DEMC_FAM_GAUSSIAN, 2, DEMC_LOGLIKE_STREAMING, x, d0, 1, nullptr, 0).refused, DEMC_EINVAL, "GAUSSIAN: theta=(mu,sigma), dims=[N]");
    REFUSED(prepare_model(DEMC_FAM_GAUSSIAN, 2, DEMC_LOGLIKE_STREAMING, x, nullptr, 0, nullptr, 0).refused, DEMC_EINVAL, "GAUSSIAN: theta=(mu,sigma), dims=[N]");

    const double nk[8] = {10, 20, 7, 1, /* k */ 3, 20, 0, 1};
    const int64_t d4[1] = {4};
    m = prepare_model(DEMC_FAM_BINOMIAL, 1, DEMC_LOGLIKE_STREAMING, nk, d4, 1, nullptr, 0);
    CHECK(!m.refused && m.N == 4 && m.data2_off == 4 && m.data.size() == 12 && m.c2 == 0.0);
    for (int i = 0; i < 4 && m.data.size() == 12; ++i)
        CHECK(same_bits(m.data[i], nk[i]) && same_bits(m.data[4 + i], nk[4 + i]) && same_bits(m.data[8 + i], lgamma_expression(nk[i], nk[4 + i])));
    REFUSED(prepare_model(DEMC_FAM_BINOMIAL, 2, DEMC_LOGLIKE_STREAMING, nk, d4, 1, nullptr, 0).refused, DEMC_EINVAL, "BINOMIAL: theta=p, dims=[N], data=[n[N],k[N]]");
    REFUSED(prepare_model(DEMC_FAM_BINOMIAL, 1, DEMC_LOGLIKE_STREAMING, nk, d0, 1, nullptr, 0).refused, DEMC_EINVAL, "BINOMIAL: theta=p, dims=[N], data=[n[N],k[N]]");

    const double k5[5] = {3, 11, 0, 12, 7}, n_trials[1] = {12};
    const int64_t d5[1] = {5};
    m = prepare_model(DEMC_FAM_HIER_BINOMIAL, 7, DEMC_LOGLIKE_STREAMING, k5, d5, 1, n_trials, 1);
    CHECK(!m.refused && m.N == 5 && m.c0 == 12.0 && m.data.size() == 10 && m.data2_off == 0);
    double sum = 0.0;
    for (int s = 0; s < 5 && m.data.size() == 10; ++s) {
        CHECK(same_bits(m.data[s], k5[s]) && same_bits(m.data[5 + s], lgamma_expression(12.0, k5[s])));
        sum += lgamma_expression(12.0, k5[s]);  // in index order
    }
    CHECK(same_bits(m.c2, sum));
    REFUSED(prepare_model(DEMC_FAM_HIER_BINOMIAL, 6, DEMC_LOGLIKE_STREAMING, k5, d5, 1, n_trials, 1).refused, DEMC_EINVAL, "HIER_BINOMIAL: D=S+2, dims=[S], hyper=[n]");
    REFUSED(prepare_model(DEMC_FAM_HIER_BINOMIAL, 7, DEMC_LOGLIKE_STREAMING, k5, d5, 1, nullptr, 0).refused, DEMC_EINVAL, "HIER_BINOMIAL: D=S+2, dims=[S], hyper=[n]");

    const double y6[6] = {1, 2, 3, 4, 5, 6};
    const int64_t d23[2] = {2, 3}, d20[2] = {2, 0};
    m = prepare_model(DEMC_FAM_HIER_GAUSSIAN, 5, DEMC_LOGLIKE_STREAMING, y6, d23, 2, nullptr, 0);
    CHECK(!m.refused && m.N == 2 && m.d == 3 && m.data == std::vector<double>(y6, y6 + 6));
    REFUSED(prepare_model(DEMC_FAM_HIER_GAUSSIAN, 4, DEMC_LOGLIKE_STREAMING, y6, d23, 2, nullptr, 0).refused, DEMC_EINVAL, "HIER_GAUSSIAN: D=S+3, dims=[S,n]");
    REFUSED(prepare_model(DEMC_FAM_HIER_GAUSSIAN, 5, DEMC_LOGLIKE_STREAMING, y6, d20, 2, nullptr, 0).refused, DEMC_EINVAL, "HIER_GAUSSIAN: D=S+3, dims=[S,n]");

    m = prepare_model(DEMC_FAM_RASTRIGIN, 4, DEMC_LOGLIKE_STREAMING, nullptr, nullptr, 0, nullptr, 0);
    CHECK(!m.refused && m.N == 1 && m.data.empty());
}

void race_models() {
    // seven trials, choices and times tied; two of the tied times are +0 and -0, equal to the comparison and distinct in their bits,
    // so that the order a stable sort leaves them in can be seen
    const double data[14] = {2, 1, 2, 1, 2, 1, 1, /* rt */ 0.5, 0.0, 0.5, -0.0, 0.25, 0.75, 0.0};
    const int64_t d72[2] = {7, 2};
    PreparedModel m = prepare_model(DEMC_FAM_LBA, 5, DEMC_LOGLIKE_STREAMING, data, d72, 2, nullptr, 0);
    CHECK(!m.refused && m.N == 7 && m.n_acc == 2 && m.c0 == 0.0 && m.data2_off == 7 && m.data.size() == 14);
    // by insertion: trial t goes behind every trial that is not greater than it
    int order[7], n = 0;
    for (int t = 0; t < 7; ++t) {
        int at = n;
        while (at > 0 && (data[order[at - 1]] > data[t] || (data[order[at - 1]] == data[t] && data[7 + order[at - 1]] > data[7 + t]))) --at;
        for (int q = n; q > at; --q) order[q] = order[q - 1];
        order[at] = t;
        ++n;
    }
    const int by_hand[7] = {1, 3, 6, 5, 4, 0, 2};  // choice 1: +0 (trial 1), -0 (3), +0 (6), 0.75; choice 2: 0.25, 0.5 (0), 0.5 (2)
    std::vector<bool> used(7, false);
    for (int q = 0; q < 7 && m.data.size() == 14; ++q) {
        CHECK(order[q] == by_hand[q]);
        CHECK(same_bits(m.data[q], data[order[q]]) && same_bits(m.data[7 + q], data[7 + order[q]]));
        if (q) CHECK(m.data[q - 1] < m.data[q] || (m.data[q - 1] == m.data[q] && m.data[7 + q - 1] <= m.data[7 + q]));
        bool found = false;  // the multiset: every output pair uses up one input pair of the same bits
        for (int t = 0; t < 7 && !found; ++t)
            if (!used[t] && same_bits(m.data[q], data[t]) && same_bits(m.data[7 + q], data[7 + t])) used[t] = found = true;
        CHECK(found);
    }
    // LNR: the data as they came; c0 = hyper[0], 1 without
    const double sigma[1] = {0.7};
    m = prepare_model(DEMC_FAM_LNR, 3, DEMC_LOGLIKE_STREAMING, data, d72, 2, sigma, 1);
    CHECK(!m.refused && m.N == 7 && m.n_acc == 2 && m.c0 == 0.7 && m.data2_off == 7 && m.data.size() == 14);
    CHECK(m.data.size() == 14 && std::memcmp(m.data.data(), data, sizeof data) == 0);
    m = prepare_model(DEMC_FAM_LNR, 3, DEMC_LOGLIKE_STREAMING, data, d72, 2, nullptr, 0);
    CHECK(!m.refused && m.c0 == 1.0);
    // refusals
    const int64_t d70[2] = {7, 0}, d79[2] = {7, 9};
    for (int fam : {DEMC_FAM_LBA, DEMC_FAM_LNR}) {
        const int D = fam == DEMC_FAM_LBA ? 5 : 3;
        REFUSED(prepare_model(fam, D, DEMC_LOGLIKE_STREAMING, data, d70, 2, nullptr, 0).refused, DEMC_EINVAL, "LBA/LNR: dims=[N,n_acc<=8]");
        REFUSED(prepare_model(fam, 9 + (D - 2), DEMC_LOGLIKE_STREAMING, data, d79, 2, nullptr, 0).refused, DEMC_EINVAL, "LBA/LNR: dims=[N,n_acc<=8]");
        REFUSED(prepare_model(fam, D + 1, DEMC_LOGLIKE_STREAMING, data, d72, 2, nullptr, 0).refused, DEMC_EINVAL, "LBA/LNR: dims=[N,n_acc<=8]");
        double bad[14];
        for (double code : {0.0, 3.0, 1.5, kNaN}) {
            std::memcpy(bad, data, sizeof bad);
            bad[4] = code;
            REFUSED(prepare_model(fam, D, DEMC_LOGLIKE_STREAMING, bad, d72, 2, nullptr, 0).refused, DEMC_EINVAL, "LBA/LNR: choice of trial 4 is not an integer in [1, n_acc]");
        }
        for (double rt : {kInf, kNaN}) {
            std::memcpy(bad, data, sizeof bad);
            bad[7 + 2] = rt;
            bad[6] = 0.5;  // ... a later trial's bad choice does not win
            PreparedModel r = prepare_model(fam, D, DEMC_LOGLIKE_STREAMING, bad, d72, 2, nullptr, 0);
            REFUSED(r.refused, DEMC_EINVAL, "LBA/LNR: decision time of trial 2 is not finite");
            CHECK(empty_model(r));
        }
    }
}

void ode_lv() {
    const double y[6] = {1, 2, 1.5, 1.75, 2, 1.5}, hy[4] = {1.0, 0.5, 0.25, 8};
    const int64_t d32[2] = {3, 2};
    PreparedModel m = prepare_model(DEMC_FAM_ODE_LV, 5, DEMC_LOGLIKE_STREAMING, y, d32, 2, hy, 4);
    CHECK(!m.refused && m.N == 3 && m.ode_substeps == 8 && m.ode_h == 0.25 / 8 && m.data == std::vector<double>(y, y + 6));
    CHECK(m.ode_u0[0] == 1.0 && m.ode_u0[1] == 0.5 && m.ode_u0[2] == 0.0 && m.ode_u0[3] == 0.0);
    auto refusal = [&](int D, const double* data, const int64_t* dims, int ndims, const double* hyper, int nhyper) {
        return prepare_model(DEMC_FAM_ODE_LV, D, DEMC_LOGLIKE_STREAMING, data, dims, ndims, hyper, nhyper).refused;
    };
    REFUSED(refusal(4, y, d32, 2, hy, 4), DEMC_EINVAL, "ODE_LV: D = 5 required, theta=(alpha,beta,gamma,delta,sigma)");
    const int64_t d33[2] = {3, 3}, d02[2] = {0, 2}, d4097[2] = {4097, 2}, d4096[2] = {4096, 2};
    REFUSED(refusal(5, y, d32, 1, hy, 4), DEMC_EINVAL, "ODE_LV: dims[1] = 2 required, dims=[T,2] (the observed x and y per time)");
    REFUSED(refusal(5, y, d33, 2, hy, 4), DEMC_EINVAL, "ODE_LV: dims[1] = 2 required, dims=[T,2] (the observed x and y per time)");
    REFUSED(refusal(5, y, d02, 2, hy, 4), DEMC_EINVAL, "ODE_LV: T = dims[0] = 0 is outside [1, 4096]");
    REFUSED(refusal(5, y, d4097, 2, hy, 4), DEMC_EINVAL, "ODE_LV: T = dims[0] = 4097 is outside [1, 4096]");
    REFUSED(refusal(5, y, d32, 2, hy, 3), DEMC_EINVAL, "ODE_LV: hyper=[x0, y0, dt, substeps] (nhyper = 4)");
    REFUSED(refusal(5, y, d32, 2, nullptr, 4), DEMC_EINVAL, "ODE_LV: hyper=[x0, y0, dt, substeps] (nhyper = 4)");
    for (double sub : {0.0, 1025.0, 2.5, kNaN}) {
        const double h2[4] = {1.0, 0.5, 0.25, sub};
        REFUSED(refusal(5, y, d32, 2, h2, 4), DEMC_EINVAL, "ODE_LV: substeps (hyper[3]) must be an integer in [1, 1024]");
    }
    for (double dt : {0.0, -1.0, kInf, kNaN}) {
        const double h2[4] = {1.0, 0.5, dt, 8};
        REFUSED(refusal(5, y, d32, 2, h2, 4), DEMC_EINVAL, "ODE_LV: dt (hyper[2]) must be finite and positive");
    }
    const double hx[4] = {kInf, 0.5, 0.25, 8}, hyy[4] = {1.0, kNaN, 0.25, 8};
    REFUSED(refusal(5, y, d32, 2, hx, 4), DEMC_EINVAL, "ODE_LV: u0 = (x0, y0) (hyper[0], hyper[1]) must be finite");
    REFUSED(refusal(5, y, d32, 2, hyy, 4), DEMC_EINVAL, "ODE_LV: u0 = (x0, y0) (hyper[0], hyper[1]) must be finite");
    REFUSED(refusal(5, nullptr, d32, 2, hy, 4), DEMC_EINVAL, "ODE_LV: data = Y[T][2] required");
    double ybad[6];
    std::memcpy(ybad, y, sizeof ybad);
    ybad[3] = kNaN;
    REFUSED(refusal(5, ybad, d32, 2, hy, 4), DEMC_EINVAL, "ODE_LV: data value 3 (time 1) is not finite");
    std::vector<double> ylong(2 * 4096, 1.0);  // the cap itself is taken
    CHECK(!refusal(5, ylong.data(), d4096, 2, hy, 4));
}

// ---- demc_set_model_sim

void sim() {
    const double obs[6] = {1, 2, 2, 0.4, 0.5, 0.6}, hy2[2] = {0.0, 1.0}, hyb[2] = {0.3, 20};
    auto refusal = [&](int D, int simulator, int est, int64_t n_sim, const char* src, const double* data, int64_t n_obs, const double* hyper, int nhyper) {
        return prepare_sim(D, simulator, est, n_sim, src, data, n_obs, hyper, nhyper).refused;
    };
    const int KDE = DEMC_SIMEST_KDE_EPANECHNIKOV, FREQ = DEMC_SIMEST_FREQUENCY, CHOICE = DEMC_SIMEST_KDE_CHOICE;
    REFUSED(refusal(2, 3, KDE, 100, nullptr, obs, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: unknown simulator");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, 3, 100, nullptr, obs, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: unknown estimator");
    REFUSED(refusal(3, DEMC_SIM_LNR, FREQ, 100, nullptr, obs, 3, hy2, 2), DEMC_EINVAL,
            "demc_set_model_sim: DEMC_SIM_LNR simulates (choice, time) pairs and cannot be scored by the scalar estimator DEMC_SIMEST_FREQUENCY (use DEMC_SIMEST_KDE_CHOICE)");
    REFUSED(refusal(3, DEMC_SIM_LNR, KDE, 100, nullptr, obs, 3, hy2, 2), DEMC_EINVAL,
            "demc_set_model_sim: DEMC_SIM_LNR simulates (choice, time) pairs and cannot be scored by the scalar estimator DEMC_SIMEST_KDE_EPANECHNIKOV (use DEMC_SIMEST_KDE_CHOICE)");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, CHOICE, 100, nullptr, obs, 3, nullptr, 0), DEMC_EINVAL,
            "demc_set_model_sim: DEMC_SIM_NORMAL simulates scalars and cannot be scored by DEMC_SIMEST_KDE_CHOICE (use DEMC_SIM_LNR or a user simulator of pairs)");
    REFUSED(refusal(1, DEMC_SIM_BINOMIAL, CHOICE, 100, nullptr, obs, 3, hyb, 2), DEMC_EINVAL,
            "demc_set_model_sim: DEMC_SIM_BINOMIAL simulates scalars and cannot be scored by DEMC_SIMEST_KDE_CHOICE (use DEMC_SIM_LNR or a user simulator of pairs)");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 1, nullptr, obs, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: n_sim < 2 (a density estimate needs at least two simulated values)");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 16385, nullptr, obs, 3, nullptr, 0), DEMC_EINVAL,
            "demc_set_model_sim: n_sim = 16385 is above the cap of 16384 simulated values (the sample of a proposal is held in LDS)");
    REFUSED(refusal(3, DEMC_SIM_LNR, CHOICE, 15001, nullptr, obs, 3, hy2, 2), DEMC_EINVAL,
            "demc_set_model_sim: n_sim = 15001 is above the cap of 15000 simulated values (the sample of a proposal is held in LDS)");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 100, nullptr, obs, 0, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: n_obs >= 1 observations required");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 100, nullptr, nullptr, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: n_obs >= 1 observations required");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 100, nullptr, obs, 3, nullptr, 1), DEMC_EINVAL, "demc_set_model_sim: nhyper > 0 without hyper");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 100, nullptr, obs, 3, hy2, -1), DEMC_EINVAL, "demc_set_model_sim: nhyper > 0 without hyper");
    for (const char* src : {(const char*)nullptr, ""})
        REFUSED(refusal(2, DEMC_SIM_USER, KDE, 100, src, obs, 3, nullptr, 0), DEMC_EINVAL,
                "demc_set_model_sim: DEMC_SIM_USER needs hip_source (a definition of demc_user_sim; demc_user_sim_choice under DEMC_SIMEST_KDE_CHOICE)");
    REFUSED(refusal(2, DEMC_SIM_NORMAL, KDE, 100, "x", obs, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: hip_source given with a registered simulator");
    REFUSED(refusal(3, DEMC_SIM_NORMAL, KDE, 100, nullptr, obs, 3, nullptr, 0), DEMC_EINVAL, "SIM_NORMAL: theta=(mu,sigma)");
    REFUSED(refusal(2, DEMC_SIM_BINOMIAL, KDE, 100, nullptr, obs, 3, hyb, 2), DEMC_EINVAL, "SIM_BINOMIAL: theta=p");
    REFUSED(refusal(1, DEMC_SIM_BINOMIAL, KDE, 100, nullptr, obs, 3, hyb, 1), DEMC_EINVAL, "SIM_BINOMIAL: hyper=[bandwidth, n_trials], n_trials an integer in [1, 1024]");
    for (double trials : {0.0, 1025.0, 2.5, kNaN}) {
        const double h2[2] = {0.3, trials};
        REFUSED(refusal(1, DEMC_SIM_BINOMIAL, FREQ, 100, nullptr, obs, 3, h2, 2), DEMC_EINVAL, "SIM_BINOMIAL: hyper=[bandwidth, n_trials], n_trials an integer in [1, 1024]");
    }
    // ("SIM_BINOMIAL: too many Philox blocks per proposal" cannot be reached: 16 384 values of at most 1024 trials are 2^22 blocks)
    for (int D : {2, 10}) REFUSED(refusal(D, DEMC_SIM_LNR, CHOICE, 100, nullptr, obs, 3, hy2, 2), DEMC_EINVAL, "SIM_LNR: theta=(nu[K],tau), K = D - 1 in [2, 8]");
    const double hneg[2] = {0.0, 0.0};
    REFUSED(refusal(3, DEMC_SIM_LNR, CHOICE, 100, nullptr, obs, 3, hneg, 2), DEMC_EINVAL, "SIM_LNR: hyper=[bandwidth, sigma], sigma > 0");
    REFUSED(refusal(3, DEMC_SIM_LNR, CHOICE, 100, nullptr, obs, 3, hy2, 1), DEMC_EINVAL, "SIM_LNR: hyper=[bandwidth, sigma], sigma > 0");
    double bad[6];
    std::memcpy(bad, obs, sizeof bad);
    bad[1] = 3;  // D = 3: two accumulators
    REFUSED(refusal(3, DEMC_SIM_LNR, CHOICE, 100, nullptr, bad, 3, hy2, 2), DEMC_EINVAL, "demc_set_model_sim: the choice of observation 1 is not an integer in [1, 2]");
    bad[1] = 256;
    REFUSED(refusal(4, DEMC_SIM_USER, CHOICE, 100, "x", bad, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: the choice of observation 1 is not an integer in [1, 255]");
    bad[1] = 1.5;
    REFUSED(refusal(4, DEMC_SIM_USER, CHOICE, 100, "x", bad, 3, nullptr, 0), DEMC_EINVAL, "demc_set_model_sim: the choice of observation 1 is not an integer in [1, 255]");
    std::memcpy(bad, obs, sizeof bad);
    bad[3 + 2] = kInf;
    REFUSED(refusal(3, DEMC_SIM_LNR, CHOICE, 100, nullptr, bad, 3, hy2, 2), DEMC_EINVAL, "demc_set_model_sim: the response time of observation 2 is not finite");
    const double frac[3] = {1, 2, 2.5};
    REFUSED(refusal(1, DEMC_SIM_BINOMIAL, FREQ, 100, nullptr, frac, 3, hyb, 2), DEMC_EINVAL,
            "demc_set_model_sim: the FREQUENCY estimator needs integer-valued data (observation 2 is not)");

    // what an accepted call yields
    PreparedSim s = prepare_sim(2, DEMC_SIM_NORMAL, KDE, 100, nullptr, obs, 3, nullptr, 0);  // no hyper: the bandwidth slot alone, 0
    CHECK(!s.refused && s.kmax == 0 && s.hyper == std::vector<double>(1, 0.0) && s.sim_bw == 0.0 && s.logtab.empty());
    const double user_obs[6] = {7, 200, 3, 0.4, 0.5, 0.6}, hy3[3] = {0.125, 4, 5}, hyneg[2] = {-1.0, 2.0};
    s = prepare_sim(4, DEMC_SIM_USER, CHOICE, 15000, "x", user_obs, 3, hy3, 3);
    CHECK(!s.refused && s.kmax == 200 && s.hyper == std::vector<double>(hy3, hy3 + 3) && s.sim_bw == 0.125 && s.logtab.empty());
    s = prepare_sim(3, DEMC_SIM_LNR, CHOICE, 100, nullptr, obs, 3, hyneg, 2);
    CHECK(!s.refused && s.kmax == 2 && s.hyper == std::vector<double>(hyneg, hyneg + 2) && s.sim_bw == 0.0);
    const double counts[3] = {4, 0, 20};
    const int n = 50;
    s = prepare_sim(1, DEMC_SIM_BINOMIAL, FREQ, n, nullptr, counts, 3, hyb, 2);
    CHECK(!s.refused && s.kmax == 0 && s.sim_bw == 0.3 && s.logtab.size() == (size_t)n + 1);
    if (s.logtab.size() == (size_t)n + 1) {
        CHECK(s.logtab[0] == -kInf && same_bits(s.logtab[n], 0.0));
        for (int c = 1; c < n; ++c) CHECK(same_bits(s.logtab[c], std::log((double)c / (double)n)) && s.logtab[c] < 0.0 && s.logtab[c] > s.logtab[c - 1]);
    }
}

// ---- the prior table

double restated_const(int kind, double a, double b) {  // the x-independent part of each log-density, as DESIGN.md defines it
    const double pi = 3.14159265358979323846264338327950288;
    switch (kind) {
        case DEMC_PRIOR_NORMAL: case DEMC_PRIOR_TRUNCNORMAL: return -0.5 * kLog2PiHere - std::log(b);
        case DEMC_PRIOR_HALFCAUCHY: return -kLogPiHere - std::log(b) - std::log(1.0 - (std::atan((0.0 - a) / b) / pi + 0.5));
        case DEMC_PRIOR_UNIFORM: return -std::log(b - a);
        case DEMC_PRIOR_BETA: return -(std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b));
        case DEMC_PRIOR_GAMMA: return -a * std::log(b) - std::lgamma(a);
        case DEMC_PRIOR_EXPONENTIAL: return -std::log(b);
        case DEMC_PRIOR_LOGNORMAL: return -std::log(b) - 0.5 * kLog2PiHere;
        case DEMC_PRIOR_CAUCHY: return -kLogPiHere - std::log(b);
        default: return 0.0;
    }
}

// log of the Normal(a, b) mass on [lo, hi] in long double, from the arguments the library forms in double (their rounding is
// not what is judged: an erfc amplifies it by about 2 x^2)
long double reference_log_mass(double a, double b, double lo, double hi) {
    const double zl = (lo - a) / b, zh = (hi - a) / b, r = std::sqrt(0.5);
    return zl > 0.0 ? logl(0.5L * (erfcl((long double)(zl * r)) - erfcl((long double)(zh * r))))
                    : logl(0.5L * (erfcl((long double)(-zh * r)) - erfcl((long double)(-zl * r))));
}

DimTab flat_entry(double lo, double hi) {
    DimTab t;
    std::memset(&t, 0, sizeof t);
    t.lo = lo; t.hi = hi; t.a = 0.0; t.b = 1.0; t.c = 0.0; t.kind = PR_FLAT; t.ref = 0;
    return t;
}
bool same_entry(const DimTab& x, const DimTab& y) { return std::memcmp(&x, &y, sizeof x) == 0; }

void prior_entries() {
    CHECK(DEMC_PRIOR_TRUNCNORMAL == 10);  // the kinds below are all there are
    const bool reciprocal[11] = {false, true, true, false, false, false, true, true, true, true, true};
    const int device_kind[11] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, /* truncated Normal: the Normal entry */ 1};
    const double a = 0.75, b = 2.5;  // (Uniform(a, b): a < b)
    const int D = 11;
    std::vector<DimTab> tab((size_t)D, flat_entry(-3.0, 4.0));
    std::vector<double> sd(3, 9.0);
    int32_t kind[11], ref[11];
    double av[11], bv[11];
    for (int j = 0; j < D; ++j) { kind[j] = j; ref[j] = 10 - j; av[j] = a; bv[j] = b; }
    CHECK(!prepare_priors(tab, sd, kind, av, bv, ref));
    for (int j = 0; j < D; ++j) {
        const DimTab& t = tab[(size_t)j];
        CHECK(t.kind == device_kind[j] && t.ref == 10 - j && t.lo == -3.0 && t.hi == 4.0 && same_bits(t.a, a));
        CHECK(same_bits(t.b, reciprocal[j] ? 1.0 / b : b));
        if (j != DEMC_PRIOR_TRUNCNORMAL) CHECK(same_bits(t.c, restated_const(j, a, b)));
        CHECK(sd.size() == (size_t)D && sd[(size_t)j] == (j == DEMC_PRIOR_TRUNCNORMAL ? b : 0.0));
    }
    {   // the truncated Normal's constant: the Normal's, less the log of the mass.  Allowed: 8 * 2^-53 on the mass (log_mass below),
        // a rounding each of the two logarithms and the two subtractions on values below 2 in size: under 16 * 2^-53 together
        const long double want = (long double)restated_const(DEMC_PRIOR_NORMAL, a, b) - reference_log_mass(a, b, -3.0, 4.0);
        CHECK(fabsl((long double)tab[10].c - want) <= 16.0L * 0x1p-53L);
    }
    // null a, b, ref: 0, 1, 0
    std::vector<DimTab> tab1(1, flat_entry(-kInf, kInf));
    const int32_t normal[1] = {DEMC_PRIOR_NORMAL};
    CHECK(!prepare_priors(tab1, sd, normal, nullptr, nullptr, nullptr));
    CHECK(tab1[0].a == 0.0 && tab1[0].b == 1.0 && tab1[0].ref == 0 && same_bits(tab1[0].c, -0.5 * kLog2PiHere) && sd == std::vector<double>(1, 0.0));

    // priors then bounds, bounds then priors: the same entry, and the one formed directly
    const int32_t k3[3] = {DEMC_PRIOR_NORMAL, DEMC_PRIOR_TRUNCNORMAL, DEMC_PRIOR_TRUNCNORMAL}, r3[3] = {0, 0, 0};
    const double a3[3] = {0.0, 0.5, -1.0}, b3[3] = {1.0, 2.0, 0.5}, lo3[3] = {-1.0, -0.2, -1.25}, hi3[3] = {1.0, 3.0, kInf};
    std::vector<DimTab> pb(3, flat_entry(-kInf, kInf)), bp = pb;
    std::vector<double> sd_pb, sd_bp;
    CHECK(!prepare_priors(pb, sd_pb, k3, a3, b3, r3) && !prepare_bounds(pb, sd_pb, lo3, hi3));
    CHECK(!prepare_bounds(bp, sd_bp, lo3, hi3) && !prepare_priors(bp, sd_bp, k3, a3, b3, r3));
    for (int j = 0; j < 3; ++j) {
        DimTab direct_entry;
        CHECK(!prior_entry((size_t)j, k3[j], a3[j], b3[j], r3[j], lo3[j], hi3[j], &direct_entry));
        CHECK(same_entry(pb[(size_t)j], bp[(size_t)j]) && same_entry(pb[(size_t)j], direct_entry));
        CHECK(pb[(size_t)j].kind == PR_NORMAL && pb[(size_t)j].lo == lo3[j] && pb[(size_t)j].hi == hi3[j] && same_bits(pb[(size_t)j].b, 1.0 / b3[j]));
        const long double want = (long double)restated_const(DEMC_PRIOR_NORMAL, a3[j], b3[j]) - (j ? reference_log_mass(a3[j], b3[j], lo3[j], hi3[j]) : 0.0L);
        CHECK(fabsl((long double)pb[(size_t)j].c - want) <= 16.0L * 0x1p-53L);
    }
    CHECK(sd_pb == sd_bp && sd_pb == std::vector<double>({0.0, 2.0, 0.5}));
    // new bounds move a truncated Normal's constant and nothing else of the entry
    const double lo4[3] = {-2.0, 0.0, -2.0}, hi4[3] = {2.0, 1.0, 0.0};
    std::vector<DimTab> moved = pb;
    CHECK(!prepare_bounds(moved, sd_pb, lo4, hi4));
    CHECK(same_bits(moved[0].c, pb[0].c) && moved[1].c > pb[1].c && moved[1].kind == PR_NORMAL && same_bits(moved[1].b, pb[1].b) && moved[1].lo == 0.0 && moved[1].hi == 1.0);

    // refusals leave the table and the scales as they were
    const std::vector<DimTab> before = pb;
    const std::vector<double> sd_before = sd_pb;
    auto untouched = [&] {
        bool same = pb.size() == before.size() && sd_pb == sd_before;
        for (size_t j = 0; same && j < pb.size(); ++j) same = same_entry(pb[j], before[j]);
        return same;
    };
    const double lo_empty[3] = {-1.0, 2.0, -1.25}, hi_empty[3] = {1.0, 2.0, kInf};
    REFUSED(prepare_bounds(pb, sd_pb, lo_empty, hi_empty), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 1: the bounds lo >= hi leave nothing to truncate to");
    CHECK(untouched());
    const double lo_far[3] = {-1.0, -0.2, 40.0}, hi_far[3] = {1.0, 3.0, 50.0};  // 82 standard deviations out
    REFUSED(prepare_bounds(pb, sd_pb, lo_far, hi_far), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 2: the mass of the Normal between the bounds is 0 or not finite");
    CHECK(untouched());
    const int32_t k_bad[3] = {DEMC_PRIOR_TRUNCNORMAL, DEMC_PRIOR_NORMAL, 11}, k_neg[3] = {-1, 0, 0};
    const double b_bad[3] = {0.0, 1.0, 1.0};  // scalar 0's scale is refused too: the unknown kind behind it wins
    REFUSED(prepare_priors(pb, sd_pb, k_bad, a3, b_bad, r3), DEMC_EUNSUPPORTED, "prior kind not registered");
    REFUSED(prepare_priors(pb, sd_pb, k_neg, a3, b3, r3), DEMC_EUNSUPPORTED, "prior kind not registered");
    CHECK(untouched());
    const int32_t k_ref[3] = {DEMC_PRIOR_TRUNCNORMAL, DEMC_PRIOR_NORMAL_REF, 0}, r_hi[3] = {0, 3, 0}, r_lo[3] = {0, -1, 0};
    REFUSED(prepare_priors(pb, sd_pb, k_ref, a3, b_bad, r_hi), DEMC_EINVAL, "prior ref out of range");
    REFUSED(prepare_priors(pb, sd_pb, k_ref, a3, b3, r_lo), DEMC_EINVAL, "prior ref out of range");
    REFUSED(prepare_priors(pb, sd_pb, k_ref, a3, b3, nullptr), DEMC_EINVAL, "prior ref out of range");
    const int32_t k_t0[3] = {DEMC_PRIOR_NORMAL, DEMC_PRIOR_NORMAL, DEMC_PRIOR_TRUNCNORMAL};
    REFUSED(prepare_priors(pb, sd_pb, k_t0, a3, b_bad, r3), DEMC_OK, "");  // (a Normal's scale is not judged)
    pb = before; sd_pb = sd_before;
    const double b_neg[3] = {1.0, 1.0, -2.0};
    REFUSED(prepare_priors(pb, sd_pb, k_t0, a3, b_neg, r3), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 2: Normal(a, b) needs a finite a and a finite b > 0");
    CHECK(untouched());
}

void log_mass() {
    // the two erfc values of every case differ by a factor of two at least, so their difference amplifies their errors at most
    // threefold; allowed on the mass: 8 * 2^-53 (two erfc of under 1 ulp each, amplified, one rounding each for the subtraction and
    // the scale).  What comes back is the LOG of the mass, rounded once more; the bound is held with that rounding inside it.
    struct Case { double a, b, lo, hi; };
    const Case cases[] = {{0, 1, 0.5, 2},  {0, 1, 1, 1.8},   {0, 1, 3, 4},      {0, 1, 2, kInf},   {1.5, 0.5, 2, 2.75},  // zl > 0: the upper tails
                          {0, 1, -2, -0.5}, {0, 1, -1, 1},   {0, 1, -kInf, 0.3}, {0.5, 2, -0.2, 3}, {-1, 0.5, -1.25, kInf}};
    long double worst = 0.0L;
    int upper = 0, lower = 0;
    for (const Case& c : cases) {
        const double zl = (c.lo - c.a) / c.b, zh = (c.hi - c.a) / c.b, r = std::sqrt(0.5);
        const double e0 = zl > 0.0 ? std::erfc(zl * r) : std::erfc(-zh * r), e1 = zl > 0.0 ? std::erfc(zh * r) : std::erfc(-zl * r);
        CHECK(e0 >= 2.0 * e1);
        (zl > 0.0 ? upper : lower)++;
        double out = kNaN;
        CHECK(!truncnormal_log_mass(3, c.a, c.b, c.lo, c.hi, &out));
        const long double rel = fabsl(expm1l((long double)out - reference_log_mass(c.a, c.b, c.lo, c.hi)));
        std::printf("truncnormal_log_mass a=%g b=%g [%g, %g]: log mass %.17g, relative error of the mass %.3Lg * 2^-53\n", c.a, c.b, c.lo, c.hi, out, rel * 0x1p53L);
        worst = std::max(worst, rel);
        CHECK(rel <= 8.0L * 0x1p-53L);
    }
    CHECK(upper >= 4 && lower >= 4);
    std::printf("truncnormal_log_mass: largest relative error of the mass: %.3Lg * 2^-53 (allowed: 8)\n", worst * 0x1p53L);
    double out = 123.0;
    for (double a : {kInf, -kInf, kNaN})
        REFUSED(truncnormal_log_mass(4, a, 1.0, -1.0, 1.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 4: Normal(a, b) needs a finite a and a finite b > 0");
    for (double b : {0.0, -1.0, kInf, kNaN})
        REFUSED(truncnormal_log_mass(4, 0.0, b, -1.0, 1.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 4: Normal(a, b) needs a finite a and a finite b > 0");
    REFUSED(truncnormal_log_mass(0, 0.0, 1.0, 1.0, 1.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 0: the bounds lo >= hi leave nothing to truncate to");
    REFUSED(truncnormal_log_mass(0, 0.0, 1.0, 2.0, 1.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 0: the bounds lo >= hi leave nothing to truncate to");
    REFUSED(truncnormal_log_mass(0, 0.0, 1.0, kNaN, 1.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 0: the bounds lo >= hi leave nothing to truncate to");
    REFUSED(truncnormal_log_mass(12, 0.0, 1.0, 40.0, 41.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 12: the mass of the Normal between the bounds is 0 or not finite");
    REFUSED(truncnormal_log_mass(12, 0.0, 1.0, -41.0, -40.0, &out), DEMC_EINVAL, "DEMC_PRIOR_TRUNCNORMAL, scalar 12: the mass of the Normal between the bounds is 0 or not finite");
    CHECK(out == 123.0);  // a refusal writes nothing
}

void segments() {
    // runs of 1 .. 3 scalars; run q differs from its neighbours in `a`, its kind goes round all ten
    for (int runs : {1, 3, 16, 17}) {
        std::vector<DimTab> tab;
        std::vector<int> start, kinds;
        for (int q = 0; q < runs; ++q) {
            DimTab t = flat_entry(-1.0, 1.0);
            t.a = (double)q;
            t.kind = (3 * q) % 10;
            start.push_back((int)tab.size());
            kinds.push_back(t.kind);
            tab.insert(tab.end(), (size_t)(1 + q % 3), t);
        }
        const SegTable s = encode_segments(tab);
        const int n = runs <= 16 ? runs : 0;
        CHECK(s.n_seg == n);
        unsigned plain = 0;
        for (int q = 0; q < n; ++q)
            if (kinds[q] == 0 || kinds[q] == 1 || kinds[q] == 5) plain |= 1u << q;  // Flat, Normal, Normal(a, theta[ref])
        CHECK(s.seg_plain == plain && (runs != 16 || plain == 0x84a1u));  // (q = 0, 5, 7, 10, 15 by hand)
        for (int q = 0; q < kMaxDimSeg; ++q) {
            CHECK(s.seg_start[q] == (q < n ? start[q] : 0));
            if (q < n) CHECK(s.segs[q].start == start[q] && s.segs[q].pad == 0 && s.segs[q].pad2 == 0.0 && same_entry(s.segs[q].t, tab[(size_t)start[q]]));
        }
        if (runs == 3) {  // nothing behind the last segment
            const DimSeg zero[kMaxDimSeg - 3] = {};
            CHECK(std::memcmp(s.segs + 3, zero, sizeof zero) == 0);
        }
    }
    // equal values in other bits are other entries: -0.0 against 0.0 in a bound starts a segment
    std::vector<DimTab> tab(4, flat_entry(0.0, 1.0));
    tab[2].lo = tab[3].lo = -0.0;
    const SegTable s = encode_segments(tab);
    CHECK(s.n_seg == 2 && s.seg_start[1] == 2 && s.seg_plain == 3u);
    CHECK(encode_segments(std::vector<DimTab>()).n_seg == 0);
}

void masks() {
    for (int runs : {1, 2, 16, 17})
        for (int first_in : {0, 1}) {
            std::vector<uint8_t> mk;
            std::vector<int> start;
            unsigned in = 0;
            for (int q = 0; q < runs; ++q) {
                const bool inside = (q & 1) != first_in;
                start.push_back((int)mk.size());
                if (inside) in |= 1u << q;
                mk.insert(mk.end(), (size_t)(1 + (q * 5) % 4), inside ? (uint8_t)(1 + q) : (uint8_t)0);  // any non-zero byte is "inside"
            }
            const MaskRuns mr = encode_mask(mk.data(), (int)mk.size());
            const bool fits = runs <= kMaxMaskRun;
            CHECK(mr.n == (fits ? runs : 0) && mr.in == (fits ? in : 0u));
            for (int q = 0; q < kMaxMaskRun; ++q) CHECK(mr.start[q] == (fits && q < runs ? start[q] : 0));
        }
    CHECK(encode_mask(nullptr, 0).n == 0);
}

}  // namespace

int main() {
    static_assert(sizeof(DimTab) == 48 && sizeof(DimSeg) == 64 && kMaxDimSeg == 16 && kMaxMaskRun == 16, "the layouts the kernels read");
    CHECK(pow2_ceil(0) == 1 && pow2_ceil(1) == 1 && pow2_ceil(3) == 4 && pow2_ceil(16) == 16 && pow2_ceil(17) == 32);
    mvn_exact();
    mvn_refusals();
    gaussian_binomial_hierarchical();
    race_models();
    ode_lv();
    sim();
    prior_entries();
    log_mass();
    segments();
    masks();
    if (failures) std::fprintf(stderr, "%d of %d check(s) failed\n", failures, checks);
    else std::printf("prep ok: %d checks\n", checks);
    return failures ? 1 : 0;
}
