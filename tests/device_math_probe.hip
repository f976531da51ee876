// device_math_probe.hip -- the FP64 helpers of csrc/demc_device.hpp and csrc/demc_kernels.hpp as DEVICE code on chosen arguments
// (tests/test_gpu_device_math.py builds it with the FLAGS line of csrc/Makefile, less -shared -fPIC, and runs it once).
//
//   device_math_probe <request file> <result file>
//
// request:  u64 magic, u64 n_cases, then per case  i64 fn, i64 n, i64 n_ycols, f64 x[n], f64 y[n_ycols][n]
// result:   u64 magic, u64 n_cases, then per case  i64 fn, i64 n, f64 out[2][n]
// One launch per case; every lane i < n evaluates helper `fn` on x[i] (further per-lane arguments in the columns of y) and stores
// up to two results.  Every HIP call is checked; any error ends the program with a non-zero status before anything else is launched.
#define DEMC_DEVICE_HELPERS_ONLY
#define DEMC_K1_EXTERN
#include "demc_kernels.hpp"
#include "demc_prep.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace demc;

enum Fn : int {
    FN_EXP_NONPOS = 0, FN_SOFTPLUS_FAST = 1, FN_SOFTPLUS_TAB = 2, FN_RECIP_POS = 3, FN_PHI_TABLE = 4, FN_LOG_PHI_NEG = 5,
    FN_LBA2 = 6, FN_LBA3 = 7, FN_LBA_RT4 = 8, FN_PRIOR_TERM = 9, FN_BOX_MULLER = 10, FN_COUNT = 11
};
// columns of y a helper reads (x is the first argument)
//   lba_trial:  choice, nu[0..3], A, k, tau      (x = rt; the per-proposal values are formed as lba_range_sum forms them)
//   prior_term: kind, a, b                       (x = the scalar; a, b as the caller of demc_set_priors gives them: main() turns each
//                                                 row into the DimTab entry the kernels read -- b or 1/b, and c -- by demc_prep.hpp's
//                                                 prior_entry, and uploads kind, a, b, c)
//   box_muller: w1                               (x = w0; the 32-bit words as doubles)
static const int kYCols[FN_COUNT] = {0, 0, 0, 0, 0, 0, 8, 8, 8, 3, 1};

constexpr int kTabPhi = kPhiIntervals * kPhiRow, kTabLogPhi = kLogPhiRows * kLogPhiRow;
constexpr int kTabMax = kTabPhi > kTabLogPhi ? (kTabPhi > kSpDoubles ? kTabPhi : kSpDoubles) : (kTabLogPhi > kSpDoubles ? kTabLogPhi : kSpDoubles);

template <int NA>
__device__ double probe_lba(const double* tab, int na_rt, double rt, const double* y, long long n, long long i) {
    const int na = NA > 0 ? NA : na_rt;
    double nu[8], nuS[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        nu[a] = a < na ? y[(1 + a) * n + i] : 0.0;
        nuS[a] = kPhiS * nu[a];
    }
    const double A = y[5 * n + i], kk = y[6 * n + i], tau = y[7 * n + i], b = A + kk, inv_A = 1.0 / A;
    const double kS = kPhiS * kk, bS = kPhiS * b, inv_SA = inv_A * (1.0 / kPhiS);
    double pneg = 1.0;
#pragma unroll
    for (int a = 0; a < (NA > 0 ? NA : 8); ++a)
        if (a < na) {
            double q, Ph;
            phiS_Phi_table(tab, -nuS[a], q, Ph);
            pneg *= Ph;
        }
    const double inv_norm = 1.0 / (1.0 - pneg);
    return lba_trial<NA>(tab, na, nu, nuS, kS, bS, tau, inv_A, inv_SA, inv_norm, (int)y[i], rt);
}

__global__ __launch_bounds__(256) void k_probe(int fn, const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ out,
                                               long long n, const double* __restrict__ params) {
    // the tables in LDS, as the shipping kernels hold them (k_obs_loglike, k_lba_wave, k_frozen_sweep)
    __shared__ double s_tab[kTabMax];
    if (fn == FN_PHI_TABLE || fn == FN_LBA2 || fn == FN_LBA3 || fn == FN_LBA_RT4) {
        for (int i = threadIdx.x; i < kTabPhi; i += 256) s_tab[i] = kPhiTable[i];
    } else if (fn == FN_LOG_PHI_NEG) {
        for (int i = threadIdx.x; i < kTabLogPhi; i += 256) s_tab[i] = kLogPhiTable[i];
    } else if (fn == FN_SOFTPLUS_TAB) {
        load_softplus_table(s_tab, threadIdx.x, 256);
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double xi = x[i];
    double r0 = 0.0, r1 = 0.0;
    switch (fn) {
        case FN_EXP_NONPOS: r0 = exp_nonpos(xi); break;
        case FN_SOFTPLUS_FAST: r0 = softplus_fast(xi); break;
        case FN_SOFTPLUS_TAB: {
            const SoftplusTab c = softplus_tab_consts(s_tab);
            r0 = softplus_tab(xi, c);
        } break;
        case FN_RECIP_POS: r0 = recip_pos(xi); break;
        case FN_PHI_TABLE: phiS_Phi_table(s_tab, xi, r0, r1); break;  // (phi / S, Phi)
        case FN_LOG_PHI_NEG: r0 = log_Phi_neg_table(s_tab, xi); break;
        case FN_LBA2: r0 = probe_lba<2>(s_tab, 2, xi, y, n, i); break;
        case FN_LBA3: r0 = probe_lba<3>(s_tab, 3, xi, y, n, i); break;
        case FN_LBA_RT4: r0 = probe_lba<0>(s_tab, (int)params[0], xi, y, n, i); break;
        case FN_PRIOR_TERM: {
            DimTab t;
            t.lo = 0.0; t.hi = 0.0; t.ref = 0;
            t.kind = (int)y[i]; t.a = y[n + i]; t.b = y[2 * n + i]; t.c = y[3 * n + i];
            r0 = prior_term(t, xi, 0.0, 0.0);
        } break;
        case FN_BOX_MULLER: {
            const double2 z = box_muller((uint32_t)xi, (uint32_t)y[i]);
            r0 = z.x; r1 = z.y;
        } break;
        default: break;
    }
    out[i] = r0;
    out[n + i] = r1;
}

#define CHECK(call)                                                                                      \
    do {                                                                                                 \
        const hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                          \
            std::fprintf(stderr, "probe: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 3;                                                                                    \
        }                                                                                                \
    } while (0)

static const unsigned long long kMagic = 0x314d564544434d44ull;  // "DMCDEVM1"
static const long long kMaxN = 1ll << 22;

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <request> <result>\n", argv[0]);
        return 2;
    }
    std::FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) { std::fprintf(stderr, "probe: cannot read %s\n", argv[1]); return 2; }
    std::FILE* fo = std::fopen(argv[2], "wb");
    if (!fo) { std::fprintf(stderr, "probe: cannot write %s\n", argv[2]); return 2; }
    unsigned long long head[2];
    if (std::fread(head, 8, 2, fi) != 2 || head[0] != kMagic || head[1] > 4096) { std::fprintf(stderr, "probe: bad request header\n"); return 2; }
    if (std::fwrite(head, 8, 2, fo) != 2) { std::fprintf(stderr, "probe: short write\n"); return 2; }
    double* d_params = nullptr;
    const double h_params[1] = {4.0};  // the run-time accumulator count of lba_trial<0>
    CHECK(hipMalloc(&d_params, sizeof(h_params)));
    CHECK(hipMemcpy(d_params, h_params, sizeof(h_params), hipMemcpyHostToDevice));
    for (unsigned long long c = 0; c < head[1]; ++c) {
        long long ch[3];
        if (std::fread(ch, 8, 3, fi) != 3) { std::fprintf(stderr, "probe: case %llu: short header\n", c); return 2; }
        const long long fn = ch[0], n = ch[1], ny = ch[2];
        if (fn < 0 || fn >= FN_COUNT || n <= 0 || n > kMaxN || ny != kYCols[fn]) {
            std::fprintf(stderr, "probe: case %llu: fn %lld n %lld ycols %lld refused\n", c, fn, n, ny);
            return 2;
        }
        std::vector<double> h_in((size_t)(1 + ny) * n), h_out((size_t)2 * n);
        if (std::fread(h_in.data(), 8, h_in.size(), fi) != h_in.size()) { std::fprintf(stderr, "probe: case %llu: short data\n", c); return 2; }
        if (fn == FN_PRIOR_TERM) {  // (x, kind, a, b) -> (x, kind, a, b as stored, c)
            h_in.resize((size_t)5 * n);
            for (long long i = 0; i < n; ++i) {
                DimTab t;
                if (Refusal r = prior_entry((size_t)i, (int)h_in[n + i], h_in[2 * n + i], h_in[3 * n + i], 0, 0.0, 0.0, &t)) {
                    std::fprintf(stderr, "probe: case %llu row %lld: %s\n", c, i, r.message.c_str());
                    return 2;
                }
                h_in[3 * n + i] = t.b;
                h_in[4 * n + i] = t.c;
            }
        }
        double *d_in = nullptr, *d_out = nullptr;
        CHECK(hipMalloc(&d_in, h_in.size() * 8));
        CHECK(hipMalloc(&d_out, h_out.size() * 8));
        CHECK(hipMemcpy(d_in, h_in.data(), h_in.size() * 8, hipMemcpyHostToDevice));
        CHECK(hipMemset(d_out, 0xff, h_out.size() * 8));  // (a lane that stored nothing reads back as NaN)
        CHECK(hipDeviceSynchronize());
        k_probe<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>((int)fn, d_in, d_in + n, d_out, n, d_params);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(h_out.data(), d_out, h_out.size() * 8, hipMemcpyDeviceToHost));
        CHECK(hipFree(d_in));
        CHECK(hipFree(d_out));
        const long long oh[2] = {fn, n};
        if (std::fwrite(oh, 8, 2, fo) != 2 || std::fwrite(h_out.data(), 8, h_out.size(), fo) != h_out.size()) {
            std::fprintf(stderr, "probe: short write\n");
            return 2;
        }
    }
    CHECK(hipFree(d_params));
    if (std::fclose(fo) != 0) { std::fprintf(stderr, "probe: close failed\n"); return 2; }
    std::fclose(fi);
    std::printf("probe ok: %llu cases\n", head[1]);
    return 0;
}
