// cross_probe.hip -- the matrix-core cross term S_p = sum_i y_p . x_i of csrc/demc_kernels.hpp as DEVICE code on chosen operands:
// k_cross_mfma<KS,4> launched as launch_loglike launches it, and cross_stage<lds_cptr | glb_cptr> / cross_ks<2 | 8, lds_cptr, true> called
// as k_propose<..., STREAM> and k_res_mvn<..., true, DT> call them (tests/test_gpu_cross.py builds it with the FLAGS line of
// csrc/Makefile, less -shared -fPIC, and runs it once; tests/cross_cases.py holds the cases, the references and this file format).
//
//   cross_probe <request file> <result file>
//
// request:  u64 magic, u64 n_cases, then per case  i64 hdr[32], f64 Y[hdr[1]], f64 X[hdr[2]]
// result:   u64 magic, u64 n_cases, then per case  i64 kind, i64 n_out, f64 out[n_out]
//   hdr[0] kind, hdr[1] doubles of Y, hdr[2] doubles of X, hdr[3] n_out
//   kind 0 (k_cross_mfma):  hdr[4] KS, [5] dpad, [6] n_kpass, [7] n_tiles, [8] n_chunks, [9] n_groups, [10] n_act, [11] Np, [12] a_lo,
//                           [13] P, [14] entries of glist (0: nullptr), [15..22] glist.   Y = Ypad[P][dpad], X = Xf[n_tiles + 1][dpad / 4][64],
//                           out = partial[n_kpass * n_chunks][P].  Pass kp: k0 = kp * 4 KS, part0 = kp * n_chunks; grid n_ptiles * n_chunks.
//   kind 1 (resident stage): hdr[4] fn (0 cross_stage<lds_cptr>, 1 cross_stage<glb_cptr>, 2 cross_ks<2,lds_cptr,true>, 3 cross_ks<8,lds_cptr,true>),
//                           [5] dpad, [6] threads (256 | 512), [7] n_act, [8] nact_max (doubles between the waves' rows of out), [9] tiles in X,
//                           [10] xt_lo (tiles of X in front of the source; fn 1 only), [11] zt, [12..19] t_lo of wave 0..7, [20..27] t_hi.
//                           Y = y[n_act][dpad], X = tiles[hdr[9]][dpad / 4][64], out = out[threads / 64][nact_max].
// Every output is pre-filled with kSentinel, so an entry nothing stored to reads back with those bits.  Every case is checked against
// its buffers before it is launched and refused (status 2) if an index could leave them; every HIP call is checked, and any error ends
// the program with a non-zero status before anything else is launched.
#define DEMC_DEVICE_HELPERS_ONLY
#define DEMC_K1_EXTERN
#include "demc_kernels.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace demc;

static const unsigned long long kMagic = 0x3153524344434d44ull;     // "DMCDCRS1"
static const unsigned long long kSentinel = 0x7ff8dead0000beefull;  // a quiet NaN no arithmetic produces

struct StageArgs {
    int fn, dpad, n_act, nact_max, n_lds_tiles, zt;
    int t_lo[8], t_hi[8];
};

// One workgroup.  LDS: ybuf[n_act][dpad] | out[waves][nact_max] | (fn != 1) the tiles, with the zero tile among them.
__global__ __launch_bounds__(512) void k_stage(StageArgs s, const double* __restrict__ Y, const double* __restrict__ X, double* __restrict__ out) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    double* ybuf = smem;
    double* part_l = ybuf + s.n_act * s.dpad;
    double* xs = part_l + ((nw * s.nact_max + 15) & ~15);
    for (int i = tid; i < s.n_act * s.dpad; i += blockDim.x) ybuf[i] = Y[i];
    for (int i = tid; i < nw * s.nact_max; i += blockDim.x) part_l[i] = __longlong_as_double((long long)kSentinel);
    const int nx = s.n_lds_tiles * (s.dpad >> 2) * 64;
    for (int i = tid; i < nx; i += blockDim.x) xs[i] = X[i];
    __syncthreads();
    const int t_lo = s.t_lo[wave], t_hi = s.t_hi[wave];
    lds_ptr outw = (lds_ptr)(part_l + (size_t)wave * s.nact_max);
    switch (s.fn) {
        case 0: cross_stage<lds_cptr>((lds_cptr)ybuf, s.dpad, s.n_act, (lds_cptr)xs, t_lo, t_hi, s.zt, outw, lane); break;
        case 1: cross_stage<glb_cptr>((lds_cptr)ybuf, s.dpad, s.n_act, (glb_cptr)X, t_lo, t_hi, s.zt, outw, lane); break;
        case 2: cross_ks<2, lds_cptr, true>((lds_cptr)ybuf, 8, s.n_act, (lds_cptr)xs, t_lo, t_hi, s.zt, outw, lane); break;
        default: cross_ks<8, lds_cptr, true>((lds_cptr)ybuf, 32, s.n_act, (lds_cptr)xs, t_lo, t_hi, s.zt, outw, lane); break;
    }
    __syncthreads();
    for (int i = tid; i < nw * s.nact_max; i += blockDim.x) out[i] = part_l[i];
}

#define CHECK(call)                                                                                      \
    do {                                                                                                 \
        const hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                          \
            std::fprintf(stderr, "probe: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return 3;                                                                                    \
        }                                                                                                \
    } while (0)
#define REFUSE(c, what)                                                      \
    do {                                                                     \
        std::fprintf(stderr, "probe: case %llu refused: %s\n", c, what);     \
        return 2;                                                            \
    } while (0)

typedef void (*CrossFn)(KParams, const double*, int, int, const double*, int, int, int);
static CrossFn cross_instance(long long ks) {
    switch (ks) {
        case 1: return k_cross_mfma<1, 4>;
        case 2: return k_cross_mfma<2, 4>;
        case 4: return k_cross_mfma<4, 4>;
        case 8: return k_cross_mfma<8, 4>;
        case 16: return k_cross_mfma<16, 4>;
        default: return nullptr;
    }
}

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
    CHECK(hipFuncSetAttribute((const void*)k_stage, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxDynLds));
    for (unsigned long long c = 0; c < head[1]; ++c) {
        long long h[32];
        if (std::fread(h, 8, 32, fi) != 32) { std::fprintf(stderr, "probe: case %llu: short header\n", c); return 2; }
        const long long kind = h[0], ny = h[1], nx = h[2], n_out = h[3];
        const long long kMax = 1ll << 22;
        if (kind < 0 || kind > 1 || ny <= 0 || ny > kMax || nx <= 0 || nx > kMax || n_out <= 0 || n_out > kMax) REFUSE(c, "sizes");
        std::vector<double> hY((size_t)ny), hX((size_t)nx), hO((size_t)n_out);
        if (std::fread(hY.data(), 8, hY.size(), fi) != hY.size() || std::fread(hX.data(), 8, hX.size(), fi) != hX.size()) {
            std::fprintf(stderr, "probe: case %llu: short data\n", c);
            return 2;
        }
        for (auto& v : hO) std::memcpy(&v, &kSentinel, 8);

        // ---- every index the launch can form, against the buffers it is given ----
        KParams p = {};
        StageArgs s = {};
        CrossFn fn = nullptr;
        int n_glist = 0, hglist[8] = {0};
        unsigned grid = 0, threads = 256;
        size_t lds = 0;
        if (kind == 0) {
            const long long KS = h[4], dpad = h[5], n_kpass = h[6], n_tiles = h[7], n_chunks = h[8], n_groups = h[9], n_act = h[10], Np = h[11],
                            a_lo = h[12], P = h[13];
            n_glist = (int)h[14];
            fn = cross_instance(KS);
            if (!fn || n_kpass < 1 || n_kpass > 4 || dpad != 4 * KS * n_kpass) REFUSE(c, "KS, dpad, n_kpass");
            if (n_tiles < 1 || n_tiles > 4096 || n_chunks < 1 || n_chunks > 64) REFUSE(c, "n_tiles, n_chunks");
            if (n_groups < 1 || n_groups > 8 || n_act < 1 || Np < 1 || a_lo < 0 || a_lo + n_act > Np || P < 1 || P > 65536) REFUSE(c, "geometry");
            if (h[14] < 0 || h[14] > 8 || (h[14] != 0 && h[14] != n_groups)) REFUSE(c, "glist length");
            for (int g = 0; g < n_groups; ++g) {
                const long long gg = n_glist ? h[15 + g] : g;
                if (gg < 0 || (gg + 1) * Np > P) REFUSE(c, "a group's slots lie outside [0, P)");
                hglist[g] = (int)gg;
            }
            if (ny != P * dpad || nx != (n_tiles + 1) * (dpad / 4) * 64 || n_out != n_kpass * n_chunks * P) REFUSE(c, "buffer sizes");
            p.n_groups = (int)n_groups; p.n_act = (int)n_act; p.Np = (int)Np; p.a_lo = (int)a_lo; p.P = P;
            const long long n_prop = n_groups * n_act, n_ptiles = (n_prop + 255) / 256;  // four waves of MT * 16 = 64 proposals
            grid = (unsigned)(n_ptiles * n_chunks);
        } else {
            const long long dpad = h[5], wg = h[6], n_act = h[7], nact_max = h[8], n_src = h[9], xt_lo = h[10], zt = h[11];
            s.fn = (int)h[4];
            if (s.fn < 0 || s.fn > 3) REFUSE(c, "fn");
            if (!(dpad == 4 || dpad == 8 || dpad == 16 || dpad == 32 || dpad == 64) || (s.fn == 2 && dpad != 8) || (s.fn == 3 && dpad != 32)) REFUSE(c, "dpad");
            if (wg != 256 && wg != 512) REFUSE(c, "threads");
            if (n_act < 1 || n_act > nact_max || nact_max > 1024) REFUSE(c, "n_act, nact_max");
            if (n_src < 1 || xt_lo < 0 || xt_lo >= n_src || (s.fn != 1 && xt_lo != 0)) REFUSE(c, "tiles, xt_lo");
            const long long n_rel = n_src - xt_lo;  // tiles the source pointer can reach
            if (zt < 0 || zt >= n_rel) REFUSE(c, "zt");
            for (int w = 0; w < 8; ++w) {
                const long long lo = h[12 + w], hi = h[20 + w];
                if (lo < 0 || lo > hi || hi > n_rel) REFUSE(c, "a wave's tile range");
                s.t_lo[w] = (int)lo; s.t_hi[w] = (int)hi;
            }
            const long long nw = wg / 64;
            if (ny != n_act * dpad || nx != n_src * (dpad / 4) * 64 || n_out != nw * nact_max) REFUSE(c, "buffer sizes");
            s.dpad = (int)dpad; s.n_act = (int)n_act; s.nact_max = (int)nact_max; s.zt = (int)zt;
            s.n_lds_tiles = s.fn == 1 ? 0 : (int)n_src;
            lds = ((size_t)n_act * dpad + (size_t)((nw * nact_max + 15) & ~15ll) + (size_t)s.n_lds_tiles * (dpad / 4) * 64) * 8;
            if (lds > kMaxDynLds) REFUSE(c, "more LDS than kMaxDynLds");
            grid = 1; threads = (unsigned)wg;
        }

        double *dY = nullptr, *dX = nullptr, *dO = nullptr;
        int* dG = nullptr;
        CHECK(hipMalloc(&dY, hY.size() * 8));
        CHECK(hipMalloc(&dX, hX.size() * 8));
        CHECK(hipMalloc(&dO, hO.size() * 8));
        CHECK(hipMemcpy(dY, hY.data(), hY.size() * 8, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(dX, hX.data(), hX.size() * 8, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(dO, hO.data(), hO.size() * 8, hipMemcpyHostToDevice));
        if (n_glist) {
            CHECK(hipMalloc(&dG, sizeof(hglist)));
            CHECK(hipMemcpy(dG, hglist, sizeof(hglist), hipMemcpyHostToDevice));
        }
        CHECK(hipDeviceSynchronize());
        if (kind == 0) {
            p.glist = dG;
            p.partial = dO;
            const int KS = (int)h[4], dpad = (int)h[5], n_chunks = (int)h[8];
            for (int kp = 0; kp < (int)h[6]; ++kp) {  // launch_loglike's loop over the k-passes
                fn<<<dim3(grid), dim3(256)>>>(p, dY, dpad, kp * 4 * KS, dX, (int)h[7], n_chunks, kp * n_chunks);
                CHECK(hipGetLastError());
            }
        } else {
            k_stage<<<dim3(1), dim3(threads), lds>>>(s, dY, dX + (size_t)h[10] * (h[5] / 4) * 64, dO);
            CHECK(hipGetLastError());
        }
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(hO.data(), dO, hO.size() * 8, hipMemcpyDeviceToHost));
        CHECK(hipFree(dY));
        CHECK(hipFree(dX));
        CHECK(hipFree(dO));
        if (dG) CHECK(hipFree(dG));
        const long long oh[2] = {kind, n_out};
        if (std::fwrite(oh, 8, 2, fo) != 2 || std::fwrite(hO.data(), 8, hO.size(), fo) != hO.size()) {
            std::fprintf(stderr, "probe: short write\n");
            return 2;
        }
    }
    if (std::fclose(fo) != 0) { std::fprintf(stderr, "probe: close failed\n"); return 2; }
    std::fclose(fi);
    std::printf("probe ok: %llu cases\n", head[1]);
    return 0;
}
