// demc_hip.cpp -- host runtime and C-ABI (include/demc.h) of libdemc_hip.so.
//
// The handle owns every device buffer (particles, proposals, partial sums, history, model data laid out
// for the kernels) and one HIP stream; demc_step() enqueues, per iteration, the launch schedule that
// step!/update!/block_update!/mutate_or_crossover! (main.jl:84-207) imply:
//     [migration pack + apply]  then per sweep (block) and per colour phase:  K1 propose -> K2 loglike -> K3 accept/store
// All per-iteration randomness is addressed by (seed, iteration, entity) inside the kernels, so the host
// loop needs no device->host traffic: what the host draws -- the alpha coin, select_groups, the frozen sweeps' mutation coins -- are
// pure functions of (seed, iteration), re-drawn in demc_schedule.hpp with the kernels' own Philox text (demc_philox.hpp).
//
// There is NO CPU fallback in this file: every compute entry point launches HIP kernels or fails.
//
// What is launched -- kernel instance, grid, workgroup size, LDS bytes, chunk counts, fuse flags -- is decided in demc_geometry.hpp,
// host-only code that knows neither HIP nor the handle; what a model's data become before they are uploaded, in demc_prep.hpp; what a
// step call does iteration by iteration -- its refusals, its segments, the phases of a sweep, the frozen order --, in demc_schedule.hpp.
// This file gathers their inputs from the handle, asks the device what only it knows, and does what the plans say.
#include "../../include/demc.h"
#include "../../include/demc_summary.h"  // demc_summarize
#include "../../include/demc_quantile.h"  // demc_quantiles
#include "../../include/demc_cov.h"  // demc_covariance
#include "../../include/demc_pointwise.h"  // demc_pointwise_loglik, demc_waic
#include "../../include/demc_loo.h"  // demc_loo
#include "../../include/demc_bridge.h"  // demc_bridge
#include "../../include/demc_rank.h"  // demc_rankstats, demc_rank_series
#include "../../include/demc_hpd.h"  // demc_hpd

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hiprtc.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#define DEMC_K1_EXTERN  // the k_propose instances live in demc_k1_{phase,res,stream}.cpp
#include "demc_kernels.hpp"
#define DEMC_LONGROW_EXTERN  // k_longrow<256 / 512> are instantiated in demc_longrow.cpp
#include "demc_longrow.hpp"
#define DEMC_FROZEN_EXTERN  // ... k_frozen_sweep in demc_frozen.cpp, k_res_mvn in demc_resmvn.cpp (compiled side by side)
#include "demc_frozen.hpp"
#define DEMC_RESMVN_EXTERN
#include "demc_resmvn.hpp"
#define DEMC_RESOBS_EXTERN
#include "demc_resobs.hpp"
#define DEMC_SIMLIKE_EXTERN  // k_sim_loglike in demc_simlike.cpp
#include "demc_simlike.hpp"
#define DEMC_ODE_EXTERN  // k_ode_loglike in demc_ode.cpp
#include "demc_ode.hpp"
#include "demc_summary.hpp"  // demc_summarize: its kernels and their launches live in demc_summary.cpp
#include "demc_quantile.hpp"  // demc_quantiles: likewise, demc_quantile.cpp
#include "demc_cov.hpp"  // demc_covariance: likewise, demc_cov.cpp
#include "demc_pointwise.hpp"  // demc_pointwise_loglik, demc_waic: likewise, demc_pointwise.cpp
#include "demc_loo.hpp"  // demc_loo: likewise, demc_loo.cpp (with its host-only plan, demc_looplan.hpp)
#include "demc_bridge.hpp"  // demc_bridge: likewise, demc_bridge.cpp (with its host-only plan, demc_bridgeplan.hpp)
#include "demc_rank.hpp"  // demc_rankstats, demc_rank_series: likewise, demc_rank.cpp (with its host-only plan, demc_rankplan.hpp)
#include "demc_devmem.hpp"  // owners of the device memory, pinned memory, events and modules the handle holds
#include "demc_prep.hpp"  // host-only: a model's data and constants, the prior table and its run-length forms, every refusal of those
#include "demc_instances.hpp"  // one table per templated kernel, built from the lists above: every choice of an instance goes through them
#include "demc_geometry.hpp"  // host-only: every launch-geometry decision, as plans the launches below carry out
#include "demc_postplan.hpp"  // host-only: the history window and the plans of demc_summarize, demc_quantiles, demc_covariance
#include "demc_pwplan.hpp"  // host-only: the families, refusals and plan of demc_pointwise_loglik and demc_waic
#include "demc_schedule.hpp"  // host-only: what a step call does iteration by iteration -- coins, refusals, segments, phases, frozen order

using namespace demc;

#ifndef DEMC_ARCH_STR
#define DEMC_ARCH_STR "gfx950"  // the Makefile passes its ARCH, so that the JIT-compiled plug-in matches the library
#endif
static_assert(kPwFamSim == FAM_SIM, "demc_pwplan.hpp names the simulation likelihood by the runtime's family");
static_assert(kBridgeFamSim == FAM_SIM, "demc_bridgeplan.hpp names the simulation likelihood by the runtime's family");
static_assert(kPrepOdeMaxT == kOdeMaxT && kPrepOdeMaxSubsteps == kOdeMaxSubsteps && kPrepSimMaxN == kSimMaxN && kPrepSimChoiceMaxN == kSimChoiceMaxN,
              "demc_prep.hpp refuses by the kernels' caps");

namespace {

struct Timed {
    hipEvent_t a, b;
    int cls;
    bool started = false;  // a kernel of the bracket carries the events (LAUNCH_T)
};

// The whole-update forms (enum Form, demc_geometry.hpp): planned once per model into a FormPlan -- the geometry plus the
// instance(s) it names (size_k1_lds) --, chosen per step (choose_form), launched by launch_form.  FORM_PHASE, which serves every
// configuration, is planned per launch (launch_phase).
struct FormPlan : FormGeo {
    // the instance(s), resolved when the model is planned (a missing one fails there, not at step 1): per LEAN level for the two
    // k_propose forms (a trace or a replay lowers it to 0 at run time: lean_level), per HIST - 1 for FORM_LEAN_Z, else [0]
    const K1Inst* k1[3] = {};
};

// The observation stream inside a resident kernel: its geometry (StreamDims) and the buffers that go with it.
struct StreamGeo : StreamDims {
    DevBuf<unsigned long long> gran;  // hand-over granules (device), [2][n_groups][C][nact_max][2]
    PinnedBuf<unsigned> err;          // time-out flag (host-mapped, zero-copy)
};

// Everything a set-model call defines: the sizes and constants prepare_model works out (ModelShape, demc_prep.hpp) and what lives
// on the device.  The default state is "no model"; clear_model is the one place a model is released.
struct Model : ModelShape {
    int family = -1;
    int direct_wgs_per_cu = 0;  // DIRECT mode: resident workgroups of its kernel per CU (wgs_per_cu: asked once per model)
    int direct4_wgs_per_cu = 0;  // ... and of the four-per-lane instance of that row length, where there is one
    DevBuf<double> data, Ainv, Ypad, Xf, sx, xbar;
    DevBuf<int> order;  // LBA: the caller's index of sorted trial k (the per-observation calls answer in the caller's order)
    // user plug-in (demc_set_model_source): JIT-compiled module, kernel and its hyper-parameters
    Module user_module;
    hipFunction_t user_kernel = nullptr;
    DevBuf<double> user_hyper;
    int user_nhyper = 0;
    bool user_row = false;        // whole-row plug-in (demc_set_model_source_row): one workgroup per proposal
    bool user_has_prior = false;  // ... whose source also defines demc_user_prior_row
    DevBuf<long long> user_dims;
    int user_ndims = 0;
    // simulation-based likelihood (demc_set_model_sim, demc_simlike.hpp); a user simulator's module lives in user_module / user_kernel
    int sim_kind = -1, sim_est = 0, sim_n = 0;
    int sim_kmax = 0;              // KDE_CHOICE: the largest observed choice
    double sim_bw = 0.0;
    DevBuf<double> sim_logtab;     // [n_sim + 1] log(c / n_sim): the frequency estimator's terms
};

// demc_set_replay: device copies of the caller's draws.  Cleared by assigning Replay{}.
struct Replay {
    DevBuf<double> group, part, noise, znoise, recomb;
    DevBuf<long long> partner, mig_particle;
    DevBuf<int> mig_groups;
    int n_mig = 0;
    bool active = false, has_step = false;
    double u_step = 0.0;
};

}  // namespace

struct demc_handle {
    demc_config c{};
    long long P = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // state
    DevBuf<double> theta, weight, prop, prop_prior, prop_adj, tr_w, partial, aux;
    DevBuf<DimTab> dimtab;
    std::vector<DimTab> h_tab;  // host copy: bounds and priors arrive in separate calls
    DevBuf<DimSeg> dimseg;      // run-length form of the table (kMaxDimSeg entries)
    int n_seg = 0;              // 0: more segments than kMaxDimSeg, the kernels read dimtab
    bool normal_ref = false;    // the table has a Normal(a, theta[ref]) entry
    int seg_start[kMaxDimSeg] = {0};
    unsigned seg_plain = 0;     // segments with a flat / Normal / Normal(a, theta[ref]) prior
    std::vector<MaskRuns> mask_runs;  // per block sweep: the mask run-length encoded (n = 0: too many runs)
    DevBuf<double> hist, lp_hist, mig_rows, scratch_theta, scratch_w;
    DevBuf<long long> id;
    DevBuf<unsigned char> prop_oob, tr_acc, masks, acc_hist;
    DevBuf<int> tr_idx, id_hist;
    Model m;                      // the model currently set (family -1: none)
    int obs_wgs_per_cu = 0;       // resident workgroups of k_obs_loglike per CU (wgs_per_cu: asked once) ...
    int lba_wave_wgs_per_cu = 0;  // ... and of k_lba_wave: whatever the model
    unsigned sim_entity_base = 0;  // demc_logpost on a simulated likelihood: row r of a call is evaluated at entity r
    // DEMC_PRIOR_TRUNCNORMAL: the device's table holds a Normal entry whose constant carries the mass between the bounds; the scale
    // the caller gave (0: the scalar's prior is not a truncated Normal) is kept here so that the constant follows the bounds
    std::vector<double> trunc_sd;
    int partial_cap = 64;
    int lpp = 1;
    K1Lds k1;  // K1 LDS carve-up for the model and the population (size_k1_lds)
    FormPlan form[N_FORMS];  // the whole-update forms (size_k1_lds plans them; [FORM_PHASE] is not used)
    StreamGeo st;
    // by-product snapshot (KParams::snap_theta / snap_weight): the rows and weights a frozen sweep over the whole population ended
    // with, valid as the sweep-start snapshot of sweep `snap2_sweep` of iteration `snap2_iter` (and of nothing else)
    DevBuf<double> snap2, snap2_w;
    int64_t snap2_iter = -1;
    int snap2_sweep = -1;
    // k_frozen_sweep: launch order of the groups per (iteration, block sweep) of the current demc_step call (fill_frozen_order)
    struct FrozenOrder {
        StagedList<int> table;  // (staged through pinned memory: a truly asynchronous copy, nothing is drained)
        long long iter0 = 0;    // the iterations it covers (none: no table for the current call)
        int iters = 0;
    } frozen;
    int n_cus = 0;
    bool bracket_open = false;  // timing: between tick(begin) and tick(end) of a bracket whose kernels carry the events
    size_t lr_two_lds = 0;     // long-row kernel: the dynamic LDS size lr_two_fit was asked for
    bool lr_two_fit = false;   // ... two 256-thread workgroups with that much LDS fit on a CU
    // update of a subset of the groups (demc_update_groups_async): each call takes the next slot of a ring of staged lists
    // (sized once, at create), and the device list in force
    struct GroupLists {
        static constexpr int kRing = 8;
        StagedList<int> slot[kRing];
        int next = 0;
    } glist;
    const int* cur_glist = nullptr;
    int cur_ng = 0;
    std::string err;
    Replay rp;
    int geo_groups = 0;  // groups the lane geometry is sized for (demc_config.geometry_groups, else n_groups)
    int hist_ld = 0;     // doubles between consecutive history cells (KParams::hist_ld)
    // the one collective of the path: an RCCL communicator owned by the handle (demc_comm_init), or lent by the
    // single-process multi-GPU set the handle is a shard of (demc_create_multi)
    ncclComm_t comm = nullptr;
    bool own_comm = false;
    int comm_rank = 0, comm_world = 1;
    bool comm_overlap = false;        // demc_comm_set_overlap: unselected groups update while the all-gather is in flight
    hipStream_t side = nullptr;       // ... on this stream
    Event ev_pack, ev_gath;
    DevBuf<double> red_dev;           // demc_comm_allreduce staging
    size_t red_cap = 0;
    long long n_exchanges = 0;        // all-gathers issued (diagnostic, demc_comm_stats)
    struct demc_multi* multi = nullptr;
    bool multi_sealed = false;  // the set is built: demc_set_stream is refused from here on
    // which kernel instances the last update launched (demc_last_kernels: lets a test name the instance it compared)
    struct LastPlan {
        const K1Inst* k1 = nullptr;  // the entry that was launched (its key names it)
        K2Kind k2 = K2_NONE;         // the likelihood kernel behind it (none: fused into K1) ...
        InstKey k2_key = {};         // ... and the key of its instance (k_cross_mfma, k_direct_mvn; k_sim_loglike: <SIM, EST>, SIM_USER for the JIT one)
        bool k3 = false;             // k_accept_store followed
    } last;
    // timing
    bool timing = false;
    std::vector<Timed> events;
    std::vector<hipEvent_t> event_pool;  // recycled events: a timed launch costs two hipEventRecord, no create/destroy
    double t_ms[5] = {0, 0, 0, 0, 0};
    long long t_n[5] = {0, 0, 0, 0, 0};
    // clock probe of the DIRECT likelihood kernel (demc_timing_clock): per workgroup {s_memtime, s_memrealtime, XCD} at its end
    DevBuf<unsigned long long> clk_dev;
    size_t clk_cap = 0, clk_n = 0;  // workgroups the buffer holds / the last timed launch wrote
};

namespace {

int fail(demc_handle* h, int code, const std::string& msg) noexcept {
    if (h) {
        try {
            h->err = msg;
        } catch (...) {  // not even the message could be stored: the code alone goes back
        }
    }
    return code;
}
int fail(demc_handle* h, const Refusal& r) noexcept { return fail(h, r.code, r.message); }

// No C++ exception crosses the C-ABI (include/demc.h): every extern "C" body runs inside this guard.
template <typename F>
int32_t guarded(demc_handle* h, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(h, DEMC_ENOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(h, DEMC_EHIP, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(h, DEMC_EHIP, "internal error (unknown exception)");
    }
}

#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(h, DEMC_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                    \
    } while (0)

// A handle belongs to one GPU; a host that drives several handles from one thread may have another device current.
#define USE_DEVICE(h) HIPCHK(hipSetDevice((h)->c.device_id))

template <typename T>
int dev_alloc(demc_handle* h, DevBuf<T>& p, size_t n) {
    if (n == 0) n = 1;
    hipError_t e = p.alloc(n);
    if (e != hipSuccess) return fail(h, DEMC_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    // hipMemset runs on the null stream and may return before the fill has happened; the handle's own stream is
    // non-blocking, i.e. NOT ordered behind the null stream -- without the wait a kernel launched right after an
    // allocation (demc_export_chains) could have its output zeroed underneath it.
    e = hipMemset(p.get(), 0, n * sizeof(T));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(h, DEMC_EHIP, std::string("hipMemset: ") + hipGetErrorString(e));
    return DEMC_OK;
}
#define ALLOC(ptr, n)                          \
    do {                                       \
        int rc_ = dev_alloc(h, (ptr), (n));    \
        if (rc_ != DEMC_OK) return rc_;        \
    } while (0)

// a prepared vector to a device buffer of its size; an empty one leaves the buffer unallocated
int upload(demc_handle* h, DevBuf<double>& dst, const std::vector<double>& src) {
    if (src.empty()) return DEMC_OK;
    ALLOC(dst, src.size());
    HIPCHK(hipMemcpy(dst, src.data(), sizeof(double) * src.size(), hipMemcpyHostToDevice));
    return DEMC_OK;
}

// Device time per kernel class (demc_timing_enable): the events of a bracket travel IN the dispatch packets of its kernels
// (hipExtLaunchKernelGGL: start event on the first, stop event on every one -- the last record stands), so they read the
// kernels' own begin / end timestamps and put no barrier packets between the launches.  (Events recorded around each launch
// cost the cfg4 share 28 us per iteration of 160.)  `classic`: record the events around the bracket instead (module launch).
void tick(demc_handle* h, int cls, bool begin, bool classic = false) {
    if (!h->timing) return;
    if (begin) {
        Timed t;
        auto take = [&](hipEvent_t* e) {
            if (!h->event_pool.empty()) {
                *e = h->event_pool.back();
                h->event_pool.pop_back();
            } else
                hipEventCreate(e);
        };
        take(&t.a);
        take(&t.b);
        t.cls = cls;
        if (classic) {
            hipEventRecord(t.a, h->stream);
            t.started = true;
        }
        h->events.push_back(t);
        h->bracket_open = !classic;
    } else {
        if (classic) hipEventRecord(h->events.back().b, h->stream);
        h->bracket_open = false;
    }
}

#define LAUNCH_T(h, kern, grid, block, lds, ...)                                                                          \
    do {                                                                                                                  \
        if ((h)->timing && (h)->bracket_open) {                                                                           \
            Timed& t__ = (h)->events.back();                                                                              \
            hipExtLaunchKernelGGL(kern, grid, block, lds, (h)->stream, t__.started ? nullptr : t__.a, t__.b, 0, __VA_ARGS__); \
            t__.started = true;                                                                                           \
        } else                                                                                                            \
            hipLaunchKernelGGL(kern, grid, block, lds, (h)->stream, __VA_ARGS__);                                         \
    } while (0)

void drain_events(demc_handle* h) {
    for (auto& t : h->events) {
        if (t.started) {  // (a bracket may hold no launch at all)
            hipEventSynchronize(t.b);
            float ms = 0.f;
            hipEventElapsedTime(&ms, t.a, t.b);
            h->t_ms[t.cls] += ms;
            h->t_n[t.cls] += 1;
        }
        h->event_pool.push_back(t.a);
        h->event_pool.push_back(t.b);
    }
    h->events.clear();
}

// The instance of `kernel` with the template arguments `key`: the table's entry, or DEMC_EUNSUPPORTED (never a null launch).
template <typename I, size_t N>
int pick(demc_handle* h, const char* kernel, const I (&tab)[N], const InstKey& key, const I** out) {
    if ((*out = find_inst(tab, key))) return DEMC_OK;
    return fail(h, DEMC_EUNSUPPORTED, std::string("no instance ") + kernel + "<" + int_list(key, kMaxKey) + "> in this library");
}
#define PICK(out, kernel, tab, ...) \
    do { if (int rc_ = pick(h, kernel, tab, InstKey{{__VA_ARGS__}}, &(out))) return rc_; } while (0)

// resident 256-thread workgroups of `fn` per CU: asked once, kept in *cached (0: not asked yet)
int wgs_per_cu(demc_handle* h, const void* fn, int* cached) {
    if (*cached == 0) {
        int nb = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, 0));
        *cached = nb > 0 ? nb : 1;
    }
    return DEMC_OK;
}

// The plain values the geometry rules read (demc_geometry.hpp), gathered from the handle: integers and pointers, built per call.
Setup setup_of(const demc_handle* h) {
    Setup s;
    s.c = &h->c; s.m = &h->m; s.family = h->m.family; s.user_row = h->m.user_row;
    s.n_seg = h->n_seg; s.seg_start = h->seg_start; s.normal_ref = h->normal_ref; s.has_hist = h->hist.get() != nullptr;
    s.partial_cap = h->partial_cap; s.geo_groups = h->geo_groups; s.n_cus = h->n_cus; s.lpp = h->lpp; s.k1 = &h->k1;
    s.replay = h->rp.active; s.subset = h->cur_glist != nullptr;
    return s;
}

KParams base_params(demc_handle* h) {
    KParams k;
    std::memset(&k, 0, sizeof k);
    const demc_config& c = h->c;
    k.n_groups = c.n_groups; k.Np = c.Np; k.D = c.D; k.group_offset = c.group_offset;
    k.a_lo = 0; k.n_act = c.Np; k.pool_lo = 0; k.pool_n = c.Np; k.exclude_self = 1;
    k.lpp = h->lpp; k.lpp3 = h->lpp > 256 ? 256 : h->lpp; k.mode = MODE_STEP;
    k.iter = 0; k.burnin = c.burnin; k.sweep = 0; k.seed = c.seed;
    k.beta = c.beta; k.eps = c.eps; k.sigma = c.sigma; k.kappa = c.kappa; k.theta_snooker = c.theta_snooker;
    k.proposal_kind = c.proposal_kind; k.partner_kind = c.partner_kind; k.update_kind = c.update_kind;
    k.fitness_kind = c.fitness_kind;
    k.theta = h->theta; k.weight = h->weight; k.id = h->id; k.prop = h->prop; k.prop_prior = h->prop_prior;
    k.prop_adj = h->prop_adj; k.prop_oob = h->prop_oob; k.tr_idx = h->tr_idx; k.tr_w = h->tr_w; k.tr_acc = h->tr_acc;
    k.dimtab = h->dimtab; k.dimseg = h->dimseg; k.n_seg = h->n_seg; k.ainv_lds = h->k1.ainv_lds; k.mask = nullptr;
    std::memcpy(k.seg_start, h->seg_start, sizeof k.seg_start);
    k.seg_plain = h->seg_plain;
    std::memset(k.mrun_start, 0, sizeof k.mrun_start);
    k.n_mrun = 1; k.mrun_in = 1u;  // no block mask: one run, inside
    k.hist = h->hist; k.acc_hist = h->acc_hist; k.lp_hist = h->lp_hist; k.id_hist = h->id_hist; k.hist_ld = h->hist_ld;
    k.P = h->P; k.store_row = -1; k.tile_in_lds = h->k1.tile_in_lds;
    k.family = h->m.family; k.N = h->m.N; k.d = h->m.d; k.n_acc = h->m.n_acc; k.n_partials = 1;
    k.partial = h->partial; k.aux = h->aux; k.data = h->m.data; k.data2 = h->m.data ? h->m.data + h->m.data2_off : nullptr;
    k.c0 = h->m.c0; k.c1 = h->m.c1; k.c2 = h->m.c2;
    k.direct = (is_mvn(h->m.family) && c.loglike_mode == DEMC_LOGLIKE_DIRECT) ? 1 : 0;
    k.n_split = 1; k.fuse_prep = 0; k.prep_mfma = 0; k.fuse_obs = 0; k.fuse_accept = 0; k.plan = 0;
    k.scr_doubles = (int)(h->k1.scr_bytes / sizeof(double)); k.write_prop = 1; k.trace = c.trace;
    k.Ainv = h->m.Ainv; k.sx = nullptr; k.xbar = h->m.xbar; k.Ypad = h->m.Ypad; k.dpad = h->m.dpad;
    k.rp_group = h->rp.group; k.rp_part = h->rp.part; k.rp_partner = h->rp.partner; k.rp_noise = h->rp.noise;
    k.rp_znoise = h->rp.znoise; k.rp_recomb = h->rp.recomb; k.rp_mig_groups = h->rp.mig_groups;
    k.rp_mig_particle = h->rp.mig_particle; k.rp_n_mig = h->rp.n_mig;
    k.glist = h->cur_glist;
    if (h->cur_glist) k.n_groups = h->cur_ng;
    return k;
}

// Kernarg of the JIT-compiled user-likelihood kernel: ONE definition, compiled here and -- as text -- prepended to the user's source.
#define DEMC_USER_KPARAMS                                                   \
    struct UserKParams {                                                    \
        int n_groups, Np, D, a_lo, n_act, n_chunks, nhyper, with_prior;     \
        long long N, P;                                                     \
        const double* prop;                                                 \
        double* partial;                                                    \
        const double* data;                                                 \
        const double* hyper;                                                \
        const long long* dims;                                              \
        const int* glist;                                                   \
        int ndims, pad;                                                     \
    };
DEMC_USER_KPARAMS
#define DEMC_STR_(...) #__VA_ARGS__
#define DEMC_STR(...) DEMC_STR_(__VA_ARGS__)
const char* kUserStruct = R"SRC(
#ifndef INFINITY
#define INFINITY __builtin_huge_val()
#endif
#ifndef NAN
#define NAN __builtin_nan("")
#endif
)SRC" DEMC_STR(DEMC_USER_KPARAMS) "\n";
const char* kUserPrologue = R"SRC(
__device__ double demc_user_obs(const double* theta, int D, const double* data, long long N, long long i,
                                const double* hyper, int nhyper);
)SRC";
// whole-row plug-in: the user's functions return the share of lane `lane` of `n_lanes` cooperating lanes
const char* kUserRowPrologue = R"SRC(
__device__ double demc_user_loglike_row(const double* theta, int D, const double* data, const long long* dims, int ndims,
                                        const double* hyper, int nhyper, int lane, int n_lanes);
#ifdef DEMC_USER_HAS_PRIOR
__device__ double demc_user_prior_row(const double* theta, int D, const double* hyper, int nhyper, int lane, int n_lanes);
#endif
)SRC";
// one workgroup of 256 lanes per proposal; the lanes' shares are summed in a fixed order (wave butterfly, then the four
// waves left to right), so the result does not depend on scheduling
const char* kUserRowKernel = R"SRC(
extern "C" __global__ __launch_bounds__(256) void k_user_row(UserKParams p) {
    __shared__ double s_part[4];
    const int q = blockIdx.x;
    const int g = q / p.n_act;
    const size_t slot = (size_t)(p.glist ? p.glist[g] : g) * p.Np + p.a_lo + (q - g * p.n_act);
    const double* th = p.prop + slot * p.D;
    double acc = demc_user_loglike_row(th, p.D, p.data, p.dims, p.ndims, p.hyper, p.nhyper, (int)threadIdx.x, 256);
#ifdef DEMC_USER_HAS_PRIOR
    if (p.with_prior) acc += demc_user_prior_row(th, p.D, p.hyper, p.nhyper, (int)threadIdx.x, 256);
#endif
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.partial[slot] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}
)SRC";
// thread per proposal x observation chunks: same mapping as k_obs_loglike
const char* kUserKernel = R"SRC(
extern "C" __global__ __launch_bounds__(256) void k_user_loglike(UserKParams p) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int chunk = blockIdx.y;
    if (q >= p.n_groups * p.n_act) return;
    const int g = q / p.n_act;
    const size_t slot = (size_t)(p.glist ? p.glist[g] : g) * p.Np + p.a_lo + (q - g * p.n_act);
    const double* th = p.prop + slot * p.D;
    const long long per = (p.N + p.n_chunks - 1) / p.n_chunks;
    const long long i0 = chunk * per, i1 = (i0 + per < p.N) ? i0 + per : p.N;
    double acc = 0.0;
    for (long long i = i0; i < i1; ++i) acc += demc_user_obs(th, p.D, p.data, p.N, i, p.hyper, p.nhyper);
    p.partial[(size_t)chunk * p.P + slot] = acc;
}
)SRC";

// demc_timing_clock: with timing enabled the compute-bound likelihood kernels (k_direct_mvn, k_lba_wave) leave per workgroup
// {s_memtime, s_memrealtime, CU} as they end; the buffer is zeroed on the stream ahead of the launch (a workgroup whose first wave
// has no proposal reports nothing) and sized for the launch's grid.  Null when timing is off.
int clock_buffer(demc_handle* h, size_t wgs, unsigned long long** out) {
    *out = nullptr;
    if (!h->timing) return DEMC_OK;
    if (wgs > h->clk_cap) {
        if (h->clk_dev) { HIPCHK(hipStreamSynchronize(h->stream)); h->clk_cap = 0; }
        ALLOC(h->clk_dev, 3 * wgs);  // (the old buffer goes as the new one comes)
        h->clk_cap = wgs;
    }
    HIPCHK(hipMemsetAsync(h->clk_dev, 0, 3 * wgs * sizeof(unsigned long long), h->stream));
    h->clk_n = wgs;
    *out = h->clk_dev;
    return DEMC_OK;
}

// The text of demc_simlike.hpp, embedded by the build (csrc/Makefile): what hiprtc compiles around a user simulator.
const char* kSimKernelSource =
#include "demc_simlike_src.inc"
    ;

// K2 of a simulation-based model: one workgroup per proposal, the simulated sample in LDS (demc_simlike.hpp)
int launch_sim_loglike(demc_handle* h, KParams& k, long long n_prop) {
    SimKParams s;
    std::memset(&s, 0, sizeof s);
    s.n_groups = k.n_groups; s.Np = k.Np; s.D = k.D; s.a_lo = k.a_lo; s.n_act = k.n_act; s.group_offset = k.group_offset;
    s.n_sim = h->m.sim_n; s.nhyper = h->m.user_nhyper > 0 ? h->m.user_nhyper - 1 : 0;
    s.n_obs = h->m.N; s.iter = k.iter; s.seed = k.seed; s.sweep = k.sweep; s.entity_base = h->sim_entity_base;
    s.bandwidth = h->m.sim_bw; s.n_pow = std::pow((double)h->m.sim_n, -0.2);
    s.prop = k.prop; s.partial = k.partial; s.obs = h->m.data; s.hyper = h->m.user_hyper ? h->m.user_hyper + 1 : nullptr;
    s.logtab = h->m.sim_logtab; s.glist = k.glist; s.k_max = h->m.sim_kmax;
    const size_t lds = h->m.sim_est == EST_KDE_CHOICE ? sim_choice_lds(h->m.sim_n) : (size_t)h->m.sim_n * sizeof(double);
    h->last.k2 = K2_SIM; h->last.k2_key = InstKey{{h->m.sim_kind, h->m.sim_est}};
    if (h->m.sim_kind == SIM_USER) {
        size_t sz = sizeof s;
        void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &s, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
        tick(h, 2, true, true);
        const hipError_t e = hipModuleLaunchKernel(h->m.user_kernel, (unsigned)n_prop, 1, 1, 256, 1, 1, 0, h->stream, nullptr, cfg);
        tick(h, 2, false, true);
        if (e != hipSuccess) return fail(h, DEMC_EHIP, std::string("hipModuleLaunchKernel: ") + hipGetErrorString(e));
        return DEMC_OK;
    }
    const Inst<SimFn>* e = nullptr;
    PICK(e, "k_sim_loglike", kSim, h->m.sim_kind, h->m.sim_est);
    tick(h, 2, true);
    LAUNCH_T(h, e->fn, dim3((unsigned)n_prop), dim3(256), lds, s);
    tick(h, 2, false);
    return DEMC_OK;
}

// K2 of an ODE-trajectory model: one thread per proposal, a grid row of workgroups per launch group (demc_ode.hpp)
int launch_ode_loglike(demc_handle* h, KParams& k) {
    OdeKParams o;
    std::memset(&o, 0, sizeof o);
    o.n_groups = k.n_groups; o.Np = k.Np; o.D = k.D; o.a_lo = k.a_lo; o.n_act = k.n_act;
    o.T = (int)h->m.N; o.substeps = h->m.ode_substeps;
    std::memcpy(o.u0, h->m.ode_u0, sizeof o.u0);
    o.h = h->m.ode_h; o.h2 = 0.5 * h->m.ode_h; o.h6 = h->m.ode_h / 6.0;
    o.prop = k.prop; o.partial = k.partial; o.obs = h->m.data; o.glist = k.glist;
    const Inst<OdeFn>* e = nullptr;
    PICK(e, "k_ode_loglike", kOde, ODE_LV);
    h->last.k2 = K2_ODE; h->last.k2_key = e->key;
    const size_t lds = (size_t)h->m.N * 2 * sizeof(double);
    tick(h, 2, true);
    LAUNCH_T(h, e->fn, dim3((unsigned)k.n_groups, (unsigned)((k.n_act + 255) / 256)), dim3(256), lds, o);
    tick(h, 2, false);
    return DEMC_OK;
}

// K2 dispatch for the active set described by k: the plan (demc_geometry.hpp: which kernel, its grid and chunk counts), then the
// launch.  Sets k.n_partials.
int launch_loglike(demc_handle* h, KParams& k) {
    const long long n_prop = (long long)k.n_groups * k.n_act;
    if (n_prop == 0) return DEMC_OK;
    k.n_partials = 1;
    if (h->m.family == FAM_SIM) return launch_sim_loglike(h, k, n_prop);
    if (h->m.family == FAM_ODE_LV) return launch_ode_loglike(h, k);
    const Setup s = setup_of(h);
    // the occupancy the kernel's chunk rule reads: asked once, kept
    Occupancy occ;
    const Inst<ChunkFn>* ec = nullptr;  // k_direct_mvn / k_lba_wave
    switch (k2_kind(s)) {
        case K2_DIRECT_MVN:
            PICK(ec, "k_direct_mvn", kDirect, h->m.dp_direct);
            if (int rc = wgs_per_cu(h, (const void*)ec->fn, &h->m.direct_wgs_per_cu)) return rc;
            occ.direct = h->m.direct_wgs_per_cu;
            if (const Inst<ChunkFn>* e4 = find_inst(kDirect, InstKey{{h->m.dp_direct, 4}})) {
                if (int rc = wgs_per_cu(h, (const void*)e4->fn, &h->m.direct4_wgs_per_cu)) return rc;
                occ.direct4 = h->m.direct4_wgs_per_cu;
            }
            break;
        case K2_OBS:
            if (int rc = wgs_per_cu(h, (const void*)k_obs_loglike, &h->obs_wgs_per_cu)) return rc;
            occ.obs = h->obs_wgs_per_cu;
            break;
        case K2_LBA_WAVE:
            PICK(ec, "k_lba_wave", kLbaWave, 3);
            if (int rc = wgs_per_cu(h, (const void*)ec->fn, &h->lba_wave_wgs_per_cu)) return rc;
            occ.lba_wave = h->lba_wave_wgs_per_cu;
            break;
        default: break;
    }
    const LoglikePlan pl = plan_loglike(s, n_prop, occ);
    if (pl.refused) return fail(h, pl.refused, pl.why);
    h->last.k2 = pl.kind;
    const dim3 grid(pl.grid_x, pl.grid_y);
    switch (pl.kind) {
        case K2_DIRECT_MVN:
        case K2_LBA_WAVE: {
            if (pl.kind == K2_LBA_WAVE) PICK(ec, "k_lba_wave", kLbaWave, pl.key[0]);
            else PICK(ec, "k_direct_mvn", kDirect, pl.key[0], pl.key[1]);
            h->last.k2_key = ec->key;
            // timing on: every workgroup also leaves its shader-clock / reference-clock ticks (demc_timing_clock)
            unsigned long long* clk = nullptr;
            if (int rc = clock_buffer(h, (size_t)pl.grid_x * (size_t)pl.n_chunks, &clk)) return rc;
            tick(h, 2, true);
            LAUNCH_T(h, ec->fn, grid, dim3(256), 0, k, pl.n_chunks, clk);
            tick(h, 2, false);
        } break;
        case K2_CROSS_MFMA: {
            const Inst<CrossFn>* e = nullptr;
            PICK(e, "k_cross_mfma", kCross, pl.key[0], pl.key[1]);
            h->last.k2_key = e->key;
            tick(h, 2, true);
            for (int kp = 0; kp < pl.n_kpass; ++kp)
                LAUNCH_T(h, e->fn, grid, dim3(256), 0, k, h->m.Ypad.get(), h->m.dpad, kp * pl.k0_stride, h->m.Xf.get(), h->m.n_tiles, pl.n_chunks,
                         kp * pl.part0_stride);
            tick(h, 2, false);
        } break;
        case K2_OBS:
            tick(h, 2, true);
            LAUNCH_T(h, k_obs_loglike, grid, dim3(256), 0, k, pl.n_chunks);
            tick(h, 2, false);
            break;
        case K2_USER:
        case K2_USER_ROW: {
            UserKParams u;
            u.n_groups = k.n_groups; u.Np = k.Np; u.D = k.D; u.a_lo = k.a_lo; u.n_act = k.n_act; u.n_chunks = pl.n_chunks;
            u.nhyper = h->m.user_nhyper; u.with_prior = h->c.fitness_kind == DEMC_FITNESS_POSTERIOR ? 1 : 0;
            u.N = h->m.N; u.P = h->P; u.prop = k.prop; u.partial = k.partial;
            u.data = h->m.data; u.hyper = h->m.user_hyper; u.dims = h->m.user_dims; u.glist = k.glist; u.ndims = h->m.user_ndims; u.pad = 0;
            size_t sz = sizeof u;
            void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &u, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
            tick(h, 2, true, true);
            const hipError_t e = hipModuleLaunchKernel(h->m.user_kernel, pl.grid_x, pl.grid_y, 1, 256, 1, 1, 0, h->stream, nullptr, cfg);
            tick(h, 2, false, true);
            if (e != hipSuccess) return fail(h, DEMC_EHIP, std::string("hipModuleLaunchKernel: ") + hipGetErrorString(e));
        } break;
        case K2_HIER:
            tick(h, 2, true);
            LAUNCH_T(h, k_hier_loglike, grid, dim3(256), 0, k);
            tick(h, 2, false);
            break;
        default: break;  // (MvNormal in SUFFSTAT mode: K1 already formed S)
    }
    k.n_partials = pl.n_partials;  // (after the launch: K2's own kernarg says one plane, K3 reads them all)
    return DEMC_OK;
}

// the tail K1 carries (tail_flags), copied into the kernarg
void apply_tail(const demc_handle* h, KParams& k, const TailFlags& t) {
    k.fuse_prep = t.fuse_prep; k.prep_mfma = t.prep_mfma; k.fuse_obs = t.fuse_obs; k.fuse_accept = t.fuse_accept;
    k.write_prop = t.write_prop;
    k.sx = t.pass_sx ? h->m.sx : nullptr;
    k.Ainv = t.pass_ainv ? h->m.Ainv : nullptr;
}

// one launch in the K1 slot, inside its timing bracket; demc_last_kernels names the instance
void launch_k1(demc_handle* h, const K1Inst* e, unsigned grid, int wg, size_t lds, const KParams& k) {
    h->last = demc_handle::LastPlan{e};
    tick(h, 0, true);
    LAUNCH_T(h, e->fn, dim3(grid), dim3(wg), lds, k);
    tick(h, 0, false);
}

// The sweep-start snapshot into the proposal buffers (which a fused sweep does not use): the weights, and the rows -- whole, or
// the columns of the sweep's block only.
int take_snapshot(demc_handle* h, const KParams& k, bool block_only) {
    const demc_config& c = h->c;
    HIPCHK(hipMemcpyAsync(h->prop_prior, h->weight, sizeof(double) * (size_t)h->P, hipMemcpyDeviceToDevice, h->stream));
    if (!block_only) {
        HIPCHK(hipMemcpyAsync(h->prop, h->theta, sizeof(double) * (size_t)h->P * c.D, hipMemcpyDeviceToDevice, h->stream));
        return DEMC_OK;
    }
    for (int r = 0; r < k.n_mrun; ++r)  // the columns of the block: a strided copy per run of the mask (a few doubles per row)
        if ((k.mrun_in >> r) & 1u) {
            const int lo = k.mrun_start[r], hi = r + 1 < k.n_mrun ? k.mrun_start[r + 1] : c.D;
            HIPCHK(hipMemcpy2DAsync(h->prop + lo, sizeof(double) * (size_t)c.D, h->theta + lo, sizeof(double) * (size_t)c.D,
                                    sizeof(double) * (size_t)(hi - lo), (size_t)h->P, hipMemcpyDeviceToDevice, h->stream));
        }
    return DEMC_OK;
}

// whether two 256-thread workgroups of k_longrow with `lds` bytes of dynamic LDS are resident on a CU (asked once per row size)
int two_longrows_fit(demc_handle* h, size_t lds) {
    if (h->lr_two_lds != lds) {
        int nb = 0;
        const K1Inst* e256 = nullptr;
        PICK(e256, "k_longrow", kLongrow, 256);
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)e256->fn, 256, lds));
        h->lr_two_lds = lds;
        h->lr_two_fit = nb >= 2;
    }
    return DEMC_OK;
}

// One sweep and colour phase: the plan (demc_geometry.hpp: kernel, geometry, fuse flags, snapshot), the copies it names, the
// kernarg, the launch, and the by-product snapshot's bookkeeping.
// (`k` by value: the frozen-sweep / snapshot overrides below -- glist, base_*, snap_*, the fuse flags -- stay inside this launch;
// run_sweep reuses its own copy for the second colour phase and for every particle of the sequential schedule)
int launch_phase(demc_handle* h, KParams k) {
    if ((long long)k.n_groups * k.n_act == 0) return DEMC_OK;
    const demc_config& c = h->c;
    Phase p;
    p.n_groups = k.n_groups; p.a_lo = k.a_lo; p.n_act = k.n_act; p.pool_lo = k.pool_lo; p.pool_n = k.pool_n; p.mode = k.mode;
    p.iter = k.iter; p.sweep = (int)k.sweep; p.lpp = k.lpp; p.lpp3 = k.lpp3;
    p.tile_in_lds = k.tile_in_lds != 0; p.live = k.theta == h->theta;
    p.masked = k.mask != nullptr; p.n_mrun = k.n_mrun; p.mrun_in = k.mrun_in; p.mrun_start = k.mrun_start;
    p.snap2 = h->snap2.get() != nullptr; p.snap2_iter = h->snap2_iter; p.snap2_sweep = h->snap2_sweep;
    p.frozen_order = h->frozen.table.dev.get() != nullptr; p.frozen_iter0 = h->frozen.iter0; p.frozen_iters = h->frozen.iters;
    int rc_fit = DEMC_OK;
    const PhasePlan pl = plan_phase(setup_of(h), p, [&](size_t lds) { return (rc_fit = two_longrows_fit(h, lds)) == DEMC_OK && h->lr_two_fit; });
    if (rc_fit != DEMC_OK) return rc_fit;
    // the snapshot the base rows are read from
    if (pl.snap == SNAP_REUSE) {
        h->snap2_iter = -1;  // (used once: by the sweep it was written for, in the demc_step call that wrote it)
        k.base_theta = h->snap2; k.base_weight = h->snap2_w;
    } else if (pl.snap != SNAP_NONE) {
        k.base_theta = h->prop; k.base_weight = h->prop_prior;
        if (int rc = take_snapshot(h, k, pl.snap == SNAP_BLOCK)) return rc;
    }
    apply_tail(h, k, pl.t);
    k.n_split = pl.n_split; k.own_in_pool = pl.own_in_pool; k.tile_rows = pl.tile_rows; k.plan = pl.plan;
    if (pl.frozen_order)
        k.glist = h->frozen.table.dev + ((size_t)(k.iter - h->frozen.iter0) * c.n_blocks + k.sweep) * (size_t)c.n_groups;
    if (pl.write_snap2) {
        k.snap_theta = h->snap2; k.snap_weight = h->snap2_w;
        h->snap2_iter = (int64_t)k.iter; h->snap2_sweep = (int)k.sweep + 1;
    }
    const K1Inst* e = nullptr;
    switch (pl.kernel) {
        case K1_FROZEN: PICK(e, "k_frozen_sweep", kFrozen, 256, 3, 2, pl.big); break;
        case K1_LONGROW: PICK(e, "k_longrow", kLongrow, pl.wg); break;
        case K1_PROPOSE: PICK(e, "k_propose", kPropose, pl.wg, pl.tile, pl.tail, false, pl.lean); break;
    }
    launch_k1(h, e, (unsigned)pl.grid, pl.wg, pl.lds, k);
    if (!pl.chain) return DEMC_OK;
    int rc = launch_loglike(h, k);
    if (rc != DEMC_OK) return rc;
    h->last.k3 = true;
    tick(h, 3, true);
    LAUNCH_T(h, k_accept_store, dim3((unsigned)pl.k3_grid), dim3(256), 0, k);
    tick(h, 3, false);
    return DEMC_OK;
}

// ---- planning the whole-update forms: once per model (size_k1_lds), the lean ones again whenever the prior table changes ----
// The geometry comes from demc_geometry.hpp (plan_resident, plan_stream, plan_lean); here the instances it names are resolved
// and the plan is stored.

int set_resident_form(demc_handle* h) {
    FormPlan& f = h->form[FORM_RESIDENT];
    f = FormPlan();
    const FormGeo g = plan_resident(setup_of(h));
    if (!g.ok) return DEMC_OK;
    for (int lean = 0; lean < 3; ++lean) PICK(f.k1[lean], "k_propose", kPropose, g.wg, true, g.tail, true, lean);
    static_cast<FormGeo&>(f) = g;
    return DEMC_OK;
}

// the stream geometry (h->st) and FORM_STREAM, the general kernel around it.  Nothing is allocated here: alloc_stream follows.
int set_stream_form(demc_handle* h) {
    FormPlan& f = h->form[FORM_STREAM];
    f = FormPlan();
    static_cast<StreamDims&>(h->st) = StreamDims();
    const StreamPlan p = plan_stream(setup_of(h));
    if (p.form.ok) {
        for (int lean = 0; lean < 3; ++lean) PICK(f.k1[lean], "k_propose", kPropose, p.form.wg, true, p.form.tail, true, lean, true);
        static_cast<FormGeo&>(f) = p.form;
    }
    static_cast<StreamDims&>(h->st) = p.dims;
    return DEMC_OK;
}

size_t granule_bytes(const demc_handle* h) { return 2 * (size_t)h->c.n_groups * h->st.C * h->st.nact_max * 2 * sizeof(unsigned long long); }

// The buffers the stream geometry asks for: the hand-over granules and the time-out word.  No memory for them means no streaming
// form, not an error (the per-phase chain serves).
void alloc_stream(demc_handle* h) {
    StreamGeo& g = h->st;
    if (!g.ok) return;
    g.ok = g.gran.alloc(granule_bytes(h) / sizeof(unsigned long long)) == hipSuccess;
    if (g.ok && !g.err) {
        g.ok = g.err.alloc(1, hipHostMallocMapped) == hipSuccess;
        if (g.ok) *g.err.get() = 0u;
    }
    if (!g.ok) h->form[FORM_STREAM].ok = false;
}

// The lean resident kernels of the default sampler: the plan follows the prior table (upload_dimtab); it reads set_resident_form's
// and set_stream_form's results and touches no device memory.
int set_lean_forms(demc_handle* h) {
    const Form lean_forms[] = {FORM_LEAN_SUFFSTAT, FORM_LEAN_STREAMING, FORM_LEAN_DIRECT, FORM_LEAN_OBS, FORM_LEAN_Z};
    for (Form f : lean_forms) h->form[f] = FormPlan();
    const LeanPlan p = plan_lean(setup_of(h), h->form[FORM_RESIDENT].ok, h->st, (size_t)kLogPhiRows * kLogPhiRow);
    if (p.form[FORM_LEAN_OBS].ok) PICK(h->form[FORM_LEAN_OBS].k1[0], "k_res_obs", kResObs, 256);
    if (const FormGeo& g = p.form[FORM_LEAN_Z]; g.ok)
        for (int hist = 1; hist <= 3; ++hist) PICK(h->form[FORM_LEAN_Z].k1[hist - 1], "k_res_mvn", kResMvn, g.wg, false, p.dt, hist, 1, p.iso);
    if (const FormGeo& g = p.form[FORM_LEAN_SUFFSTAT]; g.ok) PICK(h->form[FORM_LEAN_SUFFSTAT].k1[0], "k_res_mvn", kResMvn, g.wg, false, p.dt, 0, 1);
    for (Form f : {FORM_LEAN_STREAMING, FORM_LEAN_DIRECT})
        if (const FormGeo& g = p.form[f]; g.ok) PICK(h->form[f].k1[0], "k_res_mvn", kResMvn, g.wg, true, p.dt, 0, 1, false, f == FORM_LEAN_DIRECT);
    for (Form f : lean_forms) static_cast<FormGeo&>(h->form[f]) = p.form[f];
    return DEMC_OK;
}

// ---- launching a form (which one: choose_form, demc_geometry.hpp) ----

// the kernarg fields of the observation stream (st_rows, the general kernel's scratch rows, apart), and its granules reset
int stream_fields(demc_handle* h, KParams& k) {
    const StreamGeo& g = h->st;
    k.st_C = g.C; k.st_nact_max = g.nact_max; k.st_x_lds = g.x_lds; k.st_chunk_tiles = g.chunk_tiles;
    k.n_tiles = h->m.n_tiles; k.Xf = h->m.Xf; k.st_gran = g.gran; k.st_err = g.err;
    // Every workgroup of this grid must be resident at once (the workgroups of a group spin on each other's progress).  The
    // grid is sized for that by construction -- at most one workgroup per CU (plan_stream: n_groups * C <= CUs, and each
    // takes most of a CU's LDS) -- so a plain launch has the same residency as a cooperative one, without its launch-time
    // cost (+15-19 us, MI355X_MICROARCH.md "coop-launch"); every spin in the kernel is bounded regardless.
    if (k.n_groups * g.C > h->n_cus) return fail(h, DEMC_EINVAL, "streaming-resident grid exceeds what is resident at once");
    // epoch tags restart at 1 in every launch: the granules of the previous launch must not match them
    HIPCHK(hipMemsetAsync(g.gran, 0, granule_bytes(h), h->stream));
    return DEMC_OK;
}

// iterations [iter0, iter0 + n_iters) of every group (of the subset in force) in ONE launch of `form` (any but FORM_PHASE)
int launch_form(demc_handle* h, Form form, long long iter0, int n_iters) {
    const demc_config& c = h->c;
    const FormPlan& f = h->form[form];
    KParams k = base_params(h);
    k.iter = iter0; k.n_iters = n_iters; k.n_rows = h->hist ? c.n_rows : 0;
    const K1Inst* e = f.k1[0];
    if (form == FORM_RESIDENT || form == FORM_STREAM) {  // the general kernel: K1's own parameters, the tile being the whole group
        k.lpp = f.lpp;
        apply_tail(h, k, tail_flags(setup_of(h), k.lpp, k.mode, k.iter));
        k.n_sweeps = c.n_blocks > 0 ? c.n_blocks : 1;
        k.mask = c.n_blocks > 0 ? h->masks : nullptr;
        k.n_split = 1; k.exclude_self = 0; k.own_in_pool = 1; k.tile_rows = c.Np; k.tile_in_lds = 1;
        k.scr_doubles = f.scr_doubles;
        k.plan = (k.lpp >= 4) ? 1 : 0;
        if (form == FORM_STREAM) {  // STREAMING: the cross term comes from the tiles
            k.sx = nullptr; k.fuse_accept = 1; k.write_prop = k.trace ? 1 : 0;
            k.st_rows = h->st.rows;
        }
        e = f.k1[lean_level(c, h->rp.active, DEMC_PARTNER_CURRENT)];
    } else if (form == FORM_LEAN_SUFFSTAT || form == FORM_LEAN_Z)
        k.sx = h->m.sx;
    if (form == FORM_LEAN_Z) {
        // (the HIST instances hold back the first half's stores for ONE iteration's store_row and form the cdf once per launch: the
        // precondition is checked here, and again by the kernel -- its phase loop runs no trip for any other count)
        if (n_iters != 1) return fail(h, DEMC_EINVAL, "lean DE-MC_Z kernel: one iteration per launch");
        e = f.k1[lean_level(c, h->rp.active, DEMC_PARTNER_HISTORY) == 2 ? 2 : iter0 <= c.burnin ? 1 : 0];
    }
    unsigned grid = (unsigned)k.n_groups;
    if (spin_waiting(form)) {
        if (int rc = stream_fields(h, k)) return rc;
        grid *= (unsigned)h->st.C;
    }
    launch_k1(h, e, grid, f.wg, f.lds, k);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(h, DEMC_EHIP, e->name(e->key) + " launch: " + hipGetErrorString(err));
    return DEMC_OK;
}

// one sweep of every group: mutate_or_crossover! for all groups (main.jl:161-167, 199-207)
int run_sweep(demc_handle* h, long long iter, unsigned sweep, const unsigned char* mask, long long store_row) {
    KParams k = base_params(h);
    k.iter = iter; k.sweep = sweep; k.mask = mask; k.store_row = store_row;
    if (mask && sweep < h->mask_runs.size()) {
        const auto& mr = h->mask_runs[sweep];
        k.n_mrun = mr.n; k.mrun_in = mr.in;
        std::memcpy(k.mrun_start, mr.start, sizeof k.mrun_start);
    } else if (mask)
        k.n_mrun = 0;
    for (int i = 0, n = n_colour_phases(h->c); i < n; ++i) {  // who moves against whom: colour_phase, demc_schedule.hpp
        const ColourPhase ph = colour_phase(h->c, i);
        k.a_lo = ph.a_lo; k.n_act = ph.n_act; k.pool_lo = ph.pool_lo; k.pool_n = ph.pool_n; k.exclude_self = ph.exclude_self;
        if (int rc = launch_phase(h, k)) return rc;
    }
    return DEMC_OK;
}

int migration_enqueue(demc_handle* h, long long iter, double* dev_rows, const double* dev_all_rows, bool pack, bool apply) {
    KParams k = base_params(h);
    k.iter = iter;
    tick(h, 4, true);
    if (pack)
        LAUNCH_T(h, k_mig_pack, dim3(h->c.n_groups), dim3(256),
                           sizeof(double) * ((size_t)h->c.Np + ((size_t)h->c.Np + 15) / 16), k, dev_rows);
    if (apply) {
        const int ngt = h->c.n_groups_total;
        const int grid = ngt < 64 ? ngt : 64;
        LAUNCH_T(h, k_mig_apply, dim3(grid), dim3(256), 2 * sizeof(int) * (size_t)ngt, k, dev_all_rows, ngt);
    }
    tick(h, 4, false);
    return DEMC_OK;
}

int evaluate_rows(demc_handle* h, double* theta_dev, double* weight_dev) {
    // init_particle: evaluate_fitness! on the current rows (utilities.jl:13-22) -- identity proposal, forced accept
    KParams k = base_params(h);
    k.mode = MODE_IDENT; k.theta = theta_dev; k.weight = weight_dev; k.store_row = -1; k.iter = 0;
    k.tile_in_lds = 0;
    return launch_phase(h, k);
}

// The by-product snapshot (KParams::snap_theta / snap_weight: a frozen sweep over the whole population leaves the rows it streamed
// behind as the NEXT sweep's sweep-start snapshot) costs another P x D doubles -- 328 MB at cfg4, the size of theta itself.  The
// buffers exist exactly while the configuration can take that path (DE-MC_Z inside burn-in, long hierarchical rows, more than one
// block, enough particles for the row-streaming kernel): allocated here, when demc_set_model / demc_set_blocks learn it -- not by a
// hipMalloc in the middle of an enqueued step -- and freed when the model or the blocks change so that it no longer can.  Out of
// memory is not an error (the sweeps copy the population instead); demc_last_error then says so.
int plan_snap2(demc_handle* h) {
    const demc_config& c = h->c;
    if (!snap2_wanted(setup_of(h))) {
        if (h->snap2 || h->snap2_w) {
            HIPCHK(hipStreamSynchronize(h->stream));
            h->snap2.reset(); h->snap2_w.reset(); h->snap2_iter = -1;
        }
        return DEMC_OK;
    }
    if (h->snap2) return DEMC_OK;
    const size_t bytes = sizeof(double) * (size_t)h->P * c.D;
    if (h->snap2.alloc((size_t)h->P * c.D) != hipSuccess) (void)hipGetLastError();
    if (h->snap2 && h->snap2_w.alloc((size_t)h->P) != hipSuccess) {
        h->snap2.reset(); (void)hipGetLastError();
    }
    if (!h->snap2)
        h->err = "note: no memory for the by-product snapshot (" + std::to_string(bytes) + " bytes): DE-MC_Z sweeps inside burn-in copy the population instead";
    return DEMC_OK;
}

// every instance of a table may ask for the whole dynamic-LDS budget
template <typename I, size_t N>
int raise_dyn_lds(demc_handle* h, const I (&tab)[N]) {
    for (const I& e : tab) HIPCHK(hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxDynLds));
    return DEMC_OK;
}

// K1 LDS carve-up (carve_k1_lds, demc_geometry.hpp), the dynamic-LDS ceiling of every kernel that may ask for it, and the plans of
// the whole-update forms
int size_k1_lds(demc_handle* h) {
    if (Refusal r = carve_k1_lds(h->m.family, h->m.d, h->c.Np, h->c.D, h->lpp, h->k1)) return fail(h, r);
    // the attribute is per function, not per handle: always raise it to the same ceiling so that handles of different
    // sizes in one process do not lower each other's limit
    if (int rc = raise_dyn_lds(h, kPropose)) return rc;
    if (int rc = raise_dyn_lds(h, kLongrow)) return rc;
    if (int rc = raise_dyn_lds(h, kResMvn)) return rc;
    if (int rc = raise_dyn_lds(h, kResObs)) return rc;
    if (int rc = raise_dyn_lds(h, kSim)) return rc;
    if (int rc = raise_dyn_lds(h, kOde)) return rc;
    // the whole-update forms.  Decide, then allocate: the plans compute geometry only, the stream's buffers follow once it is known
    if (int rc = set_resident_form(h)) return rc;
    if (int rc = set_stream_form(h)) return rc;
    alloc_stream(h);
    if (int rc = set_lean_forms(h)) return rc;
    HIPCHK(hipFuncSetAttribute((const void*)k_mig_pack, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxDynLds));
    return plan_snap2(h);
}

// The one place a model is released: nothing on the stream may still read it, then every buffer, the JIT module and every
// field go with the record.  What a REFUSED set-model call leaves behind differs by entry point and is kept as it was:
// demc_set_model_sim validates everything first, so a refusal leaves the previous model in force; demc_set_model and the source
// entry points release first (after their checks of the call's shape), so a refusal past that point leaves no model.
int clear_model(demc_handle* h) {
    HIPCHK(hipStreamSynchronize(h->stream));
    h->m = Model{};
    return DEMC_OK;
}

// hiprtc: `src` compiled for the library's architecture, loaded, and its kernel `entry` looked up.  `what` names the text in the
// message of a source that does not compile (the log follows it).
template <size_t NOPT>
int compile_module(demc_handle* h, const std::string& src, const char* file, const char* (&opts)[NOPT], const char* what,
                   const char* entry, Module& mod, hipFunction_t* fn) {
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), file, 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return fail(h, DEMC_EHIP, "hiprtcCreateProgram failed");
    const hiprtcResult cr = hiprtcCompileProgram(prog, (int)NOPT, opts);
    if (cr != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls, '\0');
        if (ls) hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        return fail(h, DEMC_EINVAL, std::string(what) + " does not compile: " + hiprtcGetErrorString(cr) + "\n" + log);
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    std::vector<char> code(cs);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    HIPCHK(mod.load(code.data()));
    HIPCHK(hipModuleGetFunction(fn, mod, entry));
    return DEMC_OK;
}

}  // namespace

extern "C" {

static int upload_dimtab(demc_handle* h);  // (defined next to demc_set_priors)

int32_t demc_version(void) { return DEMC_VERSION; }

const char* demc_last_error(demc_handle* h) { return h ? h->err.c_str() : "null handle"; }

int32_t demc_create(const demc_config* cfg, demc_handle** out) {
    if (!cfg || !out) return DEMC_EINVAL;
    *out = nullptr;
    demc_handle* h = new (std::nothrow) demc_handle();
    if (!h) return DEMC_ENOMEM;
    *out = h;  // returned even on failure so that demc_last_error() can be read; caller destroys it
    return guarded(h, [&]() -> int32_t {
    h->c = *cfg;
    demc_config& c = h->c;
    if (c.n_groups < 1 || c.Np < 3 || c.D < 1 || c.n_rows < 0)
        return fail(h, DEMC_EINVAL, "need n_groups >= 1, Np >= 3 (structs.jl:43), D >= 1, n_rows >= 0");
    if (c.n_groups_total <= 0) c.n_groups_total = c.n_groups;
    if (c.n_groups_total == 1) c.alpha = 0.0;  // structs.jl:102-105
    if (c.schedule != DEMC_SCHED_SEQUENTIAL && c.schedule != DEMC_SCHED_SYNCHRONOUS && c.schedule != DEMC_SCHED_TWO_COLOUR)
        return fail(h, DEMC_EINVAL, "unknown schedule");
    if (c.geometry_groups < 0) return fail(h, DEMC_EINVAL, "geometry_groups < 0");
    if (c.loglike_mode < DEMC_LOGLIKE_STREAMING || c.loglike_mode > DEMC_LOGLIKE_DIRECT) return fail(h, DEMC_EINVAL, "unknown loglike_mode");
    h->geo_groups = c.geometry_groups > 0 ? c.geometry_groups : c.n_groups;
    if (c.schedule == DEMC_SCHED_TWO_COLOUR && c.partner_kind == DEMC_PARTNER_CURRENT) {
        const int need = c.theta_snooker > 0.0 ? 6 : 4;
        if (c.Np < need) return fail(h, DEMC_EINVAL, "two_colour needs Np >= 4 (>= 6 with snooker)");
    }
    if (c.proposal_kind < 0 || c.proposal_kind > 2 || c.partner_kind < 0 || c.partner_kind > 1 || c.update_kind < 0 ||
        c.update_kind > 2 || c.fitness_kind < 0 || c.fitness_kind > 1)
        return fail(h, DEMC_EUNSUPPORTED, "hook outside the registered set (structs.jl:71-74): no fallback");
    if (c.partner_kind == DEMC_PARTNER_HISTORY && (!c.store_history || c.n_initial < 1))
        return fail(h, DEMC_EINVAL, "history partners (resample) need store_history and n_initial > 0");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(h, DEMC_EHIP, "no HIP device visible");
    HIPCHK(hipSetDevice(c.device_id));
    HIPCHK(hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, c.device_id));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    h->P = (long long)c.n_groups * c.Np;
    const size_t P = (size_t)h->P, D = (size_t)c.D;
    ALLOC(h->theta, P * D); ALLOC(h->weight, P); ALLOC(h->id, P); ALLOC(h->prop, P * D);
    ALLOC(h->prop_prior, P); ALLOC(h->prop_adj, P); ALLOC(h->prop_oob, P);
    ALLOC(h->tr_idx, P * 4); ALLOC(h->tr_w, P); ALLOC(h->tr_acc, P);
    ALLOC(h->partial, (size_t)h->partial_cap * P); ALLOC(h->aux, P);
    ALLOC(h->dimtab, D);
    ALLOC(h->dimseg, (size_t)kMaxDimSeg);
    for (StagedList<int>& s : h->glist.slot) {  // the ring's buffers are sized here, once, for a list of every group
        int* host = nullptr;
        const hipError_t e = s.stage((size_t)c.n_groups, h->stream, &host);
        if (e != hipSuccess && s.ev && !s.dev) return fail(h, DEMC_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));  // (as ALLOC reports it)
        HIPCHK(e);
    }
    ALLOC(h->mig_rows, (size_t)c.n_groups_total * (D + 3));
    ALLOC(h->scratch_theta, P * D); ALLOC(h->scratch_w, P);
    if (c.store_history && c.n_rows > 0) {
        // (cells that partners are gathered from are padded to whole cache lines: history_cell_stride)
        h->hist_ld = history_cell_stride(D, c.partner_kind);
        ALLOC(h->hist, (size_t)c.n_rows * P * (size_t)h->hist_ld);
        ALLOC(h->acc_hist, (size_t)c.n_rows * P);
        ALLOC(h->lp_hist, (size_t)c.n_rows * P);
        ALLOC(h->id_hist, (size_t)c.n_rows * P);
    }
    {
        DimTab t0;
        t0.lo = -INFINITY; t0.hi = INFINITY; t0.a = 0.0; t0.b = 1.0; t0.c = 0.0; t0.kind = PR_FLAT; t0.ref = 0;
        h->h_tab.assign(D, t0);
        int rc_tab = upload_dimtab(h);
        if (rc_tab != DEMC_OK) return rc_tab;
        std::vector<long long> id(P);
        for (size_t s = 0; s < P; ++s) id[s] = (long long)c.group_offset * c.Np + (long long)s;
        HIPCHK(hipMemcpy(h->id, id.data(), P * sizeof(long long), hipMemcpyHostToDevice));
        if (h->id_hist) {
            std::vector<int> row(P);
            for (size_t s = 0; s < P; ++s) row[s] = (int)id[s];
            for (long long r = 0; r < c.n_rows; ++r)
                HIPCHK(hipMemcpy(h->id_hist + (size_t)r * P, row.data(), P * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    h->lpp = lanes_per_particle(c.D, c.Np, c.schedule, h->geo_groups);  // (the rule and what it was measured on: demc_geometry.hpp)
    int rc_lds = size_k1_lds(h);
    if (rc_lds != DEMC_OK) return rc_lds;
    if (2 * (size_t)c.n_groups_total * sizeof(int) > 48 * 1024) return fail(h, DEMC_EINVAL, "n_groups_total too large");
    // A documented deviation says so at run time: `resample` draws its partner cells from the history of ALL
    // particles (crossover.jl:116-124); a shard holds the history of its own groups only.  Not an error -- SURVEY 8(e) allows the
    // shard-local pool -- but the caller is told: demc_last_error() carries the note after a successful demc_create.
    if (c.partner_kind == DEMC_PARTNER_HISTORY && c.n_groups_total > c.n_groups)
        h->err = "note: sharded handle (" + std::to_string(c.n_groups) + " of " + std::to_string(c.n_groups_total) +
                 " groups) with history partners: DE-MC_Z draws its partner cells from THIS shard's history only "
                 "(the reference draws from all particles, crossover.jl:116-124)";
    return DEMC_OK;
    });
}

int32_t demc_destroy(demc_handle* h) {
    return guarded(nullptr, [&]() -> int32_t {
    if (!h) return DEMC_OK;
    if (h->multi) return DEMC_EINVAL;  // a shard of a multi-GPU set goes with the set (demc_destroy_multi)
    if (h->stream) hipStreamSynchronize(h->stream);
    drain_events(h);
    for (hipEvent_t e : h->event_pool) hipEventDestroy(e);
    h->event_pool.clear();
    if (h->side) hipStreamSynchronize(h->side);
    if (h->comm && h->own_comm) ncclCommDestroy(h->comm);
    if (h->side) hipStreamDestroy(h->side);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;  // every buffer, event and module goes with its owner (demc_devmem.hpp)
    return DEMC_OK;
    });
}

int32_t demc_set_stream(demc_handle* h, void* hip_stream) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    // a shard of a demc_multi set: shards on one device run on the first such shard's stream (demc_create_multi); a caller who
    // re-points one would either destroy a stream its borrowers still hold or put two spinning resident kernels in flight at once
    if (h->multi && h->multi_sealed) return fail(h, DEMC_EINVAL, "demc_set_stream: the streams of a demc_multi set belong to the set");
    USE_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    h->own_stream = false;
    if (hip_stream)
        h->stream = (hipStream_t)hip_stream;
    else {
        HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return DEMC_OK;
    });
}

int32_t demc_set_model(demc_handle* h, int32_t family, const double* data, const int64_t* dims, int32_t ndims,
                       const double* hyper, int32_t nhyper) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (ndims < 0 || ndims > 4 || (ndims > 0 && !dims)) return fail(h, DEMC_EINVAL, "bad dims");
    if (int rc = clear_model(h)) return rc;
    const PreparedModel pm = prepare_model(family, h->c.D, h->c.loglike_mode, data, dims, ndims, hyper, nhyper);
    if (pm.refused) return fail(h, pm.refused);
    Model& m = h->m;
    static_cast<ModelShape&>(m) = pm;
    if (int rc = upload(h, m.Ainv, pm.M)) return rc;
    if (int rc = upload(h, m.sx, pm.sx)) return rc;
    if (int rc = upload(h, m.xbar, pm.xbar)) return rc;
    if (is_mvn(family)) ALLOC(m.Ypad, (size_t)h->P * m.dpad);
    if (int rc = upload(h, m.Xf, pm.Xf)) return rc;
    if (int rc = upload(h, m.data, pm.data)) return rc;
    if (!pm.order.empty()) {
        ALLOC(m.order, pm.order.size());
        HIPCHK(hipMemcpy(m.order, pm.order.data(), sizeof(int) * pm.order.size(), hipMemcpyHostToDevice));
    }
    m.family = family;
    return size_k1_lds(h);
    });
}

static int32_t set_model_source_impl(demc_handle* h, const char* hip_source, const double* data, const int64_t* dims, int32_t ndims,
                                     const double* hyper, int32_t nhyper, bool row, bool has_prior) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !hip_source) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (ndims < 1 || ndims > 8 || !dims || dims[0] < 1 || !data) return fail(h, DEMC_EINVAL, "user model: dims[0] = number of observations, data required");
    long long n_data = 1;
    for (int i = 0; i < ndims; ++i) n_data *= dims[i];
    if (n_data < 1) return fail(h, DEMC_EINVAL, "user model: empty data");
    if (int rc = clear_model(h)) return rc;
    h->m.user_row = row; h->m.user_has_prior = row && has_prior; h->m.user_ndims = ndims;
    // compile: kernarg struct + declarations + user source + kernel, for gfx950
    const std::string src = std::string(row && has_prior ? "#define DEMC_USER_HAS_PRIOR 1\n" : "") + kUserStruct +
                            (row ? kUserRowPrologue : kUserPrologue) + hip_source + (row ? kUserRowKernel : kUserKernel);
    const char* opts[] = {"--offload-arch=" DEMC_ARCH_STR, "-O3", "-std=c++17"};
    if (int rc = compile_module(h, src, "demc_user_model.hip", opts, "user model", row ? "k_user_row" : "k_user_loglike", h->m.user_module, &h->m.user_kernel))
        return rc;
    h->m.N = dims[0];
    ALLOC(h->m.data, (size_t)n_data);
    HIPCHK(hipMemcpy(h->m.data, data, sizeof(double) * (size_t)n_data, hipMemcpyHostToDevice));
    {
        long long dm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < ndims; ++i) dm[i] = dims[i];
        ALLOC(h->m.user_dims, (size_t)8);
        HIPCHK(hipMemcpy(h->m.user_dims, dm, sizeof dm, hipMemcpyHostToDevice));
    }
    h->m.user_nhyper = nhyper > 0 ? nhyper : 0;
    if (h->m.user_nhyper) {
        if (!hyper) return fail(h, DEMC_EINVAL, "user model: nhyper > 0 without hyper");
        ALLOC(h->m.user_hyper, (size_t)h->m.user_nhyper);
        HIPCHK(hipMemcpy(h->m.user_hyper, hyper, sizeof(double) * (size_t)h->m.user_nhyper, hipMemcpyHostToDevice));
    }
    h->m.family = FAM_USER;
    return size_k1_lds(h);
    });
}

int32_t demc_set_model_source(demc_handle* h, const char* hip_source, const double* data, const int64_t* dims, int32_t ndims,
                              const double* hyper, int32_t nhyper) {
    return set_model_source_impl(h, hip_source, data, dims, ndims, hyper, nhyper, false, false);
}

int32_t demc_set_model_source_row(demc_handle* h, const char* hip_source, const double* data, const int64_t* dims, int32_t ndims,
                                  const double* hyper, int32_t nhyper, int32_t flags) {
    if (flags & ~DEMC_USER_HAS_PRIOR) return h ? fail(h, DEMC_EINVAL, "unknown flag") : DEMC_EINVAL;
    return set_model_source_impl(h, hip_source, data, dims, ndims, hyper, nhyper, true, (flags & DEMC_USER_HAS_PRIOR) != 0);
}

// Simulation-based likelihood (demc_simlike.hpp).  hyper[0] = the KDE bandwidth (<= 0 or absent: the rule of thumb), hyper[1..] the
// simulator's own hyper-parameters.  DEMC_SIMEST_KDE_CHOICE: data = the n_obs choices, then the n_obs response times.
int32_t demc_set_model_sim(demc_handle* h, int32_t simulator, int32_t estimator, int64_t n_sim, const char* hip_source,
                           const double* data, int64_t n_obs, const double* hyper, int32_t nhyper) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    static_assert(sim_choice_lds(kSimChoiceMaxN) <= kMaxDynLds && sim_choice_lds(10000) <= kMaxDynLds, "k_sim_choice: the cap does not fit the LDS of a launch");
    const PreparedSim ps = prepare_sim(h->c.D, simulator, estimator, n_sim, hip_source, data, n_obs, hyper, nhyper);
    if (ps.refused) return fail(h, ps.refused);
    if (int rc = clear_model(h)) return rc;
    if (simulator == DEMC_SIM_USER) {
        // the one kernel text (demc_simlike.hpp) with n_sim and the estimator compiled in, the user's function behind it
        const std::string src = "#define DEMC_SIM_JIT 1\n#define DEMC_SIM_JIT_N " + std::to_string(n_sim) + "\n#define DEMC_SIM_JIT_EST " +
                                std::to_string(estimator) + "\n" + kSimKernelSource + "\n" + hip_source + "\n";
        const char* opts[] = {"--offload-arch=" DEMC_ARCH_STR, "-O3", "-std=c++17", "-ffp-contract=off"};
        if (int rc = compile_module(h, src, "demc_user_sim.hip", opts, "user simulator", "k_sim_loglike_user", h->m.user_module, &h->m.user_kernel))
            return rc;
    }
    h->m.N = n_obs;
    const size_t n_data = (size_t)n_obs * (estimator == DEMC_SIMEST_KDE_CHOICE ? 2 : 1);
    ALLOC(h->m.data, n_data);
    HIPCHK(hipMemcpy(h->m.data, data, sizeof(double) * n_data, hipMemcpyHostToDevice));
    h->m.sim_kmax = ps.kmax;
    h->m.user_nhyper = (int)ps.hyper.size();
    if (int rc = upload(h, h->m.user_hyper, ps.hyper)) return rc;
    h->m.sim_bw = ps.sim_bw;
    if (int rc = upload(h, h->m.sim_logtab, ps.logtab)) return rc;
    h->m.sim_kind = simulator; h->m.sim_est = estimator; h->m.sim_n = (int)n_sim;
    h->m.family = FAM_SIM;
    return size_k1_lds(h);
    });
}

static int upload_dimtab(demc_handle* h) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->dimtab, h->h_tab.data(), (size_t)h->c.D * sizeof(DimTab), hipMemcpyHostToDevice));
    const SegTable st = encode_segments(h->h_tab);
    h->n_seg = st.n_seg;
    h->normal_ref = has_normal_ref(h->h_tab);
    std::memcpy(h->seg_start, st.seg_start, sizeof h->seg_start);
    h->seg_plain = st.seg_plain;
    HIPCHK(hipMemcpy(h->dimseg, st.segs, sizeof st.segs, hipMemcpyHostToDevice));
    // the lean resident kernel reads the table in its run-length form and knows no Normal(a, theta[ref]) prior: priors and
    // bounds arrive AFTER demc_set_model in every caller, so its plan is taken again whenever the table changes
    return h->m.family >= 0 ? set_lean_forms(h) : DEMC_OK;
}

int32_t demc_set_priors(demc_handle* h, const int32_t* kind, const double* a, const double* b, const int32_t* ref) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !kind) return DEMC_EINVAL;
    USE_DEVICE(h);
    // (checked against the bounds in force before anything is stored: a refused call leaves the table as it was)
    if (Refusal r = prepare_priors(h->h_tab, h->trunc_sd, kind, a, b, ref)) return fail(h, r);
    return upload_dimtab(h);
    });
}

int32_t demc_set_bounds(demc_handle* h, const double* lo, const double* hi) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !lo || !hi) return DEMC_EINVAL;
    USE_DEVICE(h);
    // (checked first: a refused call leaves the table as it was)
    if (Refusal r = prepare_bounds(h->h_tab, h->trunc_sd, lo, hi)) return fail(h, r);
    return upload_dimtab(h);
    });
}

int32_t demc_set_blocks(demc_handle* h, const uint8_t* masks, int32_t n_blocks) {
    return guarded(h, [&]() -> int32_t {
    if (!h || n_blocks < 0 || (n_blocks > 0 && !masks)) return DEMC_EINVAL;
    USE_DEVICE(h);
    h->masks.reset();
    h->c.n_blocks = n_blocks;
    if (n_blocks > 0) {
        ALLOC(h->masks, (size_t)n_blocks * h->c.D);
        HIPCHK(hipMemcpy(h->masks, masks, (size_t)n_blocks * h->c.D, hipMemcpyHostToDevice));
    }
    h->mask_runs.clear();
    for (int b = 0; b < n_blocks; ++b) h->mask_runs.push_back(encode_mask(masks + (size_t)b * h->c.D, h->c.D));
    return plan_snap2(h);
    });
}

int32_t demc_set_state(demc_handle* h, const double* theta, const double* weight, const int64_t* id) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !theta) return DEMC_EINVAL;
    USE_DEVICE(h);
    const size_t P = (size_t)h->P, D = (size_t)h->c.D;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->theta, theta, P * D * sizeof(double), hipMemcpyHostToDevice));
    if (id) HIPCHK(hipMemcpy(h->id, id, P * sizeof(long long), hipMemcpyHostToDevice));
    if (weight)
        HIPCHK(hipMemcpy(h->weight, weight, P * sizeof(double), hipMemcpyHostToDevice));
    else {
        if (h->m.family < 0) return fail(h, DEMC_EINVAL, "demc_set_model before demc_set_state(weight = NULL)");
        int rc = evaluate_rows(h, h->theta, h->weight);
        if (rc != DEMC_OK) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipGetLastError());
    }
    return DEMC_OK;
    });
}

int32_t demc_get_state(demc_handle* h, double* theta, double* weight, int64_t* id) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    const size_t P = (size_t)h->P, D = (size_t)h->c.D;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (theta) HIPCHK(hipMemcpy(theta, h->theta, P * D * sizeof(double), hipMemcpyDeviceToHost));
    if (weight) HIPCHK(hipMemcpy(weight, h->weight, P * sizeof(double), hipMemcpyDeviceToHost));
    if (id) HIPCHK(hipMemcpy(id, h->id, P * sizeof(long long), hipMemcpyDeviceToHost));
    return DEMC_OK;
    });
}

int32_t demc_set_history_rows(demc_handle* h, int64_t row0, int64_t nrows, const double* rows) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !rows) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (!h->hist) return fail(h, DEMC_EINVAL, kHistoryNotStored);
    if (row0 < 0 || nrows < 0 || row0 + nrows > h->c.n_rows) return fail(h, DEMC_EINVAL, "history rows out of range");
    const size_t D = (size_t)h->c.D, ld = (size_t)h->hist_ld, P = (size_t)h->P;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (ld == D) {
        HIPCHK(hipMemcpy(h->hist + (size_t)row0 * P * D, rows, (size_t)nrows * P * D * sizeof(double), hipMemcpyHostToDevice));
        return DEMC_OK;
    }
    // padded cells: the caller's dense rows go through a device staging buffer, a few rows at a time
    const size_t chunk = history_stage_rows(P, D);
    DevBuf<double> stage;
    ALLOC(stage, std::min<size_t>(chunk, (size_t)nrows) * P * D);
    for (size_t r = 0; r < (size_t)nrows; r += chunk) {
        const size_t n = std::min(chunk, (size_t)nrows - r);
        if (hipMemcpy(stage, rows + r * P * D, n * P * D * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(h, DEMC_EHIP, "history upload");
        hipLaunchKernelGGL(k_hist_repack, dim3(1024), dim3(256), 0, h->stream, h->hist + ((size_t)row0 + r) * P * ld, stage.get(), (long long)(n * P), (int)D,
                           (int)ld, (int)D);
        if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, DEMC_EHIP, "history repack");
    }
    return DEMC_OK;
    });
}

int32_t demc_get_history(demc_handle* h, int64_t row0, int64_t row1, double* th, uint8_t* acc, double* lp, int64_t* idh) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (!h->hist) return fail(h, DEMC_EINVAL, kHistoryNotStored);
    if (row0 < 0 || row1 < row0 || row1 > h->c.n_rows) return fail(h, DEMC_EINVAL, "history rows out of range");
    const size_t P = (size_t)h->P, D = (size_t)h->c.D, n = (size_t)(row1 - row0);
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t ld = (size_t)h->hist_ld;
    if (th && ld == D) HIPCHK(hipMemcpy(th, h->hist + (size_t)row0 * P * D, n * P * D * sizeof(double), hipMemcpyDeviceToHost));
    else if (th && n > 0) {  // padded cells: packed into a dense staging buffer on the device, a few rows at a time
        const size_t chunk = history_stage_rows(P, D);
        DevBuf<double> stage;
        ALLOC(stage, std::min(chunk, n) * P * D);
        for (size_t r = 0; r < n; r += chunk) {
            const size_t m = std::min(chunk, n - r);
            hipLaunchKernelGGL(k_hist_repack, dim3(1024), dim3(256), 0, h->stream, stage.get(), h->hist + ((size_t)row0 + r) * P * ld, (long long)(m * P), (int)D,
                               (int)D, (int)ld);
            if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, DEMC_EHIP, "history repack");
            if (hipMemcpy(th + r * P * D, stage, m * P * D * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(h, DEMC_EHIP, "history download");
        }
    }
    if (acc) HIPCHK(hipMemcpy(acc, h->acc_hist + (size_t)row0 * P, n * P, hipMemcpyDeviceToHost));
    if (lp) HIPCHK(hipMemcpy(lp, h->lp_hist + (size_t)row0 * P, n * P * sizeof(double), hipMemcpyDeviceToHost));
    if (idh) {
        std::vector<int> tmp(n * P);
        HIPCHK(hipMemcpy(tmp.data(), h->id_hist + (size_t)row0 * P, n * P * sizeof(int), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n * P; ++i) idh[i] = tmp[i];
    }
    return DEMC_OK;
    });
}

int32_t demc_export_chains(demc_handle* h, int64_t row0, int64_t row1, int32_t layout, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !out) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (!h->hist) return fail(h, DEMC_EINVAL, kHistoryNotStored);
    if (row0 < 0 || row1 < row0 || row1 > h->c.n_rows || (layout != 0 && layout != 1)) return fail(h, DEMC_EINVAL, "bad rows / layout");
    if (h->c.n_groups_total != h->c.n_groups)
        return fail(h, DEMC_EINVAL, "sharded handle: gather demc_get_history from every rank and re-key on the host");
    const long long n = row1 - row0;
    if (n == 0) return DEMC_OK;
    const size_t elems = (size_t)n * (size_t)h->P * (size_t)(h->c.D + 2);
    DevBuf<double> dev;
    ALLOC(dev, elems);
    KParams k = base_params(h);
    const long long blocks = (long long)((elems + 255) / 256);
    hipLaunchKernelGGL(k_export_chains, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, h->stream, k, (long long)row0, n,
                       (int)layout, (long long)h->c.group_offset * h->c.Np, dev.get());
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, dev, elems * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(h, DEMC_EHIP, std::string("demc_export_chains: ") + hipGetErrorString(e));
    return DEMC_OK;
    });
}

// The three posterior-statistics calls: the shape of the call, the history window, the plan (demc_postplan.hpp), the run.  What a
// call has against its own arguments ranks between the row window and the sharded handle, so check_probs / select_columns are
// asked once here for that order and once more by the planner, which is total.
static HistView hist_view(const demc_handle* h, int64_t row0, int64_t row1) {
    return HistView{h->hist, h->acc_hist, h->lp_hist, h->id_hist, h->P, (long long)row0, (long long)row1, (long long)h->c.group_offset * h->c.Np,
                    h->c.D, h->hist_ld};
}
// the one place the covariance is planned: demc_covariance over the history, demc_bridge over the fit half of its xi buffer
static CovPlan cov_plan(long long N, int D, const int32_t* cols, int n_cols) { return plan_cov(N, D, cols, n_cols); }
// ... and the one place a summary is planned: demc_summarize over the history, the two rank calls over their derived history
static SummaryPlan sum_plan(long long n, long long P, int D, int max_lag, long long rho_len, bool wants_rho) {
    return plan_summary(n, P, D, max_lag, rho_len, wants_rho);
}
static Refusal check_window(const demc_handle* h, PostCall call, int64_t row0, int64_t row1, Refusal args = Refusal()) {
    return check_history_window(call, h->hist != nullptr, row0, row1, h->c.n_rows, h->c.n_groups_total != h->c.n_groups, std::move(args));
}

int32_t demc_summarize(demc_handle* h, int64_t row0, int64_t row1, int32_t max_lag, double* out, double* rho_out, int64_t rho_len) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !out || rho_len < 0 || max_lag < 0) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (Refusal r = check_window(h, POST_SUMMARIZE, row0, row1)) return fail(h, r);
    if (!(rho_out && rho_len > 0)) rho_out = nullptr;
    const SummaryPlan plan = sum_plan(row1 - row0, h->P, h->c.D, (int)max_lag, (long long)rho_len, rho_out != nullptr);
    if (plan.refused) return fail(h, plan.refused);
    std::string msg;
    const int rc = summary_run(hist_view(h, row0, row1), plan, h->stream, out, rho_out, (long long)rho_len, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

int32_t demc_quantiles(demc_handle* h, int64_t row0, int64_t row1, const double* probs, int32_t n_probs, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !out || !probs) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (Refusal r = check_window(h, POST_QUANTILES, row0, row1, check_probs(probs, (int)n_probs))) return fail(h, r);
    const QuantilePlan plan = plan_quantiles((row1 - row0) * h->P, h->c.D, h->hist_ld, probs, (int)n_probs);
    if (plan.refused) return fail(h, plan.refused);
    std::string msg;
    const int rc = quantile_run(hist_view(h, row0, row1), plan, h->stream, out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

int32_t demc_covariance(demc_handle* h, int64_t row0, int64_t row1, const int32_t* cols, int32_t n_cols, double* mean_out, double* cov_out,
                        double* cor_out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (!mean_out && !cov_out && !cor_out) return fail(h, DEMC_EINVAL, "demc_covariance: mean_out, cov_out and cor_out are all NULL");
    int sel[kCovMaxCols];
    if (Refusal r = check_window(h, POST_COVARIANCE, row0, row1, select_columns(h->c.D, cols, (int)n_cols, sel))) return fail(h, r);
    const CovPlan plan = cov_plan((row1 - row0) * h->P, h->c.D, cols, (int)n_cols);
    if (plan.refused) return fail(h, plan.refused);
    std::string msg;
    const int rc = cov_run(hist_view(h, row0, row1), plan, h->stream, mean_out, cov_out, cor_out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

// The two per-observation calls (include/demc_pointwise.h): the shape of the call, the plan (demc_pwplan.hpp), the run
// (demc_pointwise.cpp).  What the plan has against the model ranks where a call's own arguments rank in check_history_window.
static PwModelView pw_model_view(const demc_handle* h) {
    const Model& m = h->m;
    PwModelView v{};
    v.m.family = m.family; v.m.direct = h->c.loglike_mode == DEMC_LOGLIKE_DIRECT; v.m.N = m.N; v.m.n_acc = m.n_acc; v.m.d = m.d; v.m.dp = m.dp_direct;
    v.data = m.data; v.data2 = m.data ? m.data + m.data2_off : nullptr; v.M = m.Ainv; v.xbar = m.xbar; v.order = m.order;
    v.c0 = m.family == DEMC_FAM_MVN_FULL ? m.c0 / (double)m.N : m.c0;  // (MVN_FULL: the constant of ONE row; LNR: sigma)
    return v;
}

int32_t demc_pointwise_loglik(demc_handle* h, const double* theta, int64_t n, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !theta || !out) return DEMC_EINVAL;
    USE_DEVICE(h);
    const PwModelView mv = pw_model_view(h);
    const PwPlan plan = plan_pointwise(PW_LOGLIK, mv.m, (long long)n, h->c.D);
    if (plan.refused) return fail(h, plan.refused);
    std::string msg;
    const int rc = pw_matrix_run(mv, theta, h->c.D, h->dimtab, plan, h->stream, out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

int32_t demc_waic(demc_handle* h, int64_t row0, int64_t row1, double* total_out, double* pointwise_out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    const PwModelView mv = pw_model_view(h);
    const bool window_ok = h->hist != nullptr && row0 >= 0 && row1 - row0 >= 1 && row1 <= h->c.n_rows;
    const PwPlan plan = plan_pointwise(PW_WAIC, mv.m, window_ok ? (long long)(row1 - row0) * h->P : 1, h->c.D);
    if (Refusal r = check_pw_window(h->hist != nullptr, row0, row1, h->c.n_rows, h->c.n_groups_total != h->c.n_groups,
                                    pw_waic_args(plan.refused, total_out || pointwise_out)))
        return fail(h, r);
    std::string msg;
    const int rc = pw_waic_run(mv, hist_view(h, row0, row1), plan, h->stream, total_out, pointwise_out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

// PSIS-LOO (include/demc_loo.h): demc_waic's window and families under its own name, then the plan (demc_looplan.hpp) and the run
// (demc_loo.cpp).  The cap on the draws is the call's own refusal and ranks last.
int32_t demc_loo(demc_handle* h, int64_t row0, int64_t row1, double* total_out, double* pointwise_out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    const PwModelView mv = pw_model_view(h);
    const bool window_ok = h->hist != nullptr && row0 >= 0 && row1 - row0 >= 1 && row1 <= h->c.n_rows;
    const LooPlan plan = plan_loo(mv.m, window_ok ? (long long)(row1 - row0) * h->P : 1);
    if (Refusal r = check_pw_window(h->hist != nullptr, row0, row1, h->c.n_rows, h->c.n_groups_total != h->c.n_groups,
                                    loo_args(plan.model, total_out || pointwise_out), kLooBadRows, kLooSharded))
        return fail(h, r);
    if (plan.refused) return fail(h, plan.refused);
    std::string msg;
    const int rc = loo_run(mv, hist_view(h, row0, row1), plan, h->stream, total_out, pointwise_out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

// The rank diagnostics (include/demc_rank.h): every refusal and the plan are demc_rankplan.hpp's, the run is demc_rank.cpp's.  The
// derived history of a batch holds four series per series ranked; its summary is planned here, for a whole batch and for the last.
// the one place the sort is planned: the two rank calls over their series, demc_hpd over one series of its window
static RankPlan sort_plan(long long n, long long P, int series) { return plan_rank(n, P, series); }
static int32_t rank_call(demc_handle* h, int64_t row0, int64_t row1, int32_t max_lag, bool single, int series, int kind, double* out) {
    if (Refusal r = check_rank_window(h->hist != nullptr, row0, row1, h->c.n_rows, h->c.n_groups_total != h->c.n_groups, h->P,
                                      rank_args(out != nullptr, (int)max_lag, single, series, kind, h->c.D)))
        return fail(h, r);
    const RankPlan plan = sort_plan(row1 - row0, h->P, single ? 1 : h->c.D + 2);
    if (plan.refused) return fail(h, plan.refused);
    const SummaryPlan full = sum_plan(plan.n, plan.P, kRankDerived * plan.batch, (int)max_lag, 0, false);
    const SummaryPlan last = sum_plan(plan.n, plan.P, kRankDerived * plan.last_batch, (int)max_lag, 0, false);
    if (full.refused) return fail(h, full.refused);
    if (last.refused) return fail(h, last.refused);
    std::string msg;
    const int rc = rank_run(hist_view(h, row0, row1), plan, full, last, single ? series : -1, kind, h->stream, out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
}

int32_t demc_rankstats(demc_handle* h, int64_t row0, int64_t row1, int32_t max_lag, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    return rank_call(h, row0, row1, max_lag, false, -1, -1, out);
    });
}

int32_t demc_rank_series(demc_handle* h, int64_t row0, int64_t row1, int32_t series, int32_t kind, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    return rank_call(h, row0, row1, 0, true, (int)series, (int)kind, out);
    });
}

// Highest-density intervals (include/demc_hpd.h): every refusal and the plan are demc_hpdplan.hpp's, on top of the sort of one series
// as demc_rankplan.hpp plans it; the run is demc_rank.cpp's, where the kernels of the sort live.
int32_t demc_hpd(demc_handle* h, int64_t row0, int64_t row1, const double* alphas, int32_t n_alphas, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (Refusal r = check_hpd_window(h->hist != nullptr, row0, row1, h->c.n_rows, h->c.n_groups_total != h->c.n_groups, h->P,
                                     hpd_args(out != nullptr, alphas, (int)n_alphas)))
        return fail(h, r);
    const HpdPlan plan = plan_hpd(sort_plan(row1 - row0, h->P, 1), h->c.D + 2, alphas, (int)n_alphas);
    if (plan.refused) return fail(h, plan.refused);
    std::string msg;
    const int rc = hpd_run(hist_view(h, row0, row1), plan, h->stream, out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

// Bridge sampling (include/demc_bridge.h): every refusal and the plan are demc_bridgeplan.hpp's, the run is demc_bridge.cpp's; the
// callback hands it evaluate_rows, the path behind demc_logpost and demc_set_state, for P rows it has laid out on the device.
int32_t demc_bridge(demc_handle* h, int64_t row0, int64_t row1, int64_t n_prop, uint64_t seed, double* out, double* prop_out, double* post_out,
                    double* fit_out) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    BridgeCall c;
    c.stored = h->hist != nullptr; c.row0 = row0; c.row1 = row1; c.n_rows = h->c.n_rows; c.family = h->m.family; c.has_out = out != nullptr;
    c.sharded = h->c.n_groups_total != h->c.n_groups; c.n_prop = n_prop; c.D = h->c.D; c.P = h->P;
    const BridgePlan plan = plan_bridge(c);
    if (plan.refused) return fail(h, plan.refused);
    int32_t cols[kCovMaxCols];
    for (int k = 0; k < h->c.D; ++k) cols[k] = k;
    const CovPlan fit = cov_plan(plan.n_fit, h->c.D, cols, h->c.D);  // (every scalar of xi, none of the two internal series)
    if (fit.refused) return fail(h, fit.refused);
    HIPCHK(hipStreamSynchronize(h->stream));
    std::string msg;
    const int rc = bridge_run(hist_view(h, row0, row1), h->dimtab, plan, fit, seed, h->stream,
                              [h](double* theta_dev, double* lp_dev) { return evaluate_rows(h, theta_dev, lp_dev); }, out, prop_out, post_out, fit_out, msg);
    return rc == DEMC_OK ? DEMC_OK : fail(h, rc, msg);
    });
}

// What next_segment (demc_schedule.hpp) reads of a call [., end) on this handle: the configuration, the form the call takes, and
// the few facts only the handle knows (its communicator, the overlap switch, a replayed alpha coin).
static StepCall step_call(const demc_handle* h, int64_t end, bool with_migration, Form form) {
    StepCall s;
    s.c = &h->c; s.end = end; s.with_migration = with_migration;
    s.per_phase = form == FORM_PHASE; s.cap = iterations_per_launch(form);
    s.sharded = h->c.n_groups_total != h->c.n_groups || (h->comm && h->own_comm);
    s.overlap = h->comm_overlap;
    s.replay = h->rp.active; s.replayed_step = h->rp.has_step; s.u_step = h->rp.u_step;
    return s;
}

#define NCCLCHK(expr)                                                                                         \
    do {                                                                                                      \
        ncclResult_t r_ = (expr);                                                                             \
        if (r_ != ncclSuccess) return fail(h, DEMC_ERCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// this shard's rows inside the [n_groups_total][D+3] exchange buffer: rank r's block starts at r * n_groups rows, which is
// where an IN-PLACE ncclAllGather expects the send buffer (recvbuff + rank * sendcount)
static double* own_rows(demc_handle* h) { return h->mig_rows + (size_t)h->c.group_offset * ((size_t)h->c.D + 3); }

// the ONE collective of the path: all-gather of every shard's candidate rows (migration.jl:11-19 split around it), enqueued
// on stream s.  No host synchronisation.
static int gather_enqueue(demc_handle* h, hipStream_t s) {
    const size_t cnt = (size_t)h->c.n_groups * ((size_t)h->c.D + 3);
    NCCLCHK(ncclAllGather(own_rows(h), h->mig_rows, cnt, ncclDouble, h->comm, s));
    h->n_exchanges += 1;
    return DEMC_OK;
}

// migration! of iteration `iter` on a handle that owns a communicator: pack -> all-gather -> apply, stream-ordered
static int exchange_enqueue(demc_handle* h, int64_t iter) {
    migration_enqueue(h, iter, own_rows(h), nullptr, true, false);
    int rc = gather_enqueue(h, h->stream);
    if (rc != DEMC_OK) return rc;
    migration_enqueue(h, iter, nullptr, h->mig_rows, false, true);
    return DEMC_OK;
}

static int step_body(demc_handle* h, int64_t iter0, int32_t n_iters, bool with_migration);

// update! + store_samples! of iterations [iter0, iter0 + n_iters) for a SUBSET of the handle's groups (local indices),
// enqueued only.  The list travels through a ring of pinned host / device copies: the device copy is refilled by a copy ON
// THE HANDLE'S STREAM, i.e. behind every kernel that still reads its previous content.
static int update_subset(demc_handle* h, int64_t iter0, int32_t n_iters, const int32_t* groups, int32_t n) {
    if (n == 0) return DEMC_OK;
    if (Refusal r = refuse_subset(h->c, h->rp.active && h->rp.n_mig > 0, groups, n)) return fail(h, r);
    // (a list of up to n_groups entries fits the slot as create sized it; a longer one -- repeated indices -- makes it grow)
    StagedList<int>& list = h->glist.slot[h->glist.next];
    h->glist.next = (h->glist.next + 1) % demc_handle::GroupLists::kRing;
    int* host = nullptr;
    if (list.stage((size_t)n, h->stream, &host) != hipSuccess) return fail(h, DEMC_EHIP, "group-list ring");
    std::memcpy(host, groups, (size_t)n * sizeof(int));
    if (list.send((size_t)n, h->stream) != hipSuccess) return fail(h, DEMC_EHIP, "copying the group list");
    h->cur_glist = list.dev;
    h->cur_ng = n;
    const int rc = step_body(h, iter0, n_iters, false);
    h->cur_glist = nullptr;
    h->cur_ng = 0;
    return rc;
}

// Per-group-asynchronous migration behind the boundary: migration of iteration `iter` + the update of
// iterations [iter, iter + run).  The sub-group of an exchange is a pure function of (seed, iter), so the groups it did NOT
// select start their update while the all-gather is in flight on the side stream; only the selected groups wait for it.
static int exchange_overlapped(demc_handle* h, int64_t iter, int run) {
    const demc_config& c = h->c;
    std::vector<int32_t> perm((size_t)groups_total(c)), sel((size_t)groups_total(c)), mine((size_t)c.n_groups), rest((size_t)c.n_groups);
    const Partition part = exchange_partition(c, iter, perm.data(), sel.data(), mine.data(), rest.data());
    migration_enqueue(h, iter, own_rows(h), nullptr, true, false);
    HIPCHK(hipEventRecord(h->ev_pack, h->stream));
    HIPCHK(hipStreamWaitEvent(h->side, h->ev_pack, 0));
    int rc = gather_enqueue(h, h->side);  // the one collective, off the main stream
    if (rc != DEMC_OK) return rc;
    HIPCHK(hipEventRecord(h->ev_gath, h->side));
    rc = update_subset(h, iter, run, rest.data(), part.n_rest);  // overlaps the gather
    if (rc != DEMC_OK) return rc;
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_gath, 0));
    migration_enqueue(h, iter, nullptr, h->mig_rows, false, true);
    return update_subset(h, iter, run, mine.data(), part.n_mine);
}

// launch order of the groups for the frozen-row sweeps of iterations [iter0, iter0 + n_iters): whether a table is built and what
// goes into it, demc_schedule.hpp; here it is staged and sent.  A table that cannot be built -- no memory, an event that fails --
// means no hint, not an error.
static void plan_frozen_order(demc_handle* h, int64_t iter0, int32_t n_iters) {
    h->frozen.iters = 0;
    const size_t need = frozen_order_entries(setup_of(h), h->mask_runs.data(), h->mask_runs.size(), n_iters);
    if (need == 0) return;
    int* order = nullptr;
    if (h->frozen.table.stage(need, h->stream, &order) != hipSuccess) { (void)hipGetLastError(); return; }
    fill_frozen_order(h->c, h->mask_runs.data(), h->mask_runs.size(), iter0, n_iters, order);
    if (h->frozen.table.send(need, h->stream) != hipSuccess) return;
    h->frozen.iter0 = iter0; h->frozen.iters = n_iters;
}

// iterations [iter0, iter0 + n_iters) enqueued on the handle's stream, segment by segment (next_segment); nothing is drained
static int step_body(demc_handle* h, int64_t iter0, int32_t n_iters, bool with_migration) {
    const demc_config& c = h->c;
    plan_frozen_order(h, iter0, n_iters);
    h->snap2_iter = -1;  // (a by-product snapshot lives inside one call)
    bool form_ok[N_FORMS];
    for (int f = 0; f < N_FORMS; ++f) form_ok[f] = h->form[f].ok;
    const Form form = choose_form(form_ok, c, h->rp.active, h->cur_glist != nullptr);
    const StepCall call = step_call(h, iter0 + n_iters, with_migration, form);
    for (int64_t iter = iter0; iter < call.end;) {
        const Segment seg = next_segment(call, iter);
        if (seg.migrate == MIG_EXCHANGE || seg.migrate == MIG_OVERLAPPED)
            if (Refusal r = refuse_exchange(h->multi != nullptr, h->comm != nullptr)) return fail(h, r);
        int rc = DEMC_OK;
        if (seg.migrate == MIG_OVERLAPPED)
            rc = exchange_overlapped(h, iter, seg.run);  // the exchange, and the segment's iterations as its two subset updates
        else {
            if (seg.migrate == MIG_LOCAL) migration_enqueue(h, iter, h->mig_rows, h->mig_rows, true, true);  // main.jl:85
            if (seg.migrate == MIG_EXCHANGE) rc = exchange_enqueue(h, iter);
            if (rc == DEMC_OK && form != FORM_PHASE) rc = launch_form(h, form, iter, seg.run);  // the segment in one launch
            for (int b = 0; rc == DEMC_OK && form == FORM_PHASE && b < n_sweeps(c); ++b) {        // ... or one iteration, sweep by sweep
                const unsigned char* mask = c.n_blocks > 0 ? h->masks + (size_t)b * c.D : nullptr;
                rc = run_sweep(h, iter, (unsigned)b, mask, stored_row(c, h->hist.get() != nullptr, iter, b));
            }
        }
        if (rc != DEMC_OK) return rc;
        iter += seg.run;
    }
    HIPCHK(hipGetLastError());
    return DEMC_OK;
}

static int step_checks(demc_handle* h, int64_t iter0, int32_t n_iters) {
    if (Refusal r = refuse_step(h->c, h->m.family >= 0, iter0, n_iters)) return fail(h, r);
    return DEMC_OK;
}

static int drain(demc_handle* h) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    if (h->st.err && *h->st.err.get()) {
        *h->st.err.get() = 0u;
        return fail(h, DEMC_EHIP, "streaming-resident kernel: a hand-over between the workgroups of a group timed out");
    }
    if (h->comm) {  // a collective that failed after it was enqueued shows up here
        ncclResult_t ar = ncclSuccess;
        if (ncclCommGetAsyncError(h->comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress)
            return fail(h, DEMC_ERCCL, std::string("communicator: ") + ncclGetErrorString(ar));
    }
    return DEMC_OK;
}

static int32_t step_impl(demc_handle* h, int64_t iter0, int32_t n_iters, bool with_migration, bool do_drain = true) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    int rc = step_checks(h, iter0, n_iters);
    if (rc != DEMC_OK) return rc;
    rc = step_body(h, iter0, n_iters, with_migration);
    if (rc != DEMC_OK || !do_drain) return rc;
    return drain(h);
    });
}

int32_t demc_step(demc_handle* h, int64_t iter0, int32_t n_iters) { return step_impl(h, iter0, n_iters, true); }
int32_t demc_update(demc_handle* h, int64_t iter0, int32_t n_iters) { return step_impl(h, iter0, n_iters, false); }
int32_t demc_step_async(demc_handle* h, int64_t iter0, int32_t n_iters) { return step_impl(h, iter0, n_iters, true, false); }
int32_t demc_synchronize(demc_handle* h) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    return drain(h);
    });
}

int32_t demc_update_groups_async(demc_handle* h, int64_t iter0, int32_t n_iters, const int32_t* groups, int32_t n) {
    return guarded(h, [&]() -> int32_t {
    if (!h || n < 0 || (n > 0 && !groups)) return DEMC_EINVAL;
    USE_DEVICE(h);
    int rc = step_checks(h, iter0, n_iters);
    if (rc != DEMC_OK) return rc;
    if (Refusal r = refuse_subset_call(h->c, n_iters)) return fail(h, r);
    return update_subset(h, iter0, n_iters, groups, n);
    });
}

int32_t demc_migration_groups(const demc_config* cfg, int64_t iter, int32_t* sel, int32_t* n_sel) {
    if (!cfg || !sel || !n_sel) return DEMC_EINVAL;
    *n_sel = 0;
    try {
        std::vector<int> perm((size_t)std::max(groups_total(*cfg), 1));
        *n_sel = select_groups(*cfg, iter, perm.data(), sel);
    } catch (...) {
        return DEMC_ENOMEM;
    }
    return DEMC_OK;
}

int32_t demc_migration_due(const demc_config* cfg, int64_t iter) { return cfg && migration_due(*cfg, iter) ? 1 : 0; }

// One half of migration! around the caller's exchange: select_particle into pack_rows (pack), or select_groups + shift_particles!
// from all_rows, the rows of all groups (apply).  The drained entry points take a null pointer for the handle's own buffer.
static int32_t migration_half(demc_handle* h, int64_t iter, bool pack, double* pack_rows, const double* all_rows, bool drained) {
    return guarded(h, [&]() -> int32_t {
    if (!h || (!drained && !(pack ? pack_rows : all_rows))) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (!pack && !all_rows && h->c.n_groups_total != h->c.n_groups)
        return fail(h, DEMC_EINVAL, "sharded handle needs the all-gathered rows");
    if (pack) migration_enqueue(h, iter, pack_rows ? pack_rows : h->mig_rows.get(), nullptr, true, false);
    else migration_enqueue(h, iter, nullptr, all_rows ? all_rows : h->mig_rows.get(), false, true);
    if (drained) HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipGetLastError());
    return DEMC_OK;
    });
}
int32_t demc_migration_pack(demc_handle* h, int64_t iter, double* dev_rows) { return migration_half(h, iter, true, dev_rows, nullptr, true); }
int32_t demc_migration_apply(demc_handle* h, int64_t iter, const double* dev_all_rows) { return migration_half(h, iter, false, nullptr, dev_all_rows, true); }
int32_t demc_migration_pack_async(demc_handle* h, int64_t iter, double* dev_rows) { return migration_half(h, iter, true, dev_rows, nullptr, false); }
int32_t demc_migration_apply_async(demc_handle* h, int64_t iter, const double* dev_all_rows) { return migration_half(h, iter, false, nullptr, dev_all_rows, false); }

// ---- the communicator behind the boundary (SURVEY 8b "demc_create_multi / DEMC_ERCCL", 8e) ----
int32_t demc_comm_unique_id(void* id_out, int32_t nbytes) {
    return guarded(nullptr, [&]() -> int32_t {
    if (!id_out || nbytes < (int32_t)sizeof(ncclUniqueId)) return DEMC_EINVAL;
    static_assert(sizeof(ncclUniqueId) == DEMC_COMM_ID_BYTES, "DEMC_COMM_ID_BYTES must be sizeof(ncclUniqueId)");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return DEMC_ERCCL;
    std::memcpy(id_out, &id, sizeof id);
    return DEMC_OK;
    });
}

static int comm_side_objects(demc_handle* h) {
    if (!h->side) HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    if (!h->ev_pack) HIPCHK(h->ev_pack.create(hipEventDisableTiming));
    if (!h->ev_gath) HIPCHK(h->ev_gath.create(hipEventDisableTiming));
    return DEMC_OK;
}

static int comm_shape_check(demc_handle* h, int rank, int world) {
    const demc_config& c = h->c;
    if (world < 1 || rank < 0 || rank >= world) return fail(h, DEMC_EINVAL, "need 0 <= rank < world");
    // equal shards in rank order: what the in-place all-gather (and select_groups over GLOBAL group indices) assume
    if ((long long)c.n_groups * world != c.n_groups_total || c.group_offset != rank * c.n_groups)
        return fail(h, DEMC_EINVAL, "communicator shape: n_groups_total must be world * n_groups and group_offset rank * n_groups");
    return DEMC_OK;
}

int32_t demc_comm_init(demc_handle* h, const void* unique_id, int32_t rank, int32_t world) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !unique_id) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (h->comm || h->multi) return fail(h, DEMC_EINVAL, "the handle already has a communicator");
    int rc = comm_shape_check(h, rank, world);
    if (rc != DEMC_OK) return rc;
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    NCCLCHK(ncclCommInitRank(&h->comm, world, id, rank));
    h->own_comm = true; h->comm_rank = rank; h->comm_world = world;
    return comm_side_objects(h);
    });
}

int32_t demc_comm_destroy(demc_handle* h) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    if (h->multi) return fail(h, DEMC_EINVAL, "the communicator of a shard belongs to its set (demc_destroy_multi)");
    USE_DEVICE(h);
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
    if (h->side) HIPCHK(hipStreamSynchronize(h->side));
    if (h->comm && h->own_comm) NCCLCHK(ncclCommDestroy(h->comm));
    h->comm = nullptr; h->own_comm = false; h->comm_rank = 0; h->comm_world = 1; h->comm_overlap = false;
    return DEMC_OK;
    });
}

int32_t demc_comm_set_overlap(demc_handle* h, int32_t on) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    if (on && (!h->comm || h->multi)) return fail(h, DEMC_EINVAL, "needs a communicator of the handle's own (demc_comm_init)");
    h->comm_overlap = on != 0;
    return DEMC_OK;
    });
}

static int32_t exchange_impl(demc_handle* h, int64_t iter, bool do_drain) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (!h->comm) return fail(h, DEMC_EINVAL, "the handle has no communicator (demc_comm_init)");
    int rc = exchange_enqueue(h, iter);
    if (rc != DEMC_OK || !do_drain) return rc;
    return drain(h);
    });
}
int32_t demc_migration_exchange(demc_handle* h, int64_t iter) { return exchange_impl(h, iter, true); }
int32_t demc_migration_exchange_async(demc_handle* h, int64_t iter) { return exchange_impl(h, iter, false); }

int32_t demc_comm_allreduce(demc_handle* h, double* host_inout, int32_t n, int32_t op) {
    return guarded(h, [&]() -> int32_t {
    if (!h || n < 0 || (n > 0 && !host_inout) || op < 0 || op > 2) return DEMC_EINVAL;
    USE_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!h->comm || h->comm_world == 1) return DEMC_OK;  // one rank: the values are the result
    const size_t m = n > 0 ? (size_t)n : 1;              // n == 0: a barrier (one dummy element goes round)
    if (h->red_cap < m) {
        h->red_cap = 0;
        ALLOC(h->red_dev, m);
        h->red_cap = m;
    }
    double dummy = 0.0;
    HIPCHK(hipMemcpyAsync(h->red_dev, n > 0 ? host_inout : &dummy, m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const ncclRedOp_t rop = op == 0 ? ncclSum : op == 1 ? ncclMax : ncclMin;
    NCCLCHK(ncclAllReduce(h->red_dev, h->red_dev, m, ncclDouble, rop, h->comm, h->stream));
    HIPCHK(hipMemcpyAsync(n > 0 ? host_inout : &dummy, h->red_dev, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return drain(h);
    });
}

int32_t demc_comm_stats(demc_handle* h, int64_t* out3) {
    if (!h || !out3) return DEMC_EINVAL;
    out3[0] = h->comm ? h->comm_world : 1;
    out3[1] = h->comm ? h->comm_rank : 0;
    out3[2] = h->n_exchanges;
    return DEMC_OK;
}

// ---- single-process multi-GPU set: one host thread (a Julia task) drives every shard ----
}  // extern "C"  (the struct below is C++)

struct demc_multi {
    std::vector<demc_handle*> shard;
    bool rccl = false;              // distinct devices: one communicator per shard from ncclCommInitAll
    std::vector<Event> packed, copied;  // shared-device transport: rows packed / peers' rows copied
    bool copied_valid = false;
    std::string err;
};

namespace {
int mfail(demc_multi* m, int code, const std::string& msg) noexcept {
    if (m) {
        try { m->err = msg; } catch (...) {}
    }
    return code;
}
// first failing shard's message becomes the set's
int mshard_fail(demc_multi* m, int r, int code) {
    return mfail(m, code, "shard " + std::to_string(r) + ": " + m->shard[(size_t)r]->err);
}
}  // namespace

extern "C" {

const char* demc_multi_last_error(demc_multi* m) { return m ? m->err.c_str() : "null set"; }

int32_t demc_destroy_multi(demc_multi* m) {
    return guarded(nullptr, [&]() -> int32_t {
    if (!m) return DEMC_OK;
    for (demc_handle* h : m->shard) {
        if (!h) continue;
        hipSetDevice(h->c.device_id);
        if (h->stream) hipStreamSynchronize(h->stream);
        if (h->comm) { ncclCommDestroy(h->comm); h->comm = nullptr; }
        h->multi = nullptr;
    }
    for (size_t r = m->shard.size(); r-- > 0;) {  // (last first: shards that share a device borrow an earlier shard's stream)
        if (m->shard[r]) hipSetDevice(m->shard[r]->c.device_id);
        if (r < m->packed.size()) m->packed[r].reset();
        if (r < m->copied.size()) m->copied[r].reset();
        if (m->shard[r]) demc_destroy(m->shard[r]);
    }
    delete m;
    return DEMC_OK;
    });
}

int32_t demc_create_multi(const demc_config* cfg, int32_t n_shards, const int32_t* device_ids, demc_multi** out) {
    if (!cfg || !out || n_shards < 1) return DEMC_EINVAL;
    *out = nullptr;
    demc_multi* m = new (std::nothrow) demc_multi();
    if (!m) return DEMC_ENOMEM;
    *out = m;  // returned even on failure so that demc_multi_last_error() can be read; the caller destroys it
    return guarded(nullptr, [&]() -> int32_t {
    if (cfg->n_groups % n_shards != 0) return mfail(m, DEMC_EINVAL, "n_groups (of the whole population) must divide by n_shards");
    if (cfg->group_offset != 0 || (cfg->n_groups_total != 0 && cfg->n_groups_total != cfg->n_groups))
        return mfail(m, DEMC_EINVAL, "demc_create_multi takes the configuration of the WHOLE population (group_offset 0)");
    // DE-MC_Z (resample, crossover.jl:113-124) draws its partner cells from the history of ALL particles; a shard holds the
    // history of its own groups only, so a sharded set would sample another pool than the single handle it promises to
    // reproduce bit for bit: refused (one shard is fine).  The one-process-per-GPU road documents the shard-local pool instead
    // (include/demc.h).
    if (cfg->partner_kind == DEMC_PARTNER_HISTORY && n_shards > 1)
        return mfail(m, DEMC_EUNSUPPORTED, "demc_create_multi: history partners (resample) draw from the history of all particles; "
                                           "a sharded set cannot reproduce that pool -- use one shard, or partner_kind current");
    const int G = cfg->n_groups / n_shards;
    std::vector<int> devs((size_t)n_shards);
    bool distinct = true;
    for (int r = 0; r < n_shards; ++r) {
        devs[(size_t)r] = device_ids ? device_ids[r] : r;
        for (int q = 0; q < r; ++q) distinct = distinct && devs[(size_t)q] != devs[(size_t)r];
    }
    m->shard.assign((size_t)n_shards, nullptr);
    for (int r = 0; r < n_shards; ++r) {
        demc_config c = *cfg;
        c.n_groups = G; c.group_offset = r * G; c.n_groups_total = cfg->n_groups; c.device_id = devs[(size_t)r];
        // one population on several GPUs: every shard takes the lane geometry of the unsharded run, so that the set
        // reproduces a single handle bit for bit (demc_config.geometry_groups)
        if (c.geometry_groups == 0) c.geometry_groups = cfg->n_groups;
        const int rc = demc_create(&c, &m->shard[(size_t)r]);
        if (rc != DEMC_OK) return mfail(m, rc, "shard " + std::to_string(r) + ": " + (m->shard[(size_t)r] ? m->shard[(size_t)r]->err : "demc_create"));
        m->shard[(size_t)r]->multi = m;
    }
    struct Seal { demc_multi* m; ~Seal() { for (demc_handle* h : m->shard) if (h) h->multi_sealed = true; } } seal{m};
    if (n_shards > 1 && distinct) {
        std::vector<ncclComm_t> comms((size_t)n_shards);
        const ncclResult_t nr = ncclCommInitAll(comms.data(), n_shards, devs.data());
        if (nr != ncclSuccess) return mfail(m, DEMC_ERCCL, std::string("ncclCommInitAll: ") + ncclGetErrorString(nr));
        for (int r = 0; r < n_shards; ++r) {
            demc_handle* h = m->shard[(size_t)r];
            h->comm = comms[(size_t)r]; h->own_comm = false; h->comm_rank = r; h->comm_world = n_shards;
        }
        m->rccl = true;
    } else if (n_shards > 1) {
        // shards that share a device (several shards per GPU): the rows change hands by device-to-device copies ordered by
        // events -- RCCL refuses two ranks on one device
        m->packed.resize((size_t)n_shards);
        m->copied.resize((size_t)n_shards);
        // Shards on ONE device run on one stream (the first such shard's): the streaming-resident kernels size their grid
        // for the whole chip and their workgroups spin on each other, so two of them in flight at once on a device would not
        // be co-resident (a 2 x 40-group set: 2 x 160 workgroups on 256 CUs).  In stream order the set is what one handle
        // of all groups does, group range by group range.
        for (int r = 1; r < n_shards; ++r)
            for (int q = 0; q < r; ++q)
                if (devs[(size_t)q] == devs[(size_t)r]) {
                    const int rc = demc_set_stream(m->shard[(size_t)r], (void*)m->shard[(size_t)q]->stream);
                    if (rc != DEMC_OK) return mshard_fail(m, r, rc);
                    break;
                }
        for (int r = 0; r < n_shards; ++r) {
            if (hipSetDevice(devs[(size_t)r]) != hipSuccess ||
                m->packed[(size_t)r].create(hipEventDisableTiming) != hipSuccess ||
                m->copied[(size_t)r].create(hipEventDisableTiming) != hipSuccess)
                return mfail(m, DEMC_EHIP, "creating the exchange events");
        }
    }
    return DEMC_OK;
    });
}

int32_t demc_multi_size(demc_multi* m) { return m ? (int32_t)m->shard.size() : 0; }
demc_handle* demc_multi_shard(demc_multi* m, int32_t r) {
    return (m && r >= 0 && (size_t)r < m->shard.size()) ? m->shard[(size_t)r] : nullptr;
}

// migration! of iteration `iter` over the whole set, enqueued on every shard's stream
static int multi_exchange(demc_multi* m, int64_t iter) {
    const int n = (int)m->shard.size();
    for (int r = 0; r < n; ++r) {
        demc_handle* h = m->shard[(size_t)r];
        if (hipSetDevice(h->c.device_id) != hipSuccess) return mfail(m, DEMC_EHIP, "hipSetDevice");
        if (!m->rccl && m->copied_valid)  // nobody may still be copying the rows this shard is about to overwrite
            for (int q = 0; q < n; ++q)
                if (q != r && hipStreamWaitEvent(h->stream, m->copied[(size_t)q], 0) != hipSuccess) return mfail(m, DEMC_EHIP, "hipStreamWaitEvent");
        migration_enqueue(h, iter, own_rows(h), nullptr, true, false);
        if (!m->rccl && hipEventRecord(m->packed[(size_t)r], h->stream) != hipSuccess) return mfail(m, DEMC_EHIP, "hipEventRecord");
    }
    if (m->rccl) {
        // one host thread, several devices: the collective calls of all ranks go out as one group
        ncclResult_t nr = ncclGroupStart();
        for (int r = 0; r < n && nr == ncclSuccess; ++r) {
            demc_handle* h = m->shard[(size_t)r];
            const size_t cnt = (size_t)h->c.n_groups * ((size_t)h->c.D + 3);
            nr = ncclAllGather(own_rows(h), h->mig_rows, cnt, ncclDouble, h->comm, h->stream);
            h->n_exchanges += 1;
        }
        const ncclResult_t ne = ncclGroupEnd();
        if (nr == ncclSuccess) nr = ne;
        if (nr != ncclSuccess) return mfail(m, DEMC_ERCCL, std::string("ncclAllGather: ") + ncclGetErrorString(nr));
    } else {
        for (int r = 0; r < n; ++r) {
            demc_handle* h = m->shard[(size_t)r];
            if (hipSetDevice(h->c.device_id) != hipSuccess) return mfail(m, DEMC_EHIP, "hipSetDevice");
            const size_t W = (size_t)h->c.D + 3, bytes = (size_t)h->c.n_groups * W * sizeof(double);
            for (int q = 0; q < n; ++q) {
                if (q == r) continue;
                demc_handle* src = m->shard[(size_t)q];
                if (hipStreamWaitEvent(h->stream, m->packed[(size_t)q], 0) != hipSuccess ||
                    hipMemcpyAsync(h->mig_rows + (size_t)src->c.group_offset * W, own_rows(src), bytes, hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
                    return mfail(m, DEMC_EHIP, "copying a peer's migration rows");
            }
            if (hipEventRecord(m->copied[(size_t)r], h->stream) != hipSuccess) return mfail(m, DEMC_EHIP, "hipEventRecord");
            h->n_exchanges += 1;
        }
        m->copied_valid = true;
    }
    for (int r = 0; r < n; ++r) {
        demc_handle* h = m->shard[(size_t)r];
        if (hipSetDevice(h->c.device_id) != hipSuccess) return mfail(m, DEMC_EHIP, "hipSetDevice");
        migration_enqueue(h, iter, nullptr, h->mig_rows, false, true);
    }
    return DEMC_OK;
}

int32_t demc_multi_step(demc_multi* m, int64_t iter0, int32_t n_iters) {
    return guarded(nullptr, [&]() -> int32_t {
    if (!m || m->shard.empty()) return DEMC_EINVAL;
    const int n = (int)m->shard.size();
    for (int r = 0; r < n; ++r) {
        const int rc = step_checks(m->shard[(size_t)r], iter0, n_iters);
        if (rc != DEMC_OK) return mshard_fail(m, r, rc);
    }
    demc_handle* h0 = m->shard[0];
    // The set's own segments: the alpha coin is a pure function of (seed, iteration), so every shard sees the same runs
    // (main.jl:85).  The coins count only between shards, and the segments are uncapped: every shard caps its own launches.
    const StepCall call = set_call(step_call(h0, iter0 + n_iters, true, FORM_PHASE), n);
    for (int64_t it = iter0; it < call.end;) {
        const Segment seg = next_segment(call, it);
        const int run = seg.run;
        if (seg.migrate == MIG_EXCHANGE) {
            const int rc = multi_exchange(m, it);
            if (rc != DEMC_OK) return rc;
        }
        for (int r = 0; r < n; ++r) {  // every shard's update enqueued before any is waited for: the GPUs run side by side
            demc_handle* h = m->shard[(size_t)r];
            if (hipSetDevice(h->c.device_id) != hipSuccess) return mfail(m, DEMC_EHIP, "hipSetDevice");
            // (a single shard keeps its on-device migration inside the update)
            const int rc = step_body(h, it, run, n == 1);
            if (rc != DEMC_OK) return mshard_fail(m, r, rc);
        }
        it += run;
    }
    for (int r = 0; r < n; ++r) {
        demc_handle* h = m->shard[(size_t)r];
        if (hipSetDevice(h->c.device_id) != hipSuccess) return mfail(m, DEMC_EHIP, "hipSetDevice");
        const int rc = drain(h);
        if (rc != DEMC_OK) return mshard_fail(m, r, rc);
    }
    return DEMC_OK;
    });
}

int32_t demc_apply_migration(demc_handle* h, const int32_t* src_slot, const int32_t* dst_slot, int32_t n) {
    return guarded(h, [&]() -> int32_t {
    if (!h || n < 0 || (n > 0 && (!src_slot || !dst_slot))) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (n == 0) return DEMC_OK;
    std::vector<char> seen((size_t)h->P, 0);
    for (int k = 0; k < n; ++k) {
        if (src_slot[k] < 0 || src_slot[k] >= h->P || dst_slot[k] < 0 || dst_slot[k] >= h->P)
            return fail(h, DEMC_EINVAL, "migration slot out of range");
        if (seen[(size_t)dst_slot[k]]) return fail(h, DEMC_EINVAL, "migration destination slots must be distinct");
        seen[(size_t)dst_slot[k]] = 1;
    }
    const size_t W = (size_t)h->c.D + 2;
    DevBuf<int> d_slots;
    DevBuf<double> d_stage;
    HIPCHK(d_slots.alloc(2 * (size_t)n));
    if (d_stage.alloc((size_t)n * W) != hipSuccess) return fail(h, DEMC_ENOMEM, "out of device memory for the migration staging rows");
    hipError_t e = hipMemcpyAsync(d_slots, src_slot, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slots + n, dst_slot, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        KParams k = base_params(h);
        const unsigned wgs = (unsigned)(((size_t)n * W + 255) / 256);
        hipLaunchKernelGGL(k_slot_moves, dim3(wgs), dim3(256), 0, h->stream, k, d_slots.get(), d_stage.get(), n, 0);
        hipLaunchKernelGGL(k_slot_moves, dim3(wgs), dim3(256), 0, h->stream, k, d_slots + n, d_stage.get(), n, 1);
        e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) e = hipGetLastError();
    }
    return e == hipSuccess ? DEMC_OK : fail(h, DEMC_EHIP, hipGetErrorString(e));
    });
}

int32_t demc_get_weights(demc_handle* h, double* weight) {
    if (!h || !weight) return DEMC_EINVAL;
    return demc_get_state(h, nullptr, weight, nullptr);
}

int32_t demc_logpost(demc_handle* h, const double* theta, int64_t n, double* out) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !theta || !out || n < 0) return DEMC_EINVAL;
    USE_DEVICE(h);
    if (Refusal r = refuse_without_model(h->m.family >= 0)) return fail(h, r);
    const size_t P = (size_t)h->P, D = (size_t)h->c.D;
    std::vector<double> w(P);
    for (int64_t off = 0; off < n; off += (int64_t)P) {
        const size_t m = (size_t)((n - off < (int64_t)P) ? n - off : (int64_t)P);
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemset(h->scratch_theta, 0, P * D * sizeof(double)));
        HIPCHK(hipMemcpy(h->scratch_theta, theta + (size_t)off * D, m * D * sizeof(double), hipMemcpyHostToDevice));
        h->sim_entity_base = (unsigned)off;  // (a simulated likelihood evaluates row r of the call at entity r)
        int rc = evaluate_rows(h, h->scratch_theta, h->scratch_w);
        h->sim_entity_base = 0;
        if (rc != DEMC_OK) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(w.data(), h->scratch_w, P * sizeof(double), hipMemcpyDeviceToHost));
        std::memcpy(out + off, w.data(), m * sizeof(double));
    }
    return DEMC_OK;
    });
}

int32_t demc_set_replay(demc_handle* h, const demc_replay* r) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rp = Replay{};
    if (!r) return DEMC_OK;
    const demc_config& c = h->c;
    const size_t P = (size_t)h->P, D = (size_t)c.D, G = (size_t)c.n_groups;
    if (r->partner)
        for (size_t i = 0; i < 3 * P; ++i)
            if (r->partner[i] >= c.Np) return fail(h, DEMC_EINVAL, "replay: partner row outside the group");
    if (r->mig_particle)
        for (size_t g = 0; g < G; ++g)
            if (r->mig_particle[g] >= c.Np) return fail(h, DEMC_EINVAL, "replay: migration particle outside the group");
    if (r->n_mig_groups < 0 || r->n_mig_groups > c.n_groups_total || (r->n_mig_groups > 0 && !r->mig_groups))
        return fail(h, DEMC_EINVAL, "replay: bad migration sub-group");
    {
        std::vector<char> seen((size_t)c.n_groups_total, 0);
        for (int i = 0; i < r->n_mig_groups; ++i) {
            const int g = r->mig_groups[i];
            if (g < 0 || g >= c.n_groups_total || seen[(size_t)g]) return fail(h, DEMC_EINVAL, "replay: migration groups must be distinct and in range");
            seen[(size_t)g] = 1;
        }
    }
    auto up = [&](auto& dst, const auto* src, size_t n) -> int {
        if (!src || n == 0) return DEMC_OK;
        int rc = dev_alloc(h, dst, n);
        if (rc != DEMC_OK) return rc;
        HIPCHK(hipMemcpy(dst, src, n * sizeof(*src), hipMemcpyHostToDevice));
        return DEMC_OK;
    };
    Replay rp;  // filled aside: a failure on the way leaves the handle without a replay
    int rc = up(rp.group, r->u_group, G);
    if (rc == DEMC_OK) rc = up(rp.part, r->u_part, 5 * P);
    if (rc == DEMC_OK) rc = up(rp.partner, reinterpret_cast<const long long*>(r->partner), 3 * P);
    if (rc == DEMC_OK) rc = up(rp.noise, r->u_noise, P * D);
    if (rc == DEMC_OK) rc = up(rp.znoise, r->z_noise, P * D);
    if (rc == DEMC_OK) rc = up(rp.recomb, r->u_recomb, P * D);
    if (rc == DEMC_OK) rc = up(rp.mig_particle, reinterpret_cast<const long long*>(r->mig_particle), G);
    if (rc == DEMC_OK) rc = up(rp.mig_groups, r->mig_groups, (size_t)r->n_mig_groups);
    if (rc != DEMC_OK) return rc;
    rp.n_mig = r->n_mig_groups;
    if (r->u_step && r->u_step[0] == r->u_step[0]) {
        rp.has_step = true;
        rp.u_step = r->u_step[0];
    }
    rp.active = true;
    h->rp = std::move(rp);
    return DEMC_OK;
    });
}

int32_t demc_get_trace(demc_handle* h, double* proposal, double* w_prop, double* log_adj, int32_t* idx, uint8_t* accepted) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    const size_t P = (size_t)h->P, D = (size_t)h->c.D;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (proposal) HIPCHK(hipMemcpy(proposal, h->prop, P * D * sizeof(double), hipMemcpyDeviceToHost));
    if (w_prop) HIPCHK(hipMemcpy(w_prop, h->tr_w, P * sizeof(double), hipMemcpyDeviceToHost));
    if (log_adj) HIPCHK(hipMemcpy(log_adj, h->prop_adj, P * sizeof(double), hipMemcpyDeviceToHost));
    if (idx) HIPCHK(hipMemcpy(idx, h->tr_idx, P * 4 * sizeof(int), hipMemcpyDeviceToHost));
    if (accepted) HIPCHK(hipMemcpy(accepted, h->tr_acc, P, hipMemcpyDeviceToHost));
    return DEMC_OK;
    });
}

int32_t demc_last_kernels(demc_handle* h, char* out, int32_t nbytes) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !out || nbytes < 1) return DEMC_EINVAL;
    const demc_handle::LastPlan& L = h->last;
    std::string s = L.k1 ? L.k1->name(L.k1->key) : "";
    switch (L.k2) {
        case K2_NONE: break;
        case K2_CROSS_MFMA: s += " + " + name_cross(L.k2_key); break;
        case K2_DIRECT_MVN: s += " + " + name_direct(L.k2_key); break;
        case K2_OBS: s += " + k_obs_loglike"; break;
        case K2_LBA_WAVE: s += " + " + name_lba_wave(L.k2_key); break;
        case K2_HIER: s += " + k_hier_loglike"; break;
        case K2_USER: s += " + k_user_loglike"; break;
        case K2_USER_ROW: s += " + k_user_row"; break;
        case K2_SIM: s += " + " + name_sim(L.k2_key); break;
        case K2_ODE: s += " + " + name_ode(L.k2_key); break;
    }
    if (L.k3) s += " + k_accept_store";
    std::snprintf(out, (size_t)nbytes, "%s", s.c_str());
    return DEMC_OK;
    });
}

int32_t demc_timing_enable(demc_handle* h, int32_t on) {
    return guarded(h, [&]() -> int32_t {
    if (!h) return DEMC_EINVAL;
    USE_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    drain_events(h);
    h->timing = on != 0;
    return DEMC_OK;
    });
}

int32_t demc_timing_read(demc_handle* h, double* out10, int32_t reset) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !out10) return DEMC_EINVAL;
    USE_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    drain_events(h);
    for (int i = 0; i < 5; ++i) {
        out10[i] = h->t_ms[i];
        out10[5 + i] = (double)h->t_n[i];
    }
    if (reset)
        for (int i = 0; i < 5; ++i) { h->t_ms[i] = 0; h->t_n[i] = 0; }
    return DEMC_OK;
    });
}

int32_t demc_timing_clock(demc_handle* h, double* out4) {
    return guarded(h, [&]() -> int32_t {
    if (!h || !out4) return DEMC_EINVAL;
    USE_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (!h->clk_dev || h->clk_n == 0) return DEMC_OK;  // no DIRECT likelihood launch ran with timing enabled
    std::vector<unsigned long long> t(3 * h->clk_n);
    HIPCHK(hipMemcpy(t.data(), h->clk_dev, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // per CU (the shader-clock counters of different CUs are not aligned: differencing across CUs gave 1.8 - 13.7 "GHz"): the
    // workgroup that finished first there and the one that finished last, by the 100 MHz reference; the shader-clock ticks between
    // the two over the reference ticks between the two is the clock the CU held over that span of the launch.  A CU whose span is
    // under 20 us (a launch of a single round of workgroups) says nothing.
    std::vector<size_t> order;
    order.reserve(h->clk_n);
    for (size_t i = 0; i < h->clk_n; ++i)
        if (t[3 * i + 1] != 0) order.push_back(i);  // (a workgroup that reported)
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return t[3 * a + 2] < t[3 * b + 2]; });
    std::vector<double> mhz;
    for (size_t a = 0; a < order.size();) {
        size_t b = a, lo = order[a], hi = order[a];
        for (; b < order.size() && t[3 * order[b] + 2] == t[3 * order[a] + 2]; ++b) {
            const size_t i = order[b];
            if (t[3 * i + 1] < t[3 * lo + 1]) lo = i;
            if (t[3 * i + 1] > t[3 * hi + 1]) hi = i;
        }
        if (t[3 * lo + 1] != 0 && t[3 * hi + 1] - t[3 * lo + 1] >= 2000 && t[3 * hi] > t[3 * lo])
            mhz.push_back(100.0 * (double)(t[3 * hi] - t[3 * lo]) / (double)(t[3 * hi + 1] - t[3 * lo + 1]));
        a = b;
    }
    if (mhz.empty()) return DEMC_OK;
    std::sort(mhz.begin(), mhz.end());
    out4[0] = mhz[mhz.size() / 2];
    out4[1] = mhz.front();
    out4[2] = mhz.back();
    out4[3] = (double)mhz.size();
    return DEMC_OK;
    });
}

}  // extern "C"
