// demc_instances.hpp -- host only: one table per templated kernel, expanded from the instance list next to the kernel (the X-macro
// its .cpp unit and its `extern template` declarations come from).  An entry is the instance's function, its template arguments as
// plain ints and the formatter that names it: the function the runtime launches, the LDS attribute it is given (size_k1_lds) and the
// name demc_last_kernels reports all come from ONE record, and adding an instance is one line in its list.
#pragma once
#include <cstddef>
#include <string>

namespace demc {

constexpr int kMaxKey = 7;
struct InstKey { int v[kMaxKey]; };  // the template arguments in declaration order, zero-padded (a trailing default of false / 0)
constexpr bool same_key(const InstKey& a, const InstKey& b) {
    for (int i = 0; i < kMaxKey; ++i)
        if (a.v[i] != b.v[i]) return false;
    return true;
}

template <typename Fn>
struct Inst {
    Fn fn;
    InstKey key;
    std::string (*name)(const InstKey&);
};

template <typename I, size_t N>
constexpr const I* find_inst(const I (&tab)[N], const InstKey& key) {
    for (const I& e : tab)
        if (same_key(e.key, key)) return &e;
    return nullptr;
}
template <typename I, size_t N>
constexpr bool unique_keys(const I (&tab)[N]) {
    for (size_t i = 0; i < N; ++i)
        for (size_t j = i + 1; j < N; ++j)
            if (same_key(tab[i].key, tab[j].key)) return false;
    return true;
}

// ---- the names demc_last_kernels reports: one formatter per kernel, reading the launched entry's own key.  Tests, bench.py and
// the tools compare these strings; their irregular forms (the LEAN level of k_propose prints as false / true / 2, k_res_mvn and
// k_frozen_sweep name only the arguments that tell their instances apart) are part of the interface.
inline std::string int_list(const InstKey& k, int n) {
    std::string s;
    for (int i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(k.v[i]);
    return s;
}
inline const char* tf(int v) { return v == 0 ? "false" : v == 1 ? "true" : "2"; }
inline std::string name_propose(const InstKey& k) {  // <WG, TILE, TAIL, RES, LEAN, STREAM>
    static const char* const tails[4] = {"TAIL_NONE", "TAIL_PREP", "TAIL_PREP_MFMA", "TAIL_OBS"};
    return "k_propose<" + std::to_string(k.v[0]) + "," + tf(k.v[1]) + "," + tails[k.v[2] & 3] + "," + tf(k.v[3]) + "," + tf(k.v[4]) +
           (k.v[5] ? ",true>" : ">");
}
inline std::string name_res_mvn(const InstKey& k) {  // <WG, STREAM, DT, HIST, OCC, ISO, DIR>
    return "k_res_mvn<" + std::to_string(k.v[0]) + "," + tf(k.v[1]) + "," + std::to_string(k.v[2]) +
           (k.v[3] ? "," + std::to_string(k.v[3]) : "") + (k.v[5] ? ",iso" : "") + (k.v[6] ? ",direct" : "") + ">";
}
inline std::string name_frozen(const InstKey& k) { return "k_frozen_sweep<" + std::to_string(k.v[0]) + (k.v[3] ? ",big>" : ">"); }  // <WG, MINW, PAIRS, BIG>
inline std::string name_longrow(const InstKey& k) { return "k_longrow<" + int_list(k, 1) + ">"; }
inline std::string name_res_obs(const InstKey& k) { return "k_res_obs<" + int_list(k, 1) + ">"; }
inline std::string name_cross(const InstKey& k) { return "k_cross_mfma<" + int_list(k, 2) + ">"; }
inline std::string name_direct(const InstKey& k) {  // <DP>, k_direct_mvn_x4<DP> as <DP, 4>: "k_direct_mvn<32>x4"
    return "k_direct_mvn<" + int_list(k, 1) + ">" + (k.v[1] ? "x" + std::to_string(k.v[1]) : "");
}
inline std::string name_lba_wave(const InstKey&) { return "k_lba_wave"; }
inline std::string name_sim(const InstKey& k) {  // <SIM, EST>; SIM_USER: the instance hiprtc compiled around the caller's simulator
    return std::string("k_sim_loglike<") + (k.v[1] == EST_KDE ? "kde" : k.v[1] == EST_FREQ ? "frequency" : "kde_choice") + "," +
           (k.v[0] == SIM_NORMAL ? "normal" : k.v[0] == SIM_BINOMIAL ? "binomial" : k.v[0] == SIM_LNR ? "lnr" : "user") + ">";
}
inline std::string name_ode(const InstKey& k) { return std::string("k_ode_loglike<") + (k.v[0] == ODE_LV ? "lv" : "?") + ">"; }  // <SYS>

// ---- the tables
using K1Fn = void (*)(KParams);  // K1 and the kernels that carry a whole update: k_propose, k_longrow, k_res_mvn, k_frozen_sweep, k_res_obs
using K1Inst = Inst<K1Fn>;
using ChunkFn = void (*)(KParams, int, unsigned long long*);  // k_direct_mvn, k_lba_wave
using CrossFn = void (*)(KParams, const double*, int, int, const double*, int, int, int);
using SimFn = void (*)(SimKParams);
using OdeFn = void (*)(OdeKParams);
#define DEMC_ENTRY(KERNEL, NAME, ...) {KERNEL<__VA_ARGS__>, {{__VA_ARGS__}}, NAME},
#define DEMC_E_PROPOSE(...) DEMC_ENTRY(k_propose, name_propose, __VA_ARGS__)
#define DEMC_E_RES_MVN(...) DEMC_ENTRY(k_res_mvn, name_res_mvn, __VA_ARGS__)
#define DEMC_E_FROZEN(...) DEMC_ENTRY(k_frozen_sweep, name_frozen, __VA_ARGS__)
#define DEMC_E_LONGROW(...) DEMC_ENTRY(k_longrow, name_longrow, __VA_ARGS__)
#define DEMC_E_RES_OBS(...) DEMC_ENTRY(k_res_obs, name_res_obs, __VA_ARGS__)
#define DEMC_E_DIRECT(...) DEMC_ENTRY(k_direct_mvn, name_direct, __VA_ARGS__)
#define DEMC_E_DIRECT_X4(DP) {k_direct_mvn_x4<DP>, {{DP, 4}}, name_direct},  // (a kernel of its own: k_direct_mvn<DP> keeps its symbol)
#define DEMC_E_CROSS(...) DEMC_ENTRY(k_cross_mfma, name_cross, __VA_ARGS__)
#define DEMC_E_LBA_WAVE(...) DEMC_ENTRY(k_lba_wave, name_lba_wave, __VA_ARGS__)
#define DEMC_E_SIM(...) DEMC_ENTRY(k_sim_loglike, name_sim, __VA_ARGS__)
#define DEMC_E_SIM_CHOICE(SIM) {k_sim_choice<SIM>, {{SIM, EST_KDE_CHOICE}}, name_sim},  // (the pair kernel: its estimator is its own)
#define DEMC_E_ODE(...) DEMC_ENTRY(k_ode_loglike, name_ode, __VA_ARGS__)
constexpr K1Inst kPropose[] = {DEMC_K1_PHASE_INSTANCES(DEMC_E_PROPOSE) DEMC_K1_RES_INSTANCES(DEMC_E_PROPOSE) DEMC_K1_STREAM_INSTANCES(DEMC_E_PROPOSE)};
constexpr K1Inst kResMvn[] = {DEMC_RESMVN_INSTANCES(DEMC_E_RES_MVN) DEMC_RESMVN_INSTANCES_DIR(DEMC_E_RES_MVN)};
constexpr K1Inst kFrozen[] = {DEMC_FROZEN_INSTANCES(DEMC_E_FROZEN)};
constexpr K1Inst kLongrow[] = {DEMC_LONGROW_INSTANCES(DEMC_E_LONGROW)};
constexpr K1Inst kResObs[] = {DEMC_RESOBS_INSTANCES(DEMC_E_RES_OBS)};
constexpr Inst<ChunkFn> kDirect[] = {DEMC_DIRECT_INSTANCES(DEMC_E_DIRECT) DEMC_DIRECT_X4_INSTANCES(DEMC_E_DIRECT_X4)};
constexpr Inst<CrossFn> kCross[] = {DEMC_CROSS_INSTANCES(DEMC_E_CROSS)};
constexpr Inst<ChunkFn> kLbaWave[] = {DEMC_LBA_WAVE_INSTANCES(DEMC_E_LBA_WAVE)};
constexpr Inst<SimFn> kSim[] = {DEMC_SIM_INSTANCES(DEMC_E_SIM) DEMC_SIM_CHOICE_INSTANCES(DEMC_E_SIM_CHOICE)};
constexpr Inst<OdeFn> kOde[] = {DEMC_ODE_INSTANCES(DEMC_E_ODE)};
static_assert(unique_keys(kPropose) && unique_keys(kResMvn) && unique_keys(kFrozen) && unique_keys(kLongrow) && unique_keys(kResObs) &&
                  unique_keys(kCross) && unique_keys(kDirect) && unique_keys(kLbaWave) && unique_keys(kSim) && unique_keys(kOde),
              "an instance list names the same template arguments twice");

}  // namespace demc
