// demc_simlike.cpp -- the instances of k_sim_loglike and k_sim_choice (demc_simlike.hpp: the likelihood kernels of the simulation-based models), in a
// translation unit of their own so that `make -j` compiles them beside the rest of the library.
#define DEMC_DEVICE_HELPERS_ONLY
#include "demc_simlike.hpp"

namespace demc {
#define DEMC_X_(...) template __global__ void k_sim_loglike<__VA_ARGS__>(SimKParams);
DEMC_SIM_INSTANCES(DEMC_X_)
#undef DEMC_X_
#define DEMC_X_(...) template __global__ void k_sim_choice<__VA_ARGS__>(SimKParams);
DEMC_SIM_CHOICE_INSTANCES(DEMC_X_)
#undef DEMC_X_
}  // namespace demc
