// demc_ode.cpp -- the instances of k_ode_loglike (demc_ode.hpp: the likelihood kernel of the ODE-trajectory families), in a
// translation unit of their own so that `make -j` compiles them beside the rest of the library.
#define DEMC_DEVICE_HELPERS_ONLY
#include "demc_ode.hpp"

namespace demc {
#define DEMC_X_(...) template __global__ void k_ode_loglike<__VA_ARGS__>(OdeKParams);
DEMC_ODE_INSTANCES(DEMC_X_)
#undef DEMC_X_
}  // namespace demc
