// demc_constants.hpp -- the plain enums and limits that both the kernels and the host-only launch geometry (demc_geometry.hpp)
// read.  Plain C++: no device header, nothing but integers.
#pragma once
#include <cstddef>

namespace demc {

enum Family : int {
    FAM_GAUSSIAN = 0, FAM_MVN_ISO = 1, FAM_MVN_FULL = 2, FAM_BINOMIAL = 3, FAM_HIER_BINOMIAL = 4,
    FAM_HIER_GAUSSIAN = 5, FAM_LBA = 6, FAM_LNR = 7, FAM_RASTRIGIN = 8, FAM_USER = 100
};
enum Mode : int { MODE_STEP = 0, MODE_IDENT = 1 };  // IDENT: theta' = theta, always accepted (init / logpost)

// the fused tail compiled into a k_propose instance (demc_kernels.hpp: TAIL)
enum K1Tail : int { TAIL_NONE = 0, TAIL_PREP = 1, TAIL_PREP_MFMA = 2, TAIL_OBS = 3 };

constexpr int kFrozenMax = 8;  // scalars a block may move for k_frozen_sweep (demc_frozen.hpp)

constexpr size_t kMaxDynLds = 150 * 1024;  // of the 160 KB per CU; the rest covers the kernels' static __shared__

}  // namespace demc
