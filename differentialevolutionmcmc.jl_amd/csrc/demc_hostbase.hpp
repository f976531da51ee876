// demc_hostbase.hpp -- the little the host-only headers share (demc_prep.hpp, demc_geometry.hpp, demc_postplan.hpp): how a refusal
// is carried, and the power-of-two rule.  Plain C++17, no device header.
#pragma once
#include "../../include/demc.h"

#include <string>

namespace demc {

// Why a call is refused: the status code and the message demc_last_error returns.  DEMC_OK: not refused.
struct Refusal {
    int code = DEMC_OK;
    std::string message;
    explicit operator bool() const { return code != DEMC_OK; }
};

inline int pow2_ceil(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace demc
