// demc_dimtab.hpp -- the bounds / prior table as the kernels read it, and the host arithmetic of its constants.  No HIP: the kernel
// headers include it (demc_device.hpp), and so does the host-only preparation (demc_prep.hpp), which fills these types.
#pragma once
#include <cmath>

namespace demc {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;
constexpr double kLogPi = 1.1447298858494001741434273513531;
constexpr double kPi = 3.14159265358979323846264338327950288;

enum Prior : int {
    PR_FLAT = 0, PR_NORMAL = 1, PR_HALFCAUCHY = 2, PR_UNIFORM = 3, PR_BETA = 4, PR_NORMAL_REF = 5, PR_GAMMA = 6,
    PR_EXPONENTIAL = 7, PR_LOGNORMAL = 8, PR_CAUCHY = 9
};

// x-independent part of a scalar's log-prior, computed on the host (keeps lgamma / atan out of the kernels)
inline double prior_const(int kind, double a, double b) {
    switch (kind) {
        case PR_NORMAL:
            return -0.5 * kLog2Pi - std::log(b);
        case PR_HALFCAUCHY:
            return -kLogPi - std::log(b) - std::log(1.0 - (std::atan((0.0 - a) / b) / kPi + 0.5));
        case PR_UNIFORM:
            return -std::log(b - a);
        case PR_BETA:
            return -(std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b));
        case PR_GAMMA:
            return -a * std::log(b) - std::lgamma(a);
        case PR_EXPONENTIAL:
            return -std::log(b);
        case PR_LOGNORMAL:
            return -std::log(b) - 0.5 * kLog2Pi;
        case PR_CAUCHY:
            return -kLogPi - std::log(b);
        default:
            return 0.0;
    }
}

// Per-scalar constants, packed so that one dimension costs three 16-byte loads: bounds (de.bounds flattened) and
// the prior entry (model.prior_loglike as data).  b = 1/scale for Normal / half-Cauchy; c = the x-independent
// part of the log-density (prior_const()).
struct DimTab {
    double lo, hi;
    double a, b;
    double c;
    int kind, ref;
};

// Run-length form of the DimTab array: models give whole blocks of scalars the same bounds and prior (cfg4: 10 000 subject
// effects ~ Normal(0, sd); cfg3: 32 means ~ Normal(0,1)), so the table is a handful of segments.  The kernels keep them in LDS
// and look a scalar's entry up by its segment instead of streaming 48 bytes per scalar from L2/HBM -- at D = 10 002 that
// stream was larger than the particle rows themselves.
struct DimSeg {
    int start, pad;  // first scalar of the segment
    DimTab t;
    double pad2;
};
constexpr int kMaxDimSeg = 16;
constexpr int kMaxMaskRun = 16;
static_assert(sizeof(DimTab) == 48 && sizeof(DimSeg) == 64, "the kernels load the table by these layouts");

}  // namespace demc
