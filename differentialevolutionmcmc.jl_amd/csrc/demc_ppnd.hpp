// demc_ppnd.hpp -- the inverse of the standard normal distribution function, Wichura's algorithm AS 241 (PPND16; Appl. Statist. 37
// (1988) 477-484), in ONE stated operation order: the text a kernel and a host test both compile, so the normal scores of
// demc_rankstats are the same expression on both sides.  Plain C++: every polynomial is Horner's rule written as
// multiply-then-add, no fma (the library is built with -ffp-contract=off), one log and one sqrt outside the central region.
//   q = p - 1/2.  |q| <= 0.425:  r = 0.180625 - q q,           z = q A(r) / B(r)
//   otherwise  r = sqrt(-log(min(p, 1 - p)));  r <= 5: r -= 1.6, z = C(r) / D(r);  else r -= 5, z = E(r) / F(r);  z = -z when q < 0
// p = 0 gives -inf, p = 1 gives +inf, p outside [0, 1] or NaN gives NaN.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define DEMC_PPND_HD __host__ __device__
#else
#define DEMC_PPND_HD
#endif

namespace demc {

DEMC_PPND_HD inline double ppnd_poly8(double r, double c7, double c6, double c5, double c4, double c3, double c2, double c1, double c0) {
    double s = c7;
    s = s * r + c6;
    s = s * r + c5;
    s = s * r + c4;
    s = s * r + c3;
    s = s * r + c2;
    s = s * r + c1;
    s = s * r + c0;
    return s;
}

DEMC_PPND_HD inline double ppnd16(double p) {
    if (!(p >= 0.0 && p <= 1.0)) {  // NaN in, or outside [0, 1]: NaN (0 / 0, or NaN / NaN)
        const double d = p - p;
        return d / d;
    }
    const double q = p - 0.5;
    if (::fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = ppnd_poly8(r, 2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                                      1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e0);
        const double den = ppnd_poly8(r, 5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                                      5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0);
        return q * num / den;
    }
    double r = q < 0.0 ? p : 1.0 - p;
    r = ::sqrt(-::log(r));  // (p = 0 or 1: r = +inf, both polynomials overflow the same way -- handled first)
    if (!(r < 1.0e300)) return q < 0.0 ? -HUGE_VAL : HUGE_VAL;
    double z;
    if (r <= 5.0) {
        r = r - 1.6;
        const double num = ppnd_poly8(r, 7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e0,
                                      3.64784832476320460504e0, 5.76949722146069140550e0, 4.63033784615654529590e0, 1.42343711074968357734e0);
        const double den = ppnd_poly8(r, 1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                                      6.89767334985100004550e-1, 1.67638483018380384940e0, 2.05319162663775882187e0, 1.0);
        z = num / den;
    } else {
        r = r - 5.0;
        const double num = ppnd_poly8(r, 2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                                      2.96560571828504891230e-1, 1.78482653991729133580e0, 5.46378491116411436990e0, 6.65790464350110377720e0);
        const double den = ppnd_poly8(r, 2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                                      1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0);
        z = num / den;
    }
    return q < 0.0 ? -z : z;
}

}  // namespace demc
