// sincos_cr.hpp -- sin and cos of an angle in [0, 2 pi], correctly rounded
// (PTG_FLAG_REFERENCE_F64's plain estimator, ref64.hpp).
//
// The reference calls libm's sin and cos; glibc's are within 0.55 ulp, so they
// return the correctly rounded value but for the few arguments whose true
// value lies within 0.05 ulp of a rounding boundary.  The device math
// library's are within about an ulp, which is a different last bit far more
// often: a diffuse bounce then leaves in a direction an ulp off, and a path
// that ends in the sky carries that into its value (tests/test_gpu_ties.py:
// on the sky-lit clusters 1.1-1.2 % of the pixels of a 48x32x16 frame differed
// from Mode A/xs in their last bit).  This one is evaluated in double-double
// (a pair of doubles, about 104 bits) and rounded once: of the 2^24 angles
// 2 pi m 2^-24 the draws can give, its sin differs from glibc's on 25,128 and
// its cos on 24,782 (0.15 % each; tests/sincos_check.cpp counts them).
//
// Plain double operations and fma only, the same on the host and the device.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTG_HD __host__ __device__
#else
#define PTG_HD
#endif

namespace ptg {
namespace cr {

struct dd {
    double h, l;  // value h + l, |l| <= ulp(h) / 2
};
PTG_HD inline dd sum(double a, double b)  // exact
{
    const double s = a + b, bb = s - a;
    return dd{s, (a - (s - bb)) + (b - bb)};
}
PTG_HD inline dd add(dd a, dd b)
{
    const dd s = sum(a.h, b.h);
    const double e = s.l + (a.l + b.l), h = s.h + e;
    return dd{h, e - (h - s.h)};
}
PTG_HD inline dd mul(dd a, dd b)
{
    const double p = a.h * b.h;
    const double e = fma(a.h, b.h, -p) + (a.h * b.l + a.l * b.h), h = p + e;
    return dd{h, e - (h - p)};
}
PTG_HD inline dd div(dd a, double d)
{
    const double q1 = a.h / d;
    const double q2 = (fma(-q1, d, a.h) + a.l) / d, h = q1 + q2;
    return dd{h, q2 - (h - q1)};
}

// a in [0, 2 pi]: a - k pi/2 with pi/2 in three pieces (33 + 33 + 53 bits: k *
// piece is exact, and so is the first subtraction), then the two Taylor series
// up to r^28 / 28! (< 2^-100 for |r| <= pi/4), term by term.
PTG_HD inline void sincos(double a, double &sn, double &cs)
{
    const double k = floor(a * 6.36619772367581382433e-01 + 0.5);
    dd r = sum(a - k * 1.57079632673412561417e+00, -(k * 6.07710050630396597660e-11));
    r = add(r, dd{-(k * 2.02226624879595063154e-21), 0.0});
    const dd z = mul(r, r);
    dd ts = r, s = r, tc = dd{1.0, 0.0}, c = dd{1.0, 0.0};
    for (int j = 1; j <= 14; ++j) {
        tc = div(mul(tc, z), -(double)((2 * j - 1) * (2 * j)));
        ts = div(mul(ts, z), -(double)((2 * j) * (2 * j + 1)));
        c = add(c, tc);
        s = add(s, ts);
    }
    const int quad = (int)k & 3;
    sn = quad == 0 ? s.h : quad == 1 ? c.h : quad == 2 ? -s.h : -c.h;
    cs = quad == 0 ? c.h : quad == 1 ? -s.h : quad == 2 ? -c.h : s.h;
}

}  // namespace cr
}  // namespace ptg
