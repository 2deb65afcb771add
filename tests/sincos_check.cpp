// csrc/sincos_cr.hpp on the host, on every 2^24 angle 2 pi m 2^-24 a draw can
// give (or every `step`-th, argv[1], and those next to the multiples of
// pi/2): the error against the long double sinl / cosl in ulps of the result,
// and how often the result differs from libm's double sin / cos.  Prints "max_ulp <e> sin_differs <n> cos_differs <n> of <N>".
// Built without FMA contraction, as the device code is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../cpu-path-tracing_amd/csrc/sincos_cr.hpp"

static double ulps(double got, long double ref)
{
    int e;
    std::frexp((double)ref, &e);  // |ref| in [2^(e-1), 2^e): ulp = 2^(e-53)
    return (double)(fabsl((long double)got - ref) / ldexpl(1.0L, e - 53));
}

int main(int argc, char **argv)
{
    const uint32_t step = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 1u;
    const double pi = 3.14159265358979323846;
    double worst = 0.0;
    long ds = 0, dc = 0, n = 0;
    auto check = [&](uint32_t m) {
        const double a = 2 * pi * (m * 0x1p-24);
        double s, c;
        ptg::cr::sincos(a, s, c);
        const long double rs = sinl((long double)a), rc = cosl((long double)a);
        if (rs != 0.0L)
            worst = std::fmax(worst, ulps(s, rs));
        if (rc != 0.0L)
            worst = std::fmax(worst, ulps(c, rc));
        ds += s != std::sin(a);
        dc += c != std::cos(a);
        ++n;
    };
    for (uint32_t m = 0; m < (1u << 24); m += step)
        check(m);
    for (uint32_t j = 1; step > 1 && j <= 4; ++j)  // next to the multiples of pi/2, where the reduced angle is tiny
        for (int d = -2; d <= 2; ++d)
            if ((j << 22) + d < (1u << 24))
                check((j << 22) + d);
    std::printf("max_ulp %.6f sin_differs %ld cos_differs %ld of %ld\n", worst, ds, dc, n);
    return 0;
}
