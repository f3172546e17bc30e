// design_window.h -- what the designed tables of the resampler (cmhip_src_design) and of the drift stage
// (cmhip_drift_design) are made of, once: I0 from its power series and one tap of a Kaiser-windowed sinc
// (include/coolmic_hip.h states both).  Host only, double precision, plain C++: no HIP, no kernel sees it.
#ifndef CMHIP_DESIGN_WINDOW_H
#define CMHIP_DESIGN_WINDOW_H

#include <math.h>

namespace cmhip {

constexpr double DESIGN_BETA = 7.5;

// I0 from its power series, summed until a term no longer changes the sum
static inline double design_i0(double x)
{
    double sum = 1.0, t = 1.0;
    for (unsigned k = 1;; k++) {
        t = t * (x / 2.0) / (double)k;
        const double next = sum + t * t;
        if (next == sum)
            return sum;
        sum = next;
    }
}

// 2 fc sinc(2 fc x) w(x), w the Kaiser window of half-width `half` around x = 0 (0 outside it); i0b = design_i0(DESIGN_BETA)
static inline double design_tap(double x, double half, double fc, double i0b)
{
    const double u = x / half;
    const double arg = 1.0 - u * u;
    const double w = design_i0(DESIGN_BETA * sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
    const double ts = 2.0 * fc * x;
    const double sinc = ts == 0.0 ? 1.0 : sin(M_PI * ts) / (M_PI * ts);
    return 2.0 * fc * sinc * w;
}

}  // namespace cmhip
#endif
