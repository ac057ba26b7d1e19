// pt_denoise_var.h -- the variance pt_adaptive_variance_device hands to pt_denoise_var_device, written once for the kernel
// (k_adaptive_variance in pt_film_adaptive.h) and the host compilers of the CPU tests (tests/test_denoise_var_cpu.py).
// Plain f64 arithmetic, like pt_adaptive.h; build with -ffp-contract=off.
//
// Per pixel: the adaptive pass's f64 sums (sum R, sum G, sum B, S1 = sum L, S2 = sum L^2), its sample count n >= 2 and the
// albedo of its feature record.  pt_adaptive.h gives mean = S1 / n and var_c = max(0, (S2 - S1 mean) / (n - 1)) / n, the
// squared standard error of the film's mean luminance.  The filter works on the demodulated colour u = c / a,
// a = max(albedo, 1e-3) per channel, so the variance is carried over by the squared ratio of the two mean luminances:
//   c_k = sums[k] / n,  L_u = 0.2126 c_0 / a_0 + 0.7152 c_1 / a_1 + 0.0722 c_2 / a_2,  var_u = var_c (L_u / mean)^2
// (exact for a grey albedo, where L_u = mean / a; an approximation otherwise).  The result is NaN when S1 or S2 is not
// finite, var_u when mean > 0 and L_u and var_u are finite, and 0 otherwise (a black pixel, a miss).  NaN tells the filter
// that the pixel has no measurement.
#pragma once
#include "pt_adaptive.h"

namespace ptdv {

PT_AD_HD float pixel_variance(const double* sums, unsigned n, float albedo_r, float albedo_g, float albedo_b) {
    double mean;
    const double var_c = ptad::mean_var(sums[3], sums[4], n, &mean);
    const double dn = (double)n;
    const double a0 = (double)albedo_r > 1e-3 ? (double)albedo_r : 1e-3;
    const double a1 = (double)albedo_g > 1e-3 ? (double)albedo_g : 1e-3;
    const double a2 = (double)albedo_b > 1e-3 ? (double)albedo_b : 1e-3;
    const double lu = 0.2126 * (sums[0] / dn / a0) + 0.7152 * (sums[1] / dn / a1) + 0.0722 * (sums[2] / dn / a2);
    const double ratio = lu / mean;
    const double var_u = var_c * (ratio * ratio);
    const bool sums_ok = ptad::finite(sums[3]) && ptad::finite(sums[4]);      // (then mean and var_c are finite too)
    const bool measured = mean > 0.0 && ptad::finite(lu) && ptad::finite(var_u);
    return (float)(!sums_ok ? __builtin_nan("") : measured ? var_u : 0.0);
}

}  // namespace ptdv
