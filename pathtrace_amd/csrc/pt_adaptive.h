// pt_adaptive.h -- the stopping rule of pt_render_adaptive, written once for the kernels (pt_film_adaptive.h) and the host
// compilers of the CPU tests (tests/test_adaptive_rule_cpu.py).  Plain f64 arithmetic; build with -ffp-contract=off so
// that no compiler fuses a multiply into an add the rule does not write as one.
//
// Per pixel, in sample order: S1 = sum L, S2 = sum L^2 with L the sample's luminance (weights of world.rs:359) in f64
// from its f32 radiance.  A check at n >= 2 samples:
//   mean = S1 / n,  var = max(0, (S2 - S1 * mean) / (n - 1)),  se = sqrt(var / n)
//   converged  <=>  S1, S2 finite  and  rel_tol > 0  and  se <= rel_tol * max(mean, abs_floor)
// rel_tol = 0 asks for no tolerance at all: nothing converges early (a pixel whose samples are all equal would otherwise
// pass 0 <= 0).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_AD_HD __host__ __device__ inline
#else
#define PT_AD_HD inline
#endif

namespace ptad {

PT_AD_HD double luminance(float r, float g, float b) {
    return 0.2126 * (double)r + 0.7152 * (double)g + 0.0722 * (double)b;
}

PT_AD_HD bool finite(double v) { return v - v == 0.0; }      // false for NaN and +-inf

// mean and var / n (= se^2) at n >= 2 samples: the rule's first line, for check() and for pt_denoise_var.h
PT_AD_HD double mean_var(double s1, double s2, unsigned n, double* mean_out) {
    const double dn = (double)n;
    const double mean = s1 / dn;
    double var = (s2 - s1 * mean) / (dn - 1.0);
    var = var > 0.0 ? var : 0.0;
    *mean_out = mean;
    return var / dn;
}

// Check at n >= 2 samples.  rel_err = se / max(mean, abs_floor) (NaN when a sum is not finite).
PT_AD_HD bool check(double s1, double s2, unsigned n, double rel_tol, double abs_floor, double* rel_err) {
    double mean;
    const double se = __builtin_sqrt(mean_var(s1, s2, n, &mean));
    const double scale = mean > abs_floor ? mean : abs_floor;
    const bool ok = finite(s1) && finite(s2);
    *rel_err = ok ? se / scale : __builtin_nan("");
    return ok && rel_tol > 0.0 && se <= rel_tol * scale;
}

}  // namespace ptad
