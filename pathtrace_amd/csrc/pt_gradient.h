// pt_gradient.h -- the temporal gradient of pt_temporal_gradient_device, written once for the kernels
// (k_gradient_list, k_gradient_strata, k_gradient_alpha, k_gradient_alpha_camera in pt_film_temporal.h), the host and the host compilers of the CPU
// tests (tests/test_gradient_cpu.py).  Plain f64 arithmetic, like pt_adaptive.h; build with -ffp-contract=off.
//
// Strata: the image W x H is cut into 3 x 3 blocks, SW = ceil(W / 3) by SH = ceil(H / 3) of them, clipped at the right and
// bottom edges.  Stratum (bx, by) has ONE gradient pixel, (min(3 bx + seed % 3, W - 1), min(3 by + (seed / 3) % 3, H - 1)):
// the caller advances seed per frame and the gradient pixel walks through its block.
// Record of a stratum, two doubles: with c_new the gradient pixel's film re-traced in the current scene, c_old its film in
// the previous frame (f32 RGB) and L(c) = 0.2126 r + 0.7152 g + 0.0722 b in f64,
//   delta = |L_new - L_old|,  N = max(L_new, L_old);  (NaN, NaN) when either L is not finite.
// Pixel (x, y): its stratum is (x / 3, y / 3); over the strata (bx + i, by + j), |i|, |j| <= radius, inside the grid, summed
// row-major (j outer): D = sum delta, Nn = sum N.
//   lambda = 1 when a record of the window is not finite;  min(1, scale D / Nn) when Nn > 0;  0 otherwise
//   alpha_p = (float)(alpha_min + lambda (1 - alpha_min))        (alpha_min, scale widened to f64 first)
// D = 0 gives alpha_p == alpha_min exactly.
//
// Under a moving camera (pt_temporal_gradient_camera_device, k_gradient_alpha_camera) the strata, their list,
// re-trace and records are those above in the PREVIOUS frame's image (rendered through the previous camera), and a pixel of
// the current image takes the window around the stratum of the previous-image pixel its first-hit point projects to: with
// (x', y') the reprojection of rule 2 of PtTemporal, (xi, yi) = (floor(x' + 0.5), floor(y' + 0.5)) -- lookup_pixel -- and
// alpha_p = pixel_alpha(rec, SW, SH, xi, yi, ...).  No measurement (NaN) where the pixel has no depth, the reprojection fails
// or (xi, yi) lies outside the image.  Cameras equal field by field: (xi, yi) = (x, y) for every pixel, misses included.
#pragma once
#include "pt_adaptive.h"

namespace ptgr {

constexpr unsigned kBlock = 3;         // a stratum is kBlock x kBlock pixels
constexpr unsigned kMaxRadius = 8;     // PtGradient.radius

PT_AD_HD unsigned strata(unsigned n) { return (n + kBlock - 1u) / kBlock; }

PT_AD_HD void stratum_pixel(unsigned bx, unsigned by, unsigned W, unsigned H, unsigned seed, unsigned* x, unsigned* y) {
    const unsigned px = kBlock * bx + seed % kBlock, py = kBlock * by + (seed / kBlock) % kBlock;
    *x = px < W - 1u ? px : W - 1u;
    *y = py < H - 1u ? py : H - 1u;
}

PT_AD_HD void stratum_record(const float* c_new, const float* c_old, double* rec) {
    const double ln = ptad::luminance(c_new[0], c_new[1], c_new[2]), lo = ptad::luminance(c_old[0], c_old[1], c_old[2]);
    const double d = ln - lo;
    const bool ok = ptad::finite(ln) && ptad::finite(lo);
    rec[0] = ok ? (d < 0.0 ? -d : d) : __builtin_nan("");
    rec[1] = ok ? (ln > lo ? ln : lo) : __builtin_nan("");
}

PT_AD_HD float pixel_alpha(const double* rec, unsigned SW, unsigned SH, unsigned x, unsigned y, unsigned radius, float scale,
                           float alpha_min) {
    const int bx = (int)(x / kBlock), by = (int)(y / kBlock), r = (int)radius;
    double D = 0.0, Nn = 0.0;
    bool bad = false;
    for (int j = -r; j <= r; ++j) {
        const int sy = by + j;
        if (sy < 0 || sy >= (int)SH) continue;
        for (int i = -r; i <= r; ++i) {
            const int sx = bx + i;
            if (sx < 0 || sx >= (int)SW) continue;
            const double* q = rec + 2 * ((unsigned long long)sy * SW + (unsigned)sx);
            bad = bad || !ptad::finite(q[0]) || !ptad::finite(q[1]);
            D += q[0];
            Nn += q[1];
        }
    }
    double lambda = 0.0;
    if (bad) lambda = 1.0;
    else if (Nn > 0.0) {
        const double v = (double)scale * D / Nn;
        lambda = v < 1.0 ? v : 1.0;
    }
    const double a = (double)alpha_min;
    return (float)(a + lambda * (1.0 - a));
}

// The nearest pixel of the previous image to (xr, yr); false when it lies outside the W x H image (or a coordinate is NaN).
PT_AD_HD bool lookup_pixel(double xr, double yr, unsigned W, unsigned H, unsigned* xi, unsigned* yi) {
    const double fx = __builtin_floor(xr + 0.5), fy = __builtin_floor(yr + 0.5);
    if (!(fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H)) return false;
    *xi = (unsigned)fx;
    *yi = (unsigned)fy;
    return true;
}

}  // namespace ptgr
