// pt_lens.h -- the thin-lens camera (pt_render_lens_device), written once for the kernels (LensSource
// under the three forms of pt_kernels_rays.hip), the host entries (pt_lens.cpp) and the host compilers of the
// tests (tests/tools/lens_san.cpp).  Build with -ffp-contract=off: no compiler fuses what the rule writes apart.
//
// Host side, f64 (setup): from the PtCamera's cached fields
//      C = lower_left + horizontal / 2 + vertical / 2 - origin      D = |C|      U = horizontal / |horizontal|,  V = vertical / |vertical|
//      inv_phi = D / focus_distance       Lu = (aperture / 2) U      Lv = (aperture / 2) V
//    and the device receives Lu, Lv and inv_phi rounded to f32.  A camera with D or an axis of length 0 or not finite is refused,
//    and so is an aperture that is negative or not finite and a focus_distance that is not finite or not > 0.
//
// Per sample, in the render's arithmetic (the struct M: div and sincos2pi of pt_device.h on the device), from the words dc[0..3]
// of the ONE Philox block camera_ray draws -- (px, py, sample, kDepthCamera, BLK_SURFACE); dc[0], dc[1] are the pixel jitter as
// ever, dc[2], dc[3], spare until now, are the lens point -- and `dir`, camera_ray's direction before it is normalised:
//   1. (a, b) = 2 u01(dc[2]) - 1, 2 u01(dc[3]) - 1: exact in f32, and never 0 (u01 is an odd multiple of 2^-24).
//   2. Shirley's concentric map, the angle in revolutions for sincos2pi:
//        |a| > |b|:  r = a, rev = (b / a) / 8        else:  r = b, rev = 1/4 - (a / b) / 8        (dx, dy) = (r cos, r sin)
//   3. l = dx Lu + dy Lv        o' = origin + l        d' = normalize(dir - l inv_phi)   (the caller normalises: camera_ray's own)
// Aperture 0: Lu = Lv = 0 exactly, l = +-0, and the ray is camera_ray's bit for bit (a component of origin or dir that is -0
// excepted: it comes out +0).  Aperture > 0: o' + t d' passes origin + dir / inv_phi, the point of the jittered screen position on
// the plane at focus_distance along the view axis, whatever the lens point.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pt_adaptive.h"      // PT_AD_HD

namespace ptlens {

struct Setup { float lu[3], lv[3], inv_phi; };     // what the device receives

enum { kOk = 0, kBadAperture = 1, kBadFocus = 2, kBadCamera = 3 };

PT_AD_HD bool finite(double v) { return v - v == 0.0; }
PT_AD_HD double len3(const double* v) { return __builtin_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// the host side; *out is written only when the answer is kOk
PT_AD_HD int setup(const double origin[3], const double lower_left[3], const double horizontal[3], const double vertical[3],
                   double aperture, double focus_distance, Setup* out) {
    if (!finite(aperture) || !(aperture >= 0.0)) return kBadAperture;
    if (!finite(focus_distance) || !(focus_distance > 0.0)) return kBadFocus;
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = lower_left[k] + horizontal[k] / 2.0 + vertical[k] / 2.0 - origin[k];
    const double d = len3(c), h = len3(horizontal), v = len3(vertical);
    if (!finite(d) || !finite(h) || !finite(v) || !(d > 0.0) || !(h > 0.0) || !(v > 0.0)) return kBadCamera;
    for (int k = 0; k < 3; ++k) if (!finite(origin[k])) return kBadCamera;
    const double half = aperture / 2.0;
    for (int k = 0; k < 3; ++k) {
        out->lu[k] = (float)(half * (horizontal[k] / h));
        out->lv[k] = (float)(half * (vertical[k] / v));
    }
    out->inv_phi = (float)(d / focus_distance);
    return kOk;
}

// rules 1 and 2: the lens point of the two words' uniforms u2 = u01(dc[2]), u3 = u01(dc[3])
template <class M>
PT_AD_HD void disc(float u2, float u3, float* dx, float* dy) {
    const float a = 2.0f * u2 - 1.0f, b = 2.0f * u3 - 1.0f;
    float r, rev;
    if (__builtin_fabsf(a) > __builtin_fabsf(b)) { r = a; rev = 0.125f * M::div(b, a); }
    else { r = b; rev = 0.25f - 0.125f * M::div(a, b); }
    float s, c;
    M::sincos2pi(rev, s, c);
    *dx = r * c; *dy = r * s;
}

// rule 3 without the normalisation: o = o', d = dir - l inv_phi
PT_AD_HD void ray(const Setup& L, const float origin[3], const float dir[3], float dx, float dy, float o[3], float d[3]) {
    for (int k = 0; k < 3; ++k) {
        const float l = dx * L.lu[k] + dy * L.lv[k];
        o[k] = origin[k] + l;
        d[k] = dir[k] - l * L.inv_phi;
    }
}

}  // namespace ptlens
