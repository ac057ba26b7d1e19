// pt_projection.h -- the camera projections beyond the pinhole (pt_render_projection_device), written once for the
// kernels (ProjectionSource under the three forms of pt_kernels_rays.hip), the host entries
// (pt_projection.cpp) and the host compilers of the tests (tests/tools/projection_san.cpp).  Build with -ffp-contract=off: no
// compiler fuses what the rule writes apart.
//
// Host side, f64 (setup): from the PtCamera's cached fields, the derivation and the refusals of ptlens::setup
//      C = lower_left + horizontal / 2 + vertical / 2 - origin      Wv = C / |C|      U = horizontal / |horizontal|
//      V = vertical / |vertical|      aspect = |vertical| / |horizontal|
//    and the device receives U, V, Wv, C, aspect and fov_degrees / 720 rounded to f32.  Refused: an unknown kind, a reserved word
//    that is not 0, a fisheye fov_degrees that is not finite or outside (0, 360], a camera with |C| or an axis of length 0 or not
//    finite, or an origin that is not finite.
//
// Per sample, in the render's arithmetic (the struct M: div, sqrt and sincos2pi of pt_device.h on the device), from words 0 and 1
// of the ONE Philox block camera_ray draws for (x, y, sample) -- the pixel jitter (ox, oy), as ever:
//   screen     camera_ray's own statements:  u = (x + ox) / (width - 1)      v = ((height - 1 - y) + oy) / (height - 1)
//              dir = ((lower_left + horizontal u) + vertical v) - origin      then  a = 2 u - 1,  b = 2 v - 1
//   PERSPECTIVE   o = origin      d = normalize(dir): camera_ray, bit for bit
//   ORTHOGRAPHIC  o = origin + (dir - C), the subtraction first, in f32 from the f32 fields      d = Wv as it is (not normalised
//                 again).  The view window is |horizontal| x |vertical| at the camera plane.
//   FISHEYE       equidistant:  bb = b aspect      rho = sqrt(a a + bb bb)      theta = min(rho (fov / 720), 1/2) revolutions
//                 d = normalize(cos Wv + (sin (a / rho)) U + (sin (bb / rho)) V), summed in that order; rho = 0: d = Wv as it is
//                 o = origin.  No masking: the corners see further, to at most 180 degrees off the axis.
//   EQUIRECT      longitude a / 2 revolutions, latitude b / 4 revolutions
//                 d = normalize(cos(lat) (sin(lon) U + cos(lon) Wv) + sin(lat) V)      o = origin
//                 Column 0 looks backwards on the left, the centre column along Wv, rows run from +V (top) to -V.
//   The caller normalises (ray answers whether it has to): the device with the normalize of its arithmetic mode, camera_ray's own.
//
// sincos2pi is documented for arguments in (0, 1) only (pt_device.h), and sincos_rev never calls it outside: for an angle of r
// revolutions,  x = |r|;  x >= 1: x = x - floor(x) (exact: x < 2^23);  x = 0: (sin, cos) = (0, 1) without a call;  otherwise
// (sin, cos) = sincos2pi(x), x in (0, 1);  r < 0: sin = -sin (the sine is odd, the cosine even).  The angles of the rule lie in
// [0, 1/2] (theta), (-1/2, 3/2] (longitude; u exceeds 1 in the last column) and (-1/4, 3/4] (latitude).
#pragma once
#include <math.h>
#include <stdint.h>

#include "pt_adaptive.h"      // PT_AD_HD

namespace ptproj {

enum { kPerspective = 0, kOrthographic = 1, kFisheye = 2, kEquirect = 3, kKinds = 4 };
enum { kOk = 0, kBadKind = 1, kBadReserved = 2, kBadFov = 3, kBadCamera = 4 };

struct Setup { float u[3], v[3], w[3], c[3], aspect, fov720; };     // what the device receives

PT_AD_HD bool finite(double v) { return v - v == 0.0; }
PT_AD_HD double len3(const double* v) { return __builtin_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// the host side; *out is written only when the answer is kOk
PT_AD_HD int setup(const double origin[3], const double lower_left[3], const double horizontal[3], const double vertical[3], uint32_t kind,
                   uint32_t reserved, double fov_degrees, Setup* out) {
    if (kind >= (uint32_t)kKinds) return kBadKind;
    if (reserved != 0u) return kBadReserved;
    if (kind == (uint32_t)kFisheye && (!finite(fov_degrees) || !(fov_degrees > 0.0) || !(fov_degrees <= 360.0))) return kBadFov;
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = lower_left[k] + horizontal[k] / 2.0 + vertical[k] / 2.0 - origin[k];
    const double d = len3(c), h = len3(horizontal), v = len3(vertical);
    if (!finite(d) || !finite(h) || !finite(v) || !(d > 0.0) || !(h > 0.0) || !(v > 0.0)) return kBadCamera;
    for (int k = 0; k < 3; ++k) if (!finite(origin[k])) return kBadCamera;
    for (int k = 0; k < 3; ++k) {
        out->u[k] = (float)(horizontal[k] / h);
        out->v[k] = (float)(vertical[k] / v);
        out->w[k] = (float)(c[k] / d);
        out->c[k] = (float)c[k];
    }
    out->aspect = (float)(v / h);
    out->fov720 = kind == (uint32_t)kFisheye ? (float)(fov_degrees / 720.0) : 0.0f;
    return kOk;
}

// camera_ray's statements up to `dir`, from the jitter (ox, oy) of pixel (px, py) of a width x height image
template <class M>
PT_AD_HD void screen(const float origin[3], const float lower_left[3], const float horizontal[3], const float vertical[3], uint32_t width,
                     uint32_t height, uint32_t px, uint32_t py, float ox, float oy, float* u, float* v, float dir[3]) {
    const float wm1 = (float)(width - 1u), hm1 = (float)(height - 1u);
    *u = M::div((float)px + ox, wm1);
    *v = M::div((float)(height - 1u - py) + oy, hm1);
    for (int k = 0; k < 3; ++k) dir[k] = ((lower_left[k] + horizontal[k] * *u) + vertical[k] * *v) - origin[k];
}

// sin and cos of r revolutions through M::sincos2pi, which is called for arguments in (0, 1) only (the reduction: above)
template <class M>
PT_AD_HD void sincos_rev(float r, float& s, float& c) {
    float x = __builtin_fabsf(r);
    if (x >= 1.0f) x = x - __builtin_floorf(x);
    if (x == 0.0f) { s = 0.0f; c = 1.0f; }
    else M::sincos2pi(x, s, c);
    if (r < 0.0f) s = -s;
}

// One kind's ray from the screen position: o and d; the answer is whether the caller has to normalise d.  KIND is a template
// argument: a kernel branches on the (wave-uniform) kind once, around the whole per-lane rule.
template <class M, int KIND>
PT_AD_HD bool ray(const Setup& P, const float origin[3], float u, float v, const float dir[3], float o[3], float d[3], float* a_out,
                  float* b_out) {
    const float a = 2.0f * u - 1.0f, b = 2.0f * v - 1.0f;
    *a_out = a; *b_out = b;
    if (KIND == kOrthographic) {
        for (int k = 0; k < 3; ++k) { o[k] = origin[k] + (dir[k] - P.c[k]); d[k] = P.w[k]; }
        return false;
    }
    for (int k = 0; k < 3; ++k) o[k] = origin[k];
    if (KIND == kFisheye) {
        const float bb = b * P.aspect;
        const float rho = M::sqrt(a * a + bb * bb);
        if (rho == 0.0f) {
            for (int k = 0; k < 3; ++k) d[k] = P.w[k];
            return false;
        }
        const float theta = __builtin_fminf(rho * P.fov720, 0.5f);
        float s, c;
        sincos_rev<M>(theta, s, c);
        const float su = s * M::div(a, rho), sv = s * M::div(bb, rho);
        for (int k = 0; k < 3; ++k) d[k] = (c * P.w[k] + su * P.u[k]) + sv * P.v[k];
        return true;
    }
    if (KIND == kEquirect) {
        float sl, cl, sp, cp;
        sincos_rev<M>(0.5f * a, sl, cl);
        sincos_rev<M>(0.25f * b, sp, cp);
        for (int k = 0; k < 3; ++k) d[k] = cp * (sl * P.u[k] + cl * P.w[k]) + sp * P.v[k];
        return true;
    }
    for (int k = 0; k < 3; ++k) d[k] = dir[k];
    return true;
}

}  // namespace ptproj
