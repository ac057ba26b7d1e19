// pt_bake.h -- the rule of light baking (pt_bake_lightmap_device, pt_bake_probes_device, pt_sh_project_device), written
// once for the kernels (BakeSource under the paths and debug-ray forms of pt_kernels_rays.hip, k_bake_mask and k_probe_sh in pt_film_bake.h),
// the host entries (pt_bake.cpp) and the host compilers of the tests.  Build with -ffp-contract=off: no compiler fuses what the
// rule writes apart.
//
// A bake traces rays that start at a surface point or at a point in space instead of a camera.  The path kernels do not know: the
// rays reach them as path states, as the lens and projection rays do (render_injected_impl, pt_api.cpp).  The film of a lightmap
// has one pixel per texel, the film of a probe bake one ROW per probe and one COLUMN per direction.
//
// Texel ray (kind kTexel): one record per texel, float[H][W][6] = point3, normal3.  Sample s of texel (x, y):
//      w = words 0 and 1 of the Philox block camera_ray draws for the key (x, y, s)      r1 = u01(w0)      r2 = u01(w1)
//      nn = normalize(normal), f32, the normalize of the render's arithmetic
//      d = cosine_sample(nn, r1, r2), pt_device.h's sampler and frame      o = point, as it is      throughput 1
//    The film is then the cosine-weighted mean of the incoming radiance, E / pi.
//    EMPTY texel: one of its six numbers is not finite, or the f32 square of the normal's length, fma(nz, nz, fma(ny, ny, nx nx)), is
//    below 1e-36 -- the clamp of the fast normalize: a shorter normal has no direction in that arithmetic -- or not finite (the
//    normal is longer than 1.8e19).  Its ray is o = 0, d = (0, 0, 1), throughput 0: an ordinary ray that contributes nothing, so
//    the render's sample count stays W H spp; k_bake_mask then overwrites its outputs with +0.0 and the black RGBA8 pixel.
//
// Probe ray (kind kProbe): direction r of R, the same for every probe and sample -- a spiral of equal-area z bands:
//      z = 1 - (2 r + 1) / R, in f64, rounded to f32 once (exact whenever R is a power of two)
//      s = sqrt((1 - z)(1 + z)), the product in f64 from the f64 z, rounded to f32, the square root in the render's arithmetic
//      phase word w = (r * 0x9E3779B9) mod 2^32      revolutions = (w >> 8) 2^-24, exact
//      d = (s cos, s sin, z) through sincos2pi, which is called inside (0, 1) only: 0 revolutions is (sin, cos) = (0, 1) without a call
//      o = the probe's position      throughput 1      solid-angle weight 4 pi / R
//    d is not normalised again.  spp > 1 repeats the direction with independent continuations.
//
// SH projection: real spherical harmonics through l = 2, k = l (l + 1) + m, with the constants of Ramamoorthi and Hanrahan,
//      Y0 = 0.282095      Y1 = 0.488603 y      Y2 = 0.488603 z      Y3 = 0.488603 x      Y4 = 1.092548 (x y)      Y5 = 1.092548 (y z)
//      Y6 = 0.315392 (3 (z z) - 1)      Y7 = 1.092548 (x z)      Y8 = 0.546274 (x x - y y)
//    in f64 from the f32 direction of the rule in EXACT arithmetic (struct Exact below), whatever arithmetic traced the rays.
//      sh[p][k][c] = (float)(((4 pi) / R) * S),      S = sum over r of (double)radiance[p][r][c] * Y_k(d_r)
//    S in a fixed order: lane j of 64 sums r = j, j + 64, ... ascending (acc = acc + product, the product rounded first); then the
//    tree  v[j] = v[j] + v[j + h] for j < h,  h = 32, 16, 8, 4, 2, 1;  S = v[0].  Host and device agree bit for bit.
//    One text per piece, for the bake and for the updates over frames (pt_probe_update.h), whose directions are rotated: one ray's
//    nine-by-three terms are sh_add, a lane's share of a bake sh_lane, the tree sh_tree on the host and sh_wave_tree (pt_film_bake.h)
//    on the device, the output word sh_finish.
//
// Irradiance from SH (host): E_c(n) = sum_k A_l sh[k][c] Y_k(n), A = (pi, 2 pi / 3, pi / 4), f64, n normalised in f64 first.
#pragma once
#include <stdint.h>

#include "pt_adaptive.h"      // PT_AD_HD

#if defined(__clang__)
#define PT_BAKE_UNROLL _Pragma("unroll")
#else
#define PT_BAKE_UNROLL
#endif

namespace ptbake {

enum { kTexel = 0, kProbe = 1, kKinds = 2 };
constexpr uint32_t kLanes = 64;
constexpr double kPi = 3.14159265358979323846;

PT_AD_HD bool finite(float v) { return v - v == 0.0f; }

// texel record t[6] = point3, normal3
PT_AD_HD bool empty(const float t[6]) {
    const float len2 = __builtin_fmaf(t[5], t[5], __builtin_fmaf(t[4], t[4], t[3] * t[3]));
    bool ok = len2 >= 1e-36f && finite(len2);
    PT_BAKE_UNROLL
    for (int k = 0; k < 6; ++k) ok = ok && finite(t[k]);
    return !ok;
}

// The render's exact arithmetic where pt_device.h cannot be included (the host; the film unit, which is built in fast mode): IEEE
// division and square root and the statements of pt_device.h's u01, sincos2pi, normalize, frame_of and cosine_sample in their
// exact form.  The GPU tests hold the two together bit for bit (pt_debug_bake_rays against pt_bake_rays_host).
struct Exact {
    static PT_AD_HD float u01(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * (1.0f / 16777216.0f); }      // exact: (2k + 1) / 2^24
    static PT_AD_HD float sqrt(float x) { return __builtin_sqrtf(x); }
    static PT_AD_HD void sincos2pi(float u, float& s, float& c) {
        const float k = __builtin_rintf(u * 4.0f);
        const float r = __builtin_fmaf(k, -0.25f, u);
        const float t = r * 6.28318530717958647692f;
        const float z = t * t;
        const float sp = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
        const float st = __builtin_fmaf(sp * z, t, t);
        const float cp = __builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
        const float ct = __builtin_fmaf(cp * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
        const int q = ((int)k) & 3;
        float ss = (q & 1) ? ct : st;
        float cc = (q & 1) ? st : ct;
        if (q == 1 || q == 2) cc = -cc;
        if (q == 2 || q == 3) ss = -ss;
        s = ss; c = cc;
    }
    static PT_AD_HD void normalize(float v[3]) {
        const float len = __builtin_sqrtf(__builtin_fmaf(v[2], v[2], __builtin_fmaf(v[1], v[1], v[0] * v[0])));
        if (len > 0.0f) {
            const float inv = 1.0f / len;
            v[0] = v[0] * inv; v[1] = v[1] * inv; v[2] = v[2] * inv;
        }
    }
    static PT_AD_HD void cosine_sample(const float n[3], float r1, float r2, float d[3]) {
        float sphi, cphi;
        sincos2pi(r1, sphi, cphi);
        const float cos_theta = __builtin_sqrtf(r2);
        const float sin_theta = __builtin_sqrtf(1.0f - cos_theta * cos_theta);
        const float x = sin_theta * cphi, y = sin_theta * sphi, z = cos_theta;
        // frame_of
        const bool use_x = __builtin_fabsf(n[1]) > 0.999f;
        float t[3] = {use_x ? 0.0f : n[2], use_x ? -n[2] : 0.0f, use_x ? n[1] : -n[0]};
        const float len = __builtin_sqrtf(__builtin_fmaf(t[2], t[2], n[2] * n[2]));
        if (len > 0.0f) {
            const float inv = 1.0f / len;
            t[0] = t[0] * inv; t[1] = t[1] * inv; t[2] = t[2] * inv;
        }
        const float b[3] = {__builtin_fmaf(n[1], t[2], -(n[2] * t[1])), __builtin_fmaf(n[2], t[0], -(n[0] * t[2])),
                            __builtin_fmaf(n[0], t[1], -(n[1] * t[0]))};
        PT_BAKE_UNROLL
        for (int k = 0; k < 3; ++k) d[k] = __builtin_fmaf(n[k], z, __builtin_fmaf(b[k], y, t[k] * x));
        normalize(d);
    }
};

// The ray of one sample of a texel from the two words of its block; *tp: the throughput (1, or 0 for an empty texel)
template <class M>
PT_AD_HD void texel_ray(const float t[6], uint32_t w0, uint32_t w1, float o[3], float d[3], float* tp) {
    // no branch: an empty texel's arithmetic runs on the normal (0, 0, 1) and nothing of it is kept
    const bool e = empty(t);
    float n[3] = {e ? 0.0f : t[3], e ? 0.0f : t[4], e ? 1.0f : t[5]};
    float dd[3];
    M::normalize(n);
    M::cosine_sample(n, M::u01(w0), M::u01(w1), dd);
    o[0] = e ? 0.0f : t[0]; o[1] = e ? 0.0f : t[1]; o[2] = e ? 0.0f : t[2];
    d[0] = e ? 0.0f : dd[0]; d[1] = e ? 0.0f : dd[1]; d[2] = e ? 1.0f : dd[2];
    *tp = e ? 0.0f : 1.0f;
}

// revolutions of direction r's phase, in [0, 1)
PT_AD_HD float probe_phase(uint32_t r) { return (float)((r * 0x9E3779B9u) >> 8) * (1.0f / 16777216.0f); }

// Direction r of R (r < R)
template <class M>
PT_AD_HD void probe_dir(uint32_t r, uint32_t R, float d[3]) {
    const double q = (double)(2u * r + 1u) / (double)R;
    const double z = 1.0 - q;
    const double lo = 1.0 - z, hi = 1.0 + z;
    const double s2 = lo * hi;
    const float s = M::sqrt((float)s2);
    const float rev = probe_phase(r);
    float sn = 0.0f, cs = 1.0f;
    if (rev != 0.0f) M::sincos2pi(rev, sn, cs);
    d[0] = s * cs; d[1] = s * sn; d[2] = (float)z;
}

// Y_k of a direction, k = l (l + 1) + m
PT_AD_HD void sh_basis(double x, double y, double z, double Y[9]) {
    const double xy = x * y, yz = y * z, zz = z * z, xz = x * z, xx = x * x, yy = y * y;
    const double z3 = 3.0 * zz;
    Y[0] = 0.282095;
    Y[1] = 0.488603 * y;
    Y[2] = 0.488603 * z;
    Y[3] = 0.488603 * x;
    Y[4] = 1.092548 * xy;
    Y[5] = 1.092548 * yz;
    Y[6] = 0.315392 * (z3 - 1.0);
    Y[7] = 1.092548 * xz;
    Y[8] = 0.546274 * (xx - yy);
}

// one ray's terms into a lane's 27 sums: d = the ray's f32 direction widened, rad = its radiance
PT_AD_HD void sh_add(const double d[3], const float rad[3], double acc[27]) {
    double Y[9];
    sh_basis(d[0], d[1], d[2], Y);
    const double v[3] = {(double)rad[0], (double)rad[1], (double)rad[2]};
    PT_BAKE_UNROLL
    for (int k = 0; k < 9; ++k)
        PT_BAKE_UNROLL
        for (int c = 0; c < 3; ++c) {
            const double p = v[c] * Y[k];
            acc[3 * k + c] = acc[3 * k + c] + p;
        }
}

// lane `lane`'s share of one probe's 27 sums; rad = the probe's float[R][3]
PT_AD_HD void sh_lane(uint32_t lane, uint32_t R, const float* rad, double acc[27]) {
    PT_BAKE_UNROLL
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (uint32_t r = lane; r < R; r += kLanes) {
        float d[3];
        probe_dir<Exact>(r, R, d);
        const double dd[3] = {(double)d[0], (double)d[1], (double)d[2]};
        sh_add(dd, rad + 3 * (size_t)r, acc);
    }
}

// the output word of a finished sum
PT_AD_HD float sh_finish(double sum, uint32_t R) {
    const double scale = (4.0 * kPi) / (double)R;
    return (float)(scale * sum);
}

// The rule's tree over the lanes' sums on the CPU: S = v[0] afterwards
inline void sh_tree(double v[kLanes][27]) {
    for (uint32_t h = kLanes / 2; h >= 1; h /= 2)
        for (uint32_t j = 0; j < h; ++j)
            for (int k = 0; k < 27; ++k) v[j][k] = v[j][k] + v[j + h][k];
}

// The whole projection of one probe on the CPU, in the kernel's order: out27 = [k][c]
inline void sh_project_probe(uint32_t R, const float* rad, float out27[27]) {
    double v[kLanes][27];
    for (uint32_t j = 0; j < kLanes; ++j) sh_lane(j, R, rad, v[j]);
    sh_tree(v);
    for (int k = 0; k < 27; ++k) out27[k] = sh_finish(v[0][k], R);
}

// E(n) of one normal from sh27 = [k][c], f64; a normal of length 0 or not finite gives 0
inline void sh_irradiance(const float sh27[27], const float n3[3], float out3[3]) {
    const double x = (double)n3[0], y = (double)n3[1], z = (double)n3[2];
    const double len = __builtin_sqrt(x * x + y * y + z * z);
    out3[0] = out3[1] = out3[2] = 0.0f;
    if (!(len > 0.0) || !(len - len == 0.0)) return;
    double Y[9];
    sh_basis(x / len, y / len, z / len, Y);
    const double A[3] = {kPi, 2.0 * kPi / 3.0, kPi / 4.0};
    for (int c = 0; c < 3; ++c) {
        double e = 0.0;
        for (int k = 0; k < 9; ++k) e = e + (A[k == 0 ? 0 : (k < 4 ? 1 : 2)] * (double)sh27[3 * k + c]) * Y[k];
        out3[c] = (float)e;
    }
}

}  // namespace ptbake
