// pt_probe_vis.h -- the rule of the irradiance volume's probe visibility (pt_probe_moments_*, pt_probe_shade_visibility_*,
// pt_render_probe_lit_visibility_*): the depth moments and the Chebyshev test of Majercik et al. 2019, the half of that
// paper's probe weight that PT_PROBE_WEIGHT_FACING leaves out.  Written once for the kernels (k_probe_moments and k_probe_shade_vis in
// pt_film_probe_vis.h), the host entries (pt_probe_grid.cpp) and the host compilers of the tests.  Build with -ffp-contract=off.  f64
// with + - * /, square root, comparisons and selects in a fixed order; no libm.  Every texel, corner and ray quantity is formed in
// f64; f32 inputs are widened first.  |x| is x < 0 ? -x : x, sgn x is x >= 0 ? +1 : -1 (sgn 0 = +1), dot(a, b) = a0 b0 + a1 b1 + a2 b2
// from the left.
//
// Map: every probe has T x T texels, T = resolution in [2, 16], of two floats (m1, m2): float[P][T][T][2], texel (i, j) of probe p
// at ((p T + j) T + i) 2.  Texel (i, j) has the centre u = ((i + 0.5) 2) / T - 1, v likewise from j.
//   oct_decode(u, v): z = (1 - |u|) - |v|; z >= 0: (x, y) = (u, v), else x = (1 - |v|) sgn u, y = (1 - |u|) sgn v;
//                     inv = 1 / sqrt(dot(d, d)); n = (x inv, y inv, z inv).
//   oct_encode(d):    s = (|x| + |y|) + |z|, a = x / s, b = y / s; z < 0: u = (1 - |b|) sgn a, v = (1 - |a|) sgn b, else (u, v) = (a, b).
//   wrap: no border is stored.  A tap (i, j) outside the map on one axis mirrors along that edge: (-1, j) -> (0, T-1-j),
//         (T, j) -> (T-1, T-1-j), (i, -1) -> (T-1-i, 0), (i, T) -> (T-1-i, T-1); outside on both axes it is the diagonally opposite
//         corner texel: (-1, -1) -> (T-1, T-1), (T, -1) -> (0, T-1), (-1, T) -> (T-1, 0), (T, T) -> (0, 0).
//   lookup(u, v):     per axis g = ((u + 1) T) / 2 - 0.5, i0 = floor(g) (-1 when g is not >= 0), at most T - 1; f = g - i0; i1 = i0 + 1.
//                     The four taps through wrap, widened; lerp(a, b, f) = a + f (b - a); along x in row j0 and row j1, then along
//                     y; m1 and m2 each.
//
// Moments of one probe from its R distances t[r] (float; pt_probe_distances_*: the first hit's t, +inf for a miss) with the
// parameters (T, k = sharpness_log2 in [0, 8], max_distance finite and > 0):
//   d_r = ptbake::probe_dir<Exact>(r, R), widened: the directions k_probe_sh uses, whatever arithmetic traced the rays.  (d_r, dist_r)
//   is staged as four doubles by ptupd::stage_ray (pt_probe_update.h) under the identity: the updates stage their rotated rays with it
//   dist_r = t[r] when 0 < t[r] <= max_distance, else max_distance (a miss, +inf, NaN, 0 and negative values)
//   per texel with n = oct_decode(centre):  c = dot(n, d_r);  w = max(c, 0) = c > 0 ? c : 0, then w = w w, k times
//   S0 = S0 + w,  S1 = S1 + w dist_r,  S2 = S2 + w (dist_r dist_r),  from 0.0 with r ASCENDING (no split order: the kernel's time is
//   not in the sums, docs/EXPERIMENTS.md "Irradiance volume: visibility")
//   texel = ((float)(S1 / S0), (float)(S2 / S0)), or (max_distance, (float)(max_distance max_distance) in f64) when S0 == 0.
//   On the CPU a probe's map from its staged rays is probe_moments below, for pt_probe_moments_host and the host update; on the device
//   the pass over the staged rays is probe_staged_rays (pt_film_probe_vis.h), for k_probe_moments and k_probe_update.
//
// Shading: steps 1-3, 5 and 6 of pt_probe_grid.h as they are.  Step 4 of corner j, whatever PtProbeShade.weight says:
//   tri = (wx wy) wz and F = h h + 0.2 as kFacing forms them (its v = pos_j - P from the UNBIASED point).  Then with Q = P +
//   normal_bias nn (all three axes) and pos_j widened:
//   v = Q - pos_j, r = sqrt(dot(v, v)).  vis = 1 when r is not > 0 or not finite.  Else (m1, m2) = lookup(oct_encode(v / r)) in
//   probe j's map; vis = 1 when m1 or m2 is not finite or r <= m1; else var = |m1 m1 - m2|, dl = r - m1, ch = var / (var + dl dl),
//   vis = (ch ch) ch.   g = F vis;  g = g > 1e-6 ? g : 1e-6 (NaN: 1e-6);  g < 0.2: g = ((g g) g) / 0.04.   w_j = tri g.
//   So den > 0 always (tri sums to 1, g > 0), and when every corner has m1 >= r the pixel is PT_PROBE_WEIGHT_FACING's bit for
//   bit: vis = 1, g = F >= 0.2, w_j = tri F.
#pragma once
#include "pt_probe_grid.h"        // (pt_probe_params.h: ptvis::Params)

namespace ptvis {

constexpr uint32_t kMinResolution = 2u, kMaxResolution = 16u, kMaxSharpness = 8u;

PT_AD_HD bool valid(const Params& p) {
    return p.resolution >= kMinResolution && p.resolution <= kMaxResolution && p.sharpness_log2 <= kMaxSharpness && p.max_distance > 0.0f &&
           ptgrid::finitef(p.max_distance);
}

PT_AD_HD double absd(double x) { return x < 0.0 ? -x : x; }
PT_AD_HD double sgn(double x) { return x >= 0.0 ? 1.0 : -1.0; }
PT_AD_HD double centre(uint32_t T, uint32_t i) { return (((double)i + 0.5) * 2.0) / (double)T - 1.0; }

PT_AD_HD void oct_decode(double u, double v, double n[3]) {
    const double au = absd(u), av = absd(v);
    const double z = (1.0 - au) - av;
    const bool up = z >= 0.0;
    const double d[3] = {up ? u : (1.0 - av) * sgn(u), up ? v : (1.0 - au) * sgn(v), z};
    const double inv = 1.0 / __builtin_sqrt(ptgrid::dot3(d, d));
    n[0] = d[0] * inv; n[1] = d[1] * inv; n[2] = d[2] * inv;
}

PT_AD_HD void oct_encode(const double d[3], double* u, double* v) {
    const double s = (absd(d[0]) + absd(d[1])) + absd(d[2]);
    const double a = d[0] / s, b = d[1] / s;
    const bool down = d[2] < 0.0;
    *u = down ? (1.0 - absd(b)) * sgn(a) : a;
    *v = down ? (1.0 - absd(a)) * sgn(b) : b;
}

// the texel a tap (i, j), each in [-1, T], resolves to
PT_AD_HD void wrap(int T, int i, int j, int* wi, int* wj) {
    const bool oi = i < 0 || i >= T, oj = j < 0 || j >= T;
    if (oi && oj) { *wi = i < 0 ? T - 1 : 0; *wj = j < 0 ? T - 1 : 0; }
    else if (oi) { *wi = i < 0 ? 0 : T - 1; *wj = T - 1 - j; }
    else if (oj) { *wi = T - 1 - i; *wj = j < 0 ? 0 : T - 1; }
    else { *wi = i; *wj = j; }
}

// the lower tap and the fraction of one axis
PT_AD_HD void tap(int T, double u, int* i0, double* f) {
    const double g = ((u + 1.0) * (double)T) / 2.0 - 0.5;
    int i = g >= 0.0 ? (int)g : -1;
    if (i > T - 1) i = T - 1;
    *i0 = i; *f = g - (double)i;
}

PT_AD_HD double lerp(double a, double b, double f) { return a + f * (b - a); }

// map = one probe's float[T][T][2]
PT_AD_HD void lookup(const float* map, int T, double u, double v, double* m1, double* m2) {
    int i0, j0;
    double fx, fy;
    tap(T, u, &i0, &fx);
    tap(T, v, &j0, &fy);
    double t[2][2][2];
    PT_BAKE_UNROLL
    for (int dj = 0; dj < 2; ++dj)
        PT_BAKE_UNROLL
        for (int di = 0; di < 2; ++di) {
            int wi, wj;
            wrap(T, i0 + di, j0 + dj, &wi, &wj);
            const float* q = map + 2 * (size_t)(wj * T + wi);
            t[dj][di][0] = (double)q[0]; t[dj][di][1] = (double)q[1];
        }
    const double a1 = lerp(t[0][0][0], t[0][1][0], fx), b1 = lerp(t[1][0][0], t[1][1][0], fx);
    const double a2 = lerp(t[0][0][1], t[0][1][1], fx), b2 = lerp(t[1][0][1], t[1][1][1], fx);
    *m1 = lerp(a1, b1, fy);
    *m2 = lerp(a2, b2, fy);
}

// ---- moments
PT_AD_HD double clamp_distance(float t, float max_distance) {
    const double d = (double)t, m = (double)max_distance;
    return (d > 0.0 && d <= m) ? d : m;
}
// ray = d3, dist
PT_AD_HD void add_ray(const double n[3], const double ray[4], uint32_t k, double S[3]) {
    const double c = ptgrid::dot3(n, ray);
    double w = c > 0.0 ? c : 0.0;
    for (uint32_t s = 0; s < k; ++s) w = w * w;
    S[0] = S[0] + w;
    S[1] = S[1] + w * ray[3];
    S[2] = S[2] + w * (ray[3] * ray[3]);
}
PT_AD_HD void finish(const double S[3], float max_distance, float out[2]) {
    const double m = (double)max_distance;
    const bool none = S[0] == 0.0;
    out[0] = none ? max_distance : (float)(S[1] / S[0]);
    out[1] = none ? (float)(m * m) : (float)(S[2] / S[0]);
}
// The moments of one probe on the CPU from its R staged rays (rays4 = R x (d3, dist): ptupd::stage_ray of pt_probe_update.h), in the
// kernels' order: out = the probe's float[T][T][2]
inline void probe_moments(const Params& p, uint32_t R, const double* rays4, float* out) {
    const uint32_t T = p.resolution;
    for (uint32_t t = 0; t < T * T; ++t) {
        double n[3], S[3] = {0.0, 0.0, 0.0};
        oct_decode(centre(T, t % T), centre(T, t / T), n);
        for (uint32_t r = 0; r < R; ++r) add_ray(n, rays4 + 4 * (size_t)r, p.sharpness_log2, S);
        finish(S, p.max_distance, out + 2 * (size_t)t);
    }
}

// ---- the visibility type of ptgrid::shade_rule
struct MomentMaps {
    static constexpr bool kOn = true;
    const float* moments;     // float[P][T][T][2]
    int T;
    PT_AD_HD double weight(uint32_t probe, const double Q[3], const double pos[3], double tri, double F) const {
        const double v[3] = {Q[0] - pos[0], Q[1] - pos[1], Q[2] - pos[2]};
        const double r = __builtin_sqrt(ptgrid::dot3(v, v));
        double vis = 1.0;
        if (r > 0.0 && ptgrid::finite(r)) {
            const double d[3] = {v[0] / r, v[1] / r, v[2] / r};
            double eu, ev, m1, m2;
            oct_encode(d, &eu, &ev);
            lookup(moments + 2 * (size_t)(T * T) * probe, T, eu, ev, &m1, &m2);
            if (ptgrid::finite(m1) && ptgrid::finite(m2) && !(r <= m1)) {
                const double var = absd(m1 * m1 - m2);
                const double dl = r - m1;
                const double ch = var / (var + dl * dl);
                vis = (ch * ch) * ch;
            }
        }
        double g = F * vis;
        g = g > 1e-6 ? g : 1e-6;
        if (g < 0.2) g = ((g * g) * g) / 0.04;
        return tri * g;
    }
};

// One pixel of pt_probe_shade_visibility_*: ptgrid::shade with the visibility term
PT_AD_HD bool shade(const ptgrid::Grid& g, float normal_bias, uint32_t W, uint32_t H, uint32_t x, uint32_t y, const float rec[8], const double cam[12],
                    const float* sh27, const float* moments, uint32_t resolution, float out[3]) {
    MomentMaps m;
    m.moments = moments; m.T = (int)resolution;
    return ptgrid::shade_rule(g, normal_bias, (uint32_t)ptgrid::kFacing, W, H, x, y, rec, cam, sh27, m, out);
}

}  // namespace ptvis
