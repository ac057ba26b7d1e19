// pt_probe_update.h -- the rule of the irradiance volume's updates over frames (pt_probe_grid_update_device, pt_probe_blend_*,
// DESIGN.md 5u): the temporal half of Majercik et al. 2019.  Each call re-traces a subset of the probes with few rays along a
// freshly rotated direction set and blends the result into the stored SH coefficients and moment maps with a per-probe hysteresis.
// Written once for the kernels (ProbeUpdateSource in pt_kernels_rays.hip, k_probe_update in pt_film_probe_update.h), the host entries
// (pt_probe_update.cpp) and the host compilers of the tests.  Build with -ffp-contract=off.  f64 where results are blended, with
// + - * /, square root, comparisons and selects in a fixed order; no libm on the device side of the rule.
//
// Slots: a call with (first, stride) updates the probes p = first + k stride < P, k = 0, 1, ...; slot k is probe first + k stride,
// n_upd = ceil((P - first) / stride).  The film of an update has one ROW per slot and one COLUMN per direction: float[n_upd][R][3],
// the distances float[n_upd][R].
//
// Ray of slot k, direction r of R: o = the probe's position by the grid rule (ptgrid::position: f64, rounded to f32 once);
//      d = ptbake::probe_dir<M>(r, R) in the render's arithmetic;  d'_a = fma(M[a][2], d_2, fma(M[a][1], d_1, M[a][0] d_0)), f32,
//      not normalised again.  When `rotation` is bit for bit the identity (1.0f on the diagonal, +0.0f elsewhere), d' = d by a
//      select, not by the multiplication.  Throughput 1, solid-angle weight 4 pi / R.
// New SH of a slot: pt_bake.h's projection with Y_k at the rotated direction in EXACT arithmetic (probe_dir<Exact>, the three fmas
//      in f32, widened), in sh_lane's order (64 lanes, r = j, j + 64, ..., then the tree), sh_finish as it is.
// New moments of a slot: ptvis::add_ray / finish as they are over the rotated exact directions, r ascending.
// Blend, per probe, with age = d_age[p]:
//      alpha = 1 when age = 0, else max(1 - (double)h, 1 / ((double)age + 1)): a plain running mean until the floor is reached.
//      change gate (change_threshold > 0, age > 0): L0 = 0.2126 C[0][0] + 0.7152 C[0][1] + 0.0722 C[0][2] of the old and of the
//      new coefficients, f64, from the left; both finite and |L0_new - L0_old| > change_threshold max(L0_old, L0_new, 0):
//      alpha = max(alpha, change_alpha), for every coefficient and moment of the probe.
//      per SH coefficient and moment component, all selects:
//          new not finite:            out = old when age > 0, +0.0 when age = 0
//          else age = 0 or old not finite:  out = new   (old is never multiplied: a NaN of a plane never written does not survive)
//          else                       out = (float)(old + alpha (new - old)) in f64
//      age' = min(age + 1, 65535).
// Probes that are not a slot of the call keep sh27, moments and age bit for bit.
//
// Rotation of a frame (host only): frame 0 is the identity exactly.  Otherwise u_i = (((frame c_i) mod 2^32) >> 8) 2^-24 with
// c = 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35; Shoemake's uniform quaternion q = (sqrt(1 - u0) sin 2 pi u1, sqrt(1 - u0) cos 2 pi u1,
// sqrt(u0) sin 2 pi u2, sqrt(u0) cos 2 pi u2) = (x, y, z, w) in f64; the matrix in f64, rounded to f32 once.
#pragma once
#include "pt_probe_vis.h"     // ptvis::clamp_distance, probe_moments; ptgrid; ptbake; pt_probe_params.h: ptupd::Params

namespace ptupd {

constexpr uint32_t kMaxAge = 65535u;

PT_AD_HD uint32_t bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}
PT_AD_HD bool is_identity(const float M[9]) {
    bool id = true;
    PT_BAKE_UNROLL
    for (int k = 0; k < 9; ++k) id = id && bits(M[k]) == ((k == 0 || k == 4 || k == 8) ? 0x3F800000u : 0u);
    return id;
}
// max |M M^T - I| and the determinant, f64 from the f32 entries
PT_AD_HD void orthonormality(const float M[9], double* err, double* det) {
    double m[9], e = 0.0;
    for (int k = 0; k < 9; ++k) m[k] = (double)M[k];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double g = m[3 * a] * m[3 * b] + m[3 * a + 1] * m[3 * b + 1] + m[3 * a + 2] * m[3 * b + 2] - (a == b ? 1.0 : 0.0);
            const double ag = g < 0.0 ? -g : g;
            e = ag > e ? ag : e;
        }
    *err = e;
    *det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// the slots of a call: first < P, stride >= 1 (no sum that could wrap: stride may be anything up to 2^32 - 1)
PT_AD_HD uint32_t slots(uint32_t P, uint32_t first, uint32_t stride) { return 1u + (P - first - 1u) / stride; }

// d' = M d (identity: d itself)
PT_AD_HD void rotate(const float M[9], bool identity, const float d[3], float out[3]) {
    PT_BAKE_UNROLL
    for (int a = 0; a < 3; ++a) {
        const float v = __builtin_fmaf(M[3 * a + 2], d[2], __builtin_fmaf(M[3 * a + 1], d[1], M[3 * a] * d[0]));
        out[a] = identity ? d[a] : v;
    }
}
// direction r of R of an update, in the arithmetic Mth
template <class Mth>
PT_AD_HD void dir(uint32_t r, uint32_t R, const float M[9], bool identity, float out[3]) {
    float d[3];
    ptbake::probe_dir<Mth>(r, R, d);
    rotate(M, identity, d, out);
}
// ray r of R as ptvis::add_ray takes it and as ptbake::sh_add reads it: the rotated exact direction widened, the clamped distance
// (0 where there is no visibility struct).  The one staging of a probe ray: the visibility pass (pt_probe_vis.h) calls it with the
// identity and a distance
PT_AD_HD void stage_ray(uint32_t r, uint32_t R, const float M[9], bool identity, bool with_distance, float t, float max_distance, double ray[4]) {
    float d[3];
    dir<ptbake::Exact>(r, R, M, identity, d);
    ray[0] = (double)d[0]; ray[1] = (double)d[1]; ray[2] = (double)d[2];
    ray[3] = with_distance ? ptvis::clamp_distance(t, max_distance) : 0.0;
}
// New SH of one slot on the CPU from its R staged rays and rad = its float[R][3], in the kernel's order: out27 = [k][c]
inline void sh_project_staged(uint32_t R, const double* rays4, const float* rad, float out27[27]) {
    double v[ptbake::kLanes][27] = {};
    for (uint32_t j = 0; j < ptbake::kLanes; ++j)
        for (uint32_t r = j; r < R; r += ptbake::kLanes) ptbake::sh_add(rays4 + 4 * (size_t)r, rad + 3 * (size_t)r, v[j]);
    ptbake::sh_tree(v);
    for (int k = 0; k < 27; ++k) out27[k] = ptbake::sh_finish(v[0][k], R);
}

// ---- blend
PT_AD_HD double luminance0(const float c[3]) { return 0.2126 * (double)c[0] + 0.7152 * (double)c[1] + 0.0722 * (double)c[2]; }
// the probe's blend weight: old0, new0 = C[0][0..2] of the stored and of the new coefficients
PT_AD_HD double alpha(const Params& u, uint32_t age, const float old0[3], const float new0[3]) {
    if (age == 0u) return 1.0;
    const double floor_w = 1.0 - (double)u.hysteresis, mean_w = 1.0 / ((double)age + 1.0);
    double a = floor_w > mean_w ? floor_w : mean_w;
    if (u.change_threshold > 0.0f) {
        const double lo = luminance0(old0), ln = luminance0(new0);
        const double diff = ln - lo, ad = diff < 0.0 ? -diff : diff;
        double m = lo > ln ? lo : ln;
        m = m > 0.0 ? m : 0.0;
        const bool trip = ptgrid::finite(lo) && ptgrid::finite(ln) && ad > (double)u.change_threshold * m;
        const double ca = (double)u.change_alpha;
        a = (trip && ca > a) ? ca : a;
    }
    return a;
}
PT_AD_HD float blend(float old, float nw, double a, uint32_t age) {
    const double o = (double)old, n = (double)nw;
    const float mixed = (float)(o + a * (n - o));
    const float kept = (age == 0u || !ptgrid::finitef(old)) ? nw : mixed;
    const float lost = age > 0u ? old : 0.0f;
    return ptgrid::finitef(nw) ? kept : lost;
}
PT_AD_HD uint32_t next_age(uint32_t age) { return age >= kMaxAge ? kMaxAge : age + 1u; }

}  // namespace ptupd
