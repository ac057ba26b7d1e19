// pt_film_temporal.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_film_denoise.h"
#include "pt_gradient.h"

// ------------------------------------------------------------------ temporal accumulation (pt_denoise_temporal_device, ..._motion_device, ..._alpha_device)
// The rule is stated in include/pathtrace_amd.h (PtTemporal) and DESIGN.md 5c.  One thread per pixel, in place of k_denoise_init.
// The reprojection runs in f64: an f32 solve puts x' about 1e-4 pixel off at 1024^2, and a bilinear tap of that weight moves
// a dim pixel next to a bright one by far more than the accumulation's own rounding.  Everything after it is f32.
//
// The rule is written once, tm_accumulate, over three compile-time forms; each kernel is one call of it.
//   Plain   k_denoise_temporal: rules 1-7.  No ids: every pixel's map is the identity and the history's id lane gets 0.
//   Motion  k_denoise_temporal_motion: rules 1', 2', 3' and 7' (DESIGN.md 5d).  The pixel's point goes back along its object's
//           motion map (f64) before the camera reprojection, the normal gate takes the normal carried by that map, a tap of
//           another object's history is taken only when neither object moved, and the history keeps id + 1.
//   Alpha   k_denoise_temporal_alpha: Motion with rule 4's least blend weight taken from alpha[p] where that entry is finite
//           and in [0, 1], t.alpha elsewhere.
// A form's additions stand under `if constexpr`; what is outside is every form's.  Each float and double value sees the same
// operations in the same order in every form that computes it, and nothing is contracted or reassociated, so a Motion pixel
// whose map is the identity (the unknown ids Plain stores, or a scene in which nothing moved) gets Plain's bits, and Alpha with
// a plane that holds no usable entry, or one constant c against t.alpha = c, gets Motion's.
namespace PTK_IMPL {
PT_DEV double tm_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PT_DEV void tm_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// pixel (x, y) at depth d seen from the frame's camera, its point P carried to the history pose by mp first (mp null: the
// identity, P as it is) -> (x', y') in the history's image and d_exp; false: no reprojection
PT_DEV bool tm_reproject(const TemporalArgs& a, const MotionMap* mp, uint32_t x, uint32_t y, float d, double& xr, double& yr, double& dexp) {
    const double* o = a.cur; const double* l = a.cur + 3; const double* hz = a.cur + 6; const double* vt = a.cur + 9;
    const double* o2 = a.prev; const double* l2 = a.prev + 3; const double* hz2 = a.prev + 6; const double* vt2 = a.prev + 9;
    const double W1 = (double)(a.dn.width - 1u), H1 = (double)(a.dn.height - 1u);
    const double s = ((double)x + 0.5) / W1, t = ((double)(a.dn.height - 1u - y) + 0.5) / H1;      // camera.rs:139-147, world.rs:299
    double D[3], P[3], c[3], r[3], bc[3], rc[3], br[3];
    for (int k = 0; k < 3; ++k) D[k] = l[k] + s * hz[k] + t * vt[k] - o[k];
    const double inv_len = 1.0 / __builtin_sqrt(tm_dot(D, D));
    for (int k = 0; k < 3; ++k) P[k] = o[k] + (double)d * (D[k] * inv_len);
    if (mp) {
        double Ph[3];
        for (int k = 0; k < 3; ++k) Ph[k] = mp->a[3 * k] * P[0] + mp->a[3 * k + 1] * P[1] + mp->a[3 * k + 2] * P[2] + mp->b[k];
        for (int k = 0; k < 3; ++k) P[k] = Ph[k];
    }
    for (int k = 0; k < 3; ++k) {
        c[k] = o2[k] - P[k];                 // -(P_h - o')
        r[k] = o2[k] - l2[k];
    }
    // s' hz' + t' vt' + lambda c = r by Cramer's rule
    tm_cross(vt2, c, bc);
    const double det = tm_dot(hz2, bc);
    if (!(det != 0.0) || !__builtin_isfinite(det)) return false;
    tm_cross(r, c, rc);
    tm_cross(vt2, r, br);
    const double inv = 1.0 / det;
    const double s2 = tm_dot(r, bc) * inv, t2 = tm_dot(hz2, rc) * inv, lam = tm_dot(hz2, br) * inv;
    if (!(lam > 0.0) || !__builtin_isfinite(s2) || !__builtin_isfinite(t2) || !__builtin_isfinite(lam)) return false;
    xr = s2 * W1 - 0.5;
    yr = (double)a.dn.height - 0.5 - t2 * H1;
    dexp = __builtin_sqrt(tm_dot(c, c));
    return true;
}

enum class Temporal { Plain, Motion, Alpha };
// m: the ids and maps of Motion and Alpha (Plain: unused); alpha: Alpha's plane (the others: unused)
template <Temporal F>
PT_DEV void tm_accumulate(const TemporalArgs& a, const TemporalMotionArgs* m, const float* alpha) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.dn.width || y >= a.dn.height) return;
    const int W = (int)a.dn.width, H = (int)a.dn.height;
    const size_t p = (size_t)y * a.dn.width + x;
    const float4 f0p = a.dn.feat[2 * p], f1p = a.dn.feat[2 * p + 1];
    const float3 uc = dn_demod(a.dn, p);
    const float Lc = dn_lum(uc.x, uc.y, uc.z);
    // the pixel's map: bit 0 identity, bit 1 invalid (no history).  Plain has no ids: the identity, as constants
    int32_t id = -1;
    uint32_t flags = 1u;
    float idf = 0.0f;
    if constexpr (F != Temporal::Plain) {      // the caller's id: checked against the scene before it indexes the maps
        id = m->ids[p];
        const bool known = id >= 0 && (uint32_t)id < m->n_objs;
        flags = known ? m->maps[id].flags : 2u;
        idf = known ? (float)(id + 1) : 0.0f;  // n_objs <= 2^24 - 2: exact
    }
    const bool ident = flags == 1u;
    // the valid-weighted history of the 2 x 2 bilinear taps around (x', y')
    float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hm1 = 0.0f, hm2 = 0.0f, hn = 0.0f;
    if (a.hist_src && f1p.w > 0.0f && !(flags & 2u)) {
        double xr = x, yr = y, dexp = f1p.w;
        float nx = f1p.x, ny = f1p.y, nz = f1p.z;
        bool ok = true;
        if (!(ident && a.same_camera)) {
            const MotionMap* mp = nullptr;
            if constexpr (F != Temporal::Plain) mp = ident ? nullptr : m->maps + id;
            ok = tm_reproject(a, mp, x, y, f1p.w, xr, yr, dexp);
            if (mp) {                         // n_h = A n_p, normalised in f64 (n_p when its length is 0)
                double v[3];
                for (int k = 0; k < 3; ++k) v[k] = mp->a[3 * k] * (double)f1p.x + mp->a[3 * k + 1] * (double)f1p.y + mp->a[3 * k + 2] * (double)f1p.z;
                const double len = __builtin_sqrt(tm_dot(v, v));
                if (len > 0.0) { nx = (float)(v[0] / len); ny = (float)(v[1] / len); nz = (float)(v[2] / len); }
            }
        }
        if (ok && xr > -1.0 && xr < (double)W && yr > -1.0 && yr < (double)H) {      // else no tap lies inside the image
            const int x0 = (int)__builtin_floor(xr), y0 = (int)__builtin_floor(yr);
            const float fx = (float)(xr - x0), fy = (float)(yr - y0);
            const float de = (float)dexp, dmax = a.depth_tol * de;
            const bool em = f0p.w > 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int qx = x0 + i, qy = y0 + j;
                    const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                    if (!(w > 0.0f) || qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    const float4 h2 = a.hist_src[3 * q + 2];
                    if (!(h2.w > 0.0f) || !(fabsf(h2.w - de) <= dmax)) continue;
                    if (!(nx * h2.x + ny * h2.y + nz * h2.z >= a.normal_tol)) continue;
                    const float4 h1 = a.hist_src[3 * q + 1];
                    if (em != (h1.z > 0.0f)) continue;
                    if constexpr (F != Temporal::Plain) {
                        if (h1.w != 0.0f && h1.w != idf) {       // another object's history: only when neither object moved
                            if (!ident || !(h1.w >= 1.0f && h1.w <= (float)m->n_objs)) continue;
                            if (m->maps[(uint32_t)h1.w - 1u].flags != 1u) continue;
                        }
                    }
                    const float4 h0 = a.hist_src[3 * q];
                    S += w;
                    hr += w * h0.x; hg += w * h0.y; hb += w * h0.z; hm1 += w * h0.w;
                    hm2 += w * h1.x; hn += w * h1.y;
                }
        }
    }
    float3 u = uc;
    float m1 = Lc, m2 = Lc * Lc, n = 1.0f;            // a fresh pixel
    if (S >= 1e-2f) {
        const float inv = 1.0f / S;
        const float ur = hr * inv, ug = hg * inv, ub = hb * inv, um1 = hm1 * inv, um2 = hm2 * inv;
        n = hn * inv + 1.0f;
        float least = a.alpha;
        if constexpr (F == Temporal::Alpha) {
            const float ap = alpha[p];
            least = ap >= 0.0f && ap <= 1.0f ? ap : a.alpha;      // (NaN fails both comparisons)
        }
        const float al = fmaxf(least, 1.0f / n);
        u = make_float3(ur + al * (uc.x - ur), ug + al * (uc.y - ug), ub + al * (uc.z - ub));
        m1 = um1 + al * (Lc - um1);
        m2 = um2 + al * (Lc * Lc - um2);
    }
    const float var = n >= 4.0f ? fmaxf(0.0f, m2 - m1 * m1) : dn_spatial_var(a.dn, x, y);
    a.hist_dst[3 * p] = make_float4(u.x, u.y, u.z, m1);
    a.hist_dst[3 * p + 1] = make_float4(m2, n, f0p.w, idf);
    a.hist_dst[3 * p + 2] = f1p;
    if (a.dn.finalize) dn_store(a.dn, p, u.x, u.y, u.z, f0p);
    else a.dn.dst[p] = make_float4(u.x, u.y, u.z, var);
}
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal(TemporalArgs a) { tm_accumulate<Temporal::Plain>(a, nullptr, nullptr); }
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal_motion(TemporalMotionArgs m) { tm_accumulate<Temporal::Motion>(m.t, &m, nullptr); }
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal_alpha(TemporalAlphaArgs g) { tm_accumulate<Temporal::Alpha>(g.m.t, &g.m, g.alpha); }
}  // namespace PTK_IMPL
namespace ptk {
void launch_denoise_temporal(const TemporalArgs& a, hipStream_t st) {
    const dim3 g = dn_grid(a.dn.width, a.dn.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal, g, b, 0, st, a);
}
void launch_denoise_temporal_motion(const TemporalMotionArgs& a, hipStream_t st) {
    const dim3 g = dn_grid(a.t.dn.width, a.t.dn.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal_motion, g, b, 0, st, a);
}
void launch_denoise_temporal_alpha(const TemporalAlphaArgs& a, hipStream_t st) {
    const dim3 g = dn_grid(a.m.t.dn.width, a.m.t.dn.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal_alpha, g, b, 0, st, a);
}
}  // namespace ptk

// ------------------------------------------------------------------ temporal gradients (pt_temporal_gradient_device)
// The rule is pt_gradient.h and DESIGN.md 5h: one gradient pixel per 3 x 3 stratum, re-traced in the current scene with the
// previous frame's samples (a pixel-list render between k_gradient_list and k_gradient_strata), its change of luminance
// spread over a window of strata into every pixel's blend weight (the plane k_denoise_temporal_alpha takes).  f64 + - * /
// and comparisons only: the same bits as the host compiler's.
namespace PTK_IMPL {
// one thread per stratum: its gradient pixel, list slot = by * SW + bx
__global__ void __launch_bounds__(kBlock) k_gradient_list(GradientArgs a) {
    const uint32_t SW = ptgr::strata(a.width), SH = ptgr::strata(a.height);
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= SW * SH) return;
    uint32_t x, y;
    ptgr::stratum_pixel(s % SW, s / SW, a.width, a.height, a.seed, &x, &y);
    a.list[s] = make_uint2(x, y);
}
// one thread per stratum: the record of its gradient pixel
__global__ void __launch_bounds__(kBlock) k_gradient_strata(GradientArgs a) {
    const uint32_t SW = ptgr::strata(a.width), SH = ptgr::strata(a.height);
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= SW * SH) return;
    uint32_t x, y;
    ptgr::stratum_pixel(s % SW, s / SW, a.width, a.height, a.seed, &x, &y);
    const size_t p = (size_t)y * a.width + x;
    const float cn[3] = {a.retraced[3 * (size_t)s], a.retraced[3 * (size_t)s + 1], a.retraced[3 * (size_t)s + 2]};
    const float co[3] = {a.prev[3 * p], a.prev[3 * p + 1], a.prev[3 * p + 2]};
    double rec[2];
    ptgr::stratum_record(cn, co, rec);
    a.rec[2 * (size_t)s] = rec[0]; a.rec[2 * (size_t)s + 1] = rec[1];
}
// one thread per pixel: its window of records -> alpha_p
__global__ void __launch_bounds__(kDnBx * kDnBy) k_gradient_alpha(GradientArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    a.alpha[(size_t)y * a.width + x] = ptgr::pixel_alpha(a.rec, ptgr::strata(a.width), ptgr::strata(a.height), x, y, a.radius, a.scale, a.alpha_min);
}
// ... under a moving camera: the records are those of the previous frame's image; the pixel's first-hit point
// goes through tm_reproject (f64, the temporal kernels' lookup, no motion map) to the previous-image pixel whose stratum
// measured it.  One float4 of features, the solve, then the window of 16-byte records; NaN where there is nothing to look up.
__global__ void __launch_bounds__(kDnBx * kDnBy) k_gradient_alpha_camera(GradientArgs a, TemporalArgs t) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    uint32_t xi = x, yi = y;
    bool ok = true;
    if (!t.same_camera) {
        const float d = t.dn.feat[2 * p + 1].w;
        double xr = 0.0, yr = 0.0, dexp = 0.0;
        ok = d > 0.0f && tm_reproject(t, nullptr, x, y, d, xr, yr, dexp) && ptgr::lookup_pixel(xr, yr, a.width, a.height, &xi, &yi);
    }
    a.alpha[p] = ok ? ptgr::pixel_alpha(a.rec, ptgr::strata(a.width), ptgr::strata(a.height), xi, yi, a.radius, a.scale, a.alpha_min)
                    : __builtin_nanf("");
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_gradient_list(const GradientArgs& a, hipStream_t st) {
    const uint32_t ns = ptgr::strata(a.width) * ptgr::strata(a.height);
    if (ns) hipLaunchKernelGGL(PTK_IMPL::k_gradient_list, dim3((ns + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_gradient_strata(const GradientArgs& a, hipStream_t st) {
    const uint32_t ns = ptgr::strata(a.width) * ptgr::strata(a.height);
    if (ns) hipLaunchKernelGGL(PTK_IMPL::k_gradient_strata, dim3((ns + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_gradient_alpha(const GradientArgs& a, hipStream_t st) {
    const dim3 g = dn_grid(a.width, a.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_gradient_alpha, g, b, 0, st, a);
}
void launch_gradient_alpha_camera(const GradientArgs& a, const TemporalArgs& t, hipStream_t st) {
    const dim3 g = dn_grid(a.width, a.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_gradient_alpha_camera, g, b, 0, st, a, t);
}
}  // namespace ptk
