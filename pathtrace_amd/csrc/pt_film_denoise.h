// pt_film_denoise.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"

// ------------------------------------------------------------------ edge-avoiding a-trous denoiser (pt_denoise_device)
// The rule is stated in include/pathtrace_amd.h (PtDenoise) and DESIGN.md 5b.  One thread per pixel, one launch per step.
// State plane: float4 (u.rgb, var) per pixel, u = colour / max(albedo, 1e-3); the features: (albedo rgb, emitter),
// (normal xyz, depth).  Every tap is three 16-byte loads; at 1024^2 the 48 MB of the three planes stay in the Infinity Cache.
// The sums are formed as u_p + sum w (u_q - u_p) / sum w (the rule's sum w u_q / sum w): a flat region stays exactly flat.
namespace PTK_IMPL {
constexpr uint32_t kDnBx = 32, kDnBy = 8;      // a wave covers 32 x 2 pixels: its 5 x 5 taps touch few cache lines
PT_DEV float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
PT_DEV float dn_albedo(float a) { return fmaxf(a, 1e-3f); }
// c' = u * a, and the RGBA8 word of c' through k_resolve's gamma / clamp / `as u8` (world.rs:322-331)
PT_DEV void dn_store(const DenoiseArgs& a, size_t p, float ur, float ug, float ub, float4 f0) {
    const float c[3] = {ur * dn_albedo(f0.x), ug * dn_albedo(f0.y), ub * dn_albedo(f0.z)};
    uint32_t q8 = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.out_linear[3 * p + k] = c[k];
        const double gm = __builtin_sqrt((double)c[k]);
        const double cl = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);
        const double q = cl * 255.0;
        q8 |= (uint32_t)((q != q) ? (uint8_t)0 : (uint8_t)q) << (8 * k);
    }
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * p) = q8;
}
// demodulated colour of pixel q straight from the film
PT_DEV float3 dn_demod(const DenoiseArgs& a, size_t q) {
    const float4 f0 = a.feat[2 * q];
    return make_float3(a.linear[3 * q] / dn_albedo(f0.x), a.linear[3 * q + 1] / dn_albedo(f0.y), a.linear[3 * q + 2] / dn_albedo(f0.z));
}
// the 3 x 3 population variance of L(u) around pixel (x, y), taps outside the image skipped: k_denoise_temporal's variance
// of a pixel with fewer than 4 frames of history.  The statements are k_denoise_init's, in its order, so the value is the
// same bits (tests/test_gpu_temporal.py); k_denoise_init keeps its own text because calling this function there changes
// the instructions the compiler schedules for that kernel.
PT_DEV float dn_spatial_var(const DenoiseArgs& a, uint32_t x, uint32_t y) {
    float Ls[9];
    uint32_t cnt = 0;
    float sum = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx, qy = (int)y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) continue;
            const float3 uq = dn_demod(a, (size_t)qy * a.width + qx);
            Ls[cnt] = dn_lum(uq.x, uq.y, uq.z);
            sum += Ls[cnt];
            ++cnt;
        }
    const float mu = sum / (float)cnt;
    float var = 0.0f;
    for (uint32_t k = 0; k < cnt; ++k) var += (Ls[k] - mu) * (Ls[k] - mu);
    var /= (float)cnt;
    return var;
}
// first launch: u and the 3 x 3 population variance of L(u) (taps outside the image skipped); finalize: iterations = 0
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_init(DenoiseArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float3 u = dn_demod(a, p);
    float Ls[9];
    uint32_t cnt = 0;
    float sum = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx, qy = (int)y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) continue;
            const float3 uq = dn_demod(a, (size_t)qy * a.width + qx);
            Ls[cnt] = dn_lum(uq.x, uq.y, uq.z);
            sum += Ls[cnt];
            ++cnt;
        }
    const float mu = sum / (float)cnt;
    float var = 0.0f;
    for (uint32_t k = 0; k < cnt; ++k) var += (Ls[k] - mu) * (Ls[k] - mu);
    var /= (float)cnt;
    if (a.finalize) dn_store(a, p, u.x, u.y, u.z, a.feat[2 * p]);
    else a.dst[p] = make_float4(u.x, u.y, u.z, var);
}
// one a-trous step of size h: the 3 x 3 Gaussian of var (renormalised over the in-image taps) gives g_p, then the 5 x 5
// B3-spline taps at (dx, dy) h with the edge-stopping weights; finalize: remodulate and write both film planes
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_step(DenoiseArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const int W = (int)a.width, H = (int)a.height, h = (int)a.step;
    const size_t p = (size_t)y * a.width + x;
    const float4 sp = a.src[p], f0p = a.feat[2 * p], f1p = a.feat[2 * p + 1];
    float4 res = sp;
    if (!(f0p.w > 0.0f)) {                     // an emitter pixel takes no other tap: it keeps (u, var)
        float gs = 0.0f, gw = 0.0f;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = (int)x + dx, qy = (int)y + dy;
                if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                gs += k * a.src[(size_t)qy * W + qx].w;
                gw += k;
            }
        const float g = __builtin_sqrtf(gs / gw);
        const float Lp = dn_lum(sp.x, sp.y, sp.z);
        const float inv_l = 1.0f / (a.sigma_l * g + 1e-10f);
        const float inv_d = 1.0f / (a.sigma_d * (float)h * fmaxf(f1p.w, 1e-3f) + 1e-10f);
        constexpr float kB3[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const float kc = kB3[2] * kB3[2];
        float wsum = kc, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = kc * kc * sp.w;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int qy = (int)y + (j - 2) * h;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (i == 2 && j == 2) continue;
                const int qx = (int)x + (i - 2) * h;
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                const float4 sq = a.src[q], f0q = a.feat[2 * q], f1q = a.feat[2 * q + 1];
                const float nd = f1p.x * f1q.x + f1p.y * f1q.y + f1p.z * f1q.z;
                if (!(nd > 0.0f) || f0q.w > 0.0f) continue;
                const float el = fabsf(Lp - dn_lum(sq.x, sq.y, sq.z)) * inv_l;
                const float ed = fabsf(f1p.w - f1q.w) * inv_d;
                // k * nd^sigma_n * exp(-el - ed), as one exp2
                const float w = kB3[j] * kB3[i] * exp2f(a.sigma_n * log2f(nd) - (el + ed) * 1.44269504f);
                wsum += w;
                ar += w * (sq.x - sp.x); ag += w * (sq.y - sp.y); ab += w * (sq.z - sp.z);
                av += w * w * sq.w;
            }
        }
        const float inv = 1.0f / wsum;
        res = make_float4(sp.x + ar * inv, sp.y + ag * inv, sp.z + ab * inv, av * inv * inv);
    }
    if (a.finalize) dn_store(a, p, res.x, res.y, res.z, f0p);
    else a.dst[p] = res;
}
// k_denoise_init with the caller's variance plane (pt_denoise_var_device): var = var_in[p] when that is finite and >= 0; a
// lane whose entry is NaN, infinite or negative walks the 9 taps of dn_spatial_var instead, the others skip them.
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_init_var(DenoiseArgs a, const float* __restrict__ var_in) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float3 u = dn_demod(a, p);
    if (a.finalize) { dn_store(a, p, u.x, u.y, u.z, a.feat[2 * p]); return; }
    float var = var_in[p];
    if (!(var >= 0.0f && var <= 3.402823466e+38f)) var = dn_spatial_var(a, x, y);
    a.dst[p] = make_float4(u.x, u.y, u.z, var);
}
}  // namespace PTK_IMPL
namespace ptk {
// host: the grid of kDnBx x kDnBy pixel workgroups over a width x height image (every one-thread-per-pixel kernel of this
// header and of pt_film_temporal.h)
static dim3 dn_grid(uint32_t width, uint32_t height) {
    return dim3((width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy);
}
void launch_denoise(const DenoiseArgs& a, bool init, hipStream_t st) {
    const dim3 g = dn_grid(a.width, a.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    if (init) hipLaunchKernelGGL(PTK_IMPL::k_denoise_init, g, b, 0, st, a);
    else hipLaunchKernelGGL(PTK_IMPL::k_denoise_step, g, b, 0, st, a);
}
void launch_denoise_init_var(const DenoiseArgs& a, const float* var, hipStream_t st) {
    const dim3 g = dn_grid(a.width, a.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_init_var, g, b, 0, st, a, var);
}
}  // namespace ptk
