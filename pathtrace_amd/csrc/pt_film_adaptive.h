// pt_film_adaptive.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_adaptive.h"
#include "pt_denoise_var.h"

// ------------------------------------------------------------------ adaptive sampling (pt_render_adaptive, rule: pt_adaptive.h)
namespace PTK_IMPL {
// k_resolve for one sample batch of an adaptive pass: list slot i -> image pixel pix, whose f64 sums (R, G, B and the
// luminance sums S1, S2) take the batch's samples in sample order.  A pixel's sums are thus exactly the ones k_resolve forms
// for it in a uniform render of as many samples, and its mean, gamma and RGBA8 are the same expressions (world.rs:311-332).
__global__ void __launch_bounds__(kBlock) k_resolve_adaptive(AdaptiveResolveArgs a) {
    if (blockIdx.x == 0u && a.zero_words)
        for (uint32_t k = threadIdx.x; k < a.n_zero; k += kBlock) a.zero_words[k] = 0u;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    uint32_t pix = i;
    if (a.pixels) { const uint2 xy = a.pixels[i]; pix = xy.y * a.width + xy.x; }
    double* const sp = a.f.sums + 5 * (size_t)pix;
    double r = 0.0, g = 0.0, b = 0.0, s1 = 0.0, s2 = 0.0;
    if (a.load) { r = sp[0]; g = sp[1]; b = sp[2]; s1 = sp[3]; s2 = sp[4]; }
    auto add = [&](const Rgb& v) {
        r += (double)v.r; g += (double)v.g; b += (double)v.b;                     // world.rs:311
        const double L = ptad::luminance(v.r, v.g, v.b);
        s1 += L; s2 += L * L;
    };
    uint32_t s = 0;
    for (; s + 4u <= a.nb; s += 4u) {              // four samples' loads in flight before the ordered additions (as k_resolve)
        Rgb v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = a.lsamp[(size_t)(s + k) * a.n + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) add(v[k]);
    }
    for (; s < a.nb; ++s) add(a.lsamp[(size_t)s * a.n + i]);
    sp[0] = r; sp[1] = g; sp[2] = b; sp[3] = s1; sp[4] = s2;
    if (!a.finalize) return;
    const double dn = (double)a.n_total;
    const double c[3] = {r / dn, g / dn, b / dn};                                 // world.rs:315
    uint32_t q8 = 0xFF000000u;                                                    // alpha 255, world.rs:331
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double gm = __builtin_sqrt(c[k]);                                   // gamma 2.0, world.rs:322-324
        const double cl = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);                 // clamp keeps NaN
        const double q = cl * 255.0;
        q8 |= (uint32_t)((q != q) ? (uint8_t)0 : (uint8_t)q) << (8 * k);          // `as u8`: truncation, NaN -> 0
        a.f.out_linear[3 * (size_t)pix + k] = (float)c[k];
    }
    *reinterpret_cast<uint32_t*>(a.f.out_rgba + 4 * (size_t)pix) = q8;
    double rel;
    const bool conv = ptad::check(s1, s2, a.n_total, a.f.rel_tol, a.f.abs_floor, &rel);
    a.f.count[pix] = a.n_total;
    a.f.rel_err[pix] = (float)rel;
    a.f.conv[pix] = conv ? 1u : 0u;
}

// The list's pixels that failed their last check, compacted in list order.  Workgroup b owns the kSelectTile slots from
// b * kSelectTile; k_adaptive_count leaves its survivor count in block_counts[b], and k_adaptive_select adds up the counts
// of the workgroups before it (its output offset), then writes its survivors by wave ballot + prefix popcount.
constexpr uint32_t kSelectRounds = kSelectTile / kBlock;
PT_DEV uint2 select_pixel(const uint2* pixels, uint32_t width, uint32_t i) {
    return pixels ? pixels[i] : make_uint2(i % width, i / width);
}
PT_DEV bool select_keep(const uint2* pixels, uint32_t n, uint32_t width, const uint32_t* conv, uint32_t i, uint2& xy) {
    if (i >= n) return false;
    xy = select_pixel(pixels, width, i);
    return conv[xy.y * width + xy.x] == 0u;
}
__global__ void __launch_bounds__(kBlock) k_adaptive_count(const uint2* __restrict__ pixels, uint32_t n, uint32_t width,
                                                           const uint32_t* __restrict__ conv, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    uint32_t cnt = 0;                              // wave-uniform
    for (uint32_t r = 0; r < kSelectRounds; ++r) {
        uint2 xy;
        const bool keep = select_keep(pixels, n, width, conv, blockIdx.x * kSelectTile + r * kBlock + threadIdx.x, xy);
        cnt += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0u) s_wave[wib] = cnt;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_wave[w];
        block_counts[blockIdx.x] = t;
    }
}
__global__ void __launch_bounds__(kBlock) k_adaptive_select(const uint2* __restrict__ pixels, uint32_t n, uint32_t width,
                                                            const uint32_t* __restrict__ conv, const uint32_t* __restrict__ block_counts,
                                                            uint2* __restrict__ out, uint32_t* __restrict__ out_n) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    // output offset of this workgroup: survivors of the workgroups before it
    uint32_t part = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += kBlock) part += block_counts[k];
    for (int off = 32; off > 0; off >>= 1) part += (uint32_t)__shfl_xor((int)part, off);
    if (lane == 0u) s_wave[wib] = part;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) base += s_wave[w];
    for (uint32_t r = 0; r < kSelectRounds; ++r) {
        __syncthreads();                           // (everybody has read s_wave)
        uint2 xy;
        const bool keep = select_keep(pixels, n, width, conv, blockIdx.x * kSelectTile + r * kBlock + threadIdx.x, xy);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0u) s_wave[wib] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) { before += w < wib ? s_wave[w] : 0u; total += s_wave[w]; }
        if (keep) out[base + before + lane_rank(mask)] = xy;
        base += total;
    }
    if (blockIdx.x + 1u == gridDim.x && threadIdx.x == 0u) *out_n = base;
}

// pt_adaptive_variance_device: the state a completed pt_render_adaptive left (sums and count of every image pixel) and the
// pixel's feature albedo -> the variance plane of pt_denoise_var_device.  The rule is pt_denoise_var.h; one thread per pixel.
__global__ void __launch_bounds__(kBlock) k_adaptive_variance(const double* __restrict__ sums, const uint32_t* __restrict__ count,
                                                              const float4* __restrict__ feat, uint32_t np, float* __restrict__ var) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= np) return;
    const double* const sp = sums + 5 * (size_t)p;
    const double s[5] = {sp[0], sp[1], sp[2], sp[3], sp[4]};
    const float4 f0 = feat[2 * (size_t)p];
    var[p] = ptdv::pixel_variance(s, count[p], f0.x, f0.y, f0.z);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_resolve_adaptive(const AdaptiveResolveArgs& a, hipStream_t st) {
    if (a.n) hipLaunchKernelGGL(PTK_IMPL::k_resolve_adaptive, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_adaptive_select(const uint2* pixels, uint32_t n, uint32_t width, const uint32_t* conv, uint32_t* block_counts,
                            uint2* out, uint32_t* out_n, hipStream_t st) {
    if (n == 0u) { (void)hipMemsetAsync(out_n, 0, sizeof(uint32_t), st); return; }
    const dim3 g((n + kSelectTile - 1) / kSelectTile), b(kBlock);
    hipLaunchKernelGGL(PTK_IMPL::k_adaptive_count, g, b, 0, st, pixels, n, width, conv, block_counts);
    hipLaunchKernelGGL(PTK_IMPL::k_adaptive_select, g, b, 0, st, pixels, n, width, conv, (const uint32_t*)block_counts, out, out_n);
}
void launch_adaptive_variance(const double* sums, const uint32_t* count, const float4* feat, uint32_t np, float* var, hipStream_t st) {
    if (np) hipLaunchKernelGGL(PTK_IMPL::k_adaptive_variance, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sums, count, feat, np, var);
}
}  // namespace ptk
