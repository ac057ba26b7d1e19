// pt_kernels_film.hip -- the kernels that work on the film, not on paths: multi-GPU film exchange, adaptive sampling, the
// a-trous denoiser and its temporal accumulation.  None of them has a division or square root whose result depends on the
// arithmetic mode, so the unit is compiled once, in fast mode (its kernels live in ptk_fast_impl), and serves both modes.
#include "pt_kernels_scan.h"
#include "pt_adaptive.h"
#include "pt_denoise_var.h"
#if PT_MATH_EXACT
#error "pt_kernels_film.hip is built once, with -DPT_MATH_EXACT=0"
#endif

namespace PTK_IMPL {
// ------------------------------------------------------------------ multi-GPU film exchange (pt_multi.cpp)
// A device's tile -> one 16-byte record per pixel (12 B linear RGB + 4 B RGBA8), so that both film planes travel in
// ONE gather; rows beyond the tile (tiles are padded to the largest one) are left untouched.
__global__ void __launch_bounds__(kBlock) k_film_pack(const float* __restrict__ lin, const uint8_t* __restrict__ rgba,
                                                      uint32_t np, uint4* __restrict__ packed) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= np) return;
    uint4 v;
    v.x = __float_as_uint(lin[3 * (size_t)p]); v.y = __float_as_uint(lin[3 * (size_t)p + 1]); v.z = __float_as_uint(lin[3 * (size_t)p + 2]);
    v.w = rgba ? *reinterpret_cast<const uint32_t*>(rgba + 4 * (size_t)p) : 0u;
    packed[p] = v;
}
// The gathered tiles (device g's padded tile at recv + g * max_rows * W) -> the frame in image order.  Image row y lies
// in band y / band_rows, which device (band % n_dev) rendered as its tile row (band / n_dev) * band_rows + y % band_rows.
__global__ void __launch_bounds__(kBlock) k_film_unpack(const uint4* __restrict__ recv, uint32_t W, uint32_t H, uint32_t band_rows,
                                                        uint32_t n_dev, uint32_t max_rows, float* __restrict__ lin,
                                                        uint8_t* __restrict__ rgba) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= W * H) return;
    const uint32_t y = p / W, x = p - y * W;
    const uint32_t band = y / band_rows, g = band % n_dev;
    const uint32_t k = (band / n_dev) * band_rows + (y - band * band_rows);
    const uint4 v = recv[((size_t)g * max_rows + k) * W + x];
    lin[3 * (size_t)p] = __uint_as_float(v.x); lin[3 * (size_t)p + 1] = __uint_as_float(v.y); lin[3 * (size_t)p + 2] = __uint_as_float(v.z);
    if (rgba) *reinterpret_cast<uint32_t*>(rgba + 4 * (size_t)p) = v.w;
}

// ------------------------------------------------------------------ adaptive sampling (pt_render_adaptive, rule: pt_adaptive.h)
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
void launch_film_pack(const float* lin, const uint8_t* rgba, uint32_t np, void* packed, hipStream_t st) {
    if (np) hipLaunchKernelGGL(PTK_IMPL::k_film_pack, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, lin, rgba, np, (uint4*)packed);
}
void launch_film_unpack(const void* recv, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_dev, uint32_t max_rows, float* lin,
                        uint8_t* rgba, hipStream_t st) {
    if (W * H) hipLaunchKernelGGL(PTK_IMPL::k_film_unpack, dim3((W * H + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint4*)recv, W, H,
                                  band_rows, n_dev, max_rows, lin, rgba);
}
}  // namespace ptk

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
void launch_denoise(const DenoiseArgs& a, bool init, hipStream_t st) {
    const dim3 g((a.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    if (init) hipLaunchKernelGGL(PTK_IMPL::k_denoise_init, g, b, 0, st, a);
    else hipLaunchKernelGGL(PTK_IMPL::k_denoise_step, g, b, 0, st, a);
}
void launch_denoise_init_var(const DenoiseArgs& a, const float* var, hipStream_t st) {
    const dim3 g((a.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_init_var, g, b, 0, st, a, var);
}
}  // namespace ptk

// ------------------------------------------------------------------ temporal accumulation (pt_denoise_temporal_device)
// The rule is stated in include/pathtrace_amd.h (PtTemporal) and DESIGN.md 5c.  One thread per pixel, in place of k_denoise_init.
// The reprojection runs in f64: an f32 solve puts x' about 1e-4 pixel off at 1024^2, and a bilinear tap of that weight moves
// a dim pixel next to a bright one by far more than the accumulation's own rounding.  Everything after it is f32.
namespace PTK_IMPL {
PT_DEV double tm_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PT_DEV void tm_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// pixel (x, y) at depth d seen from the frame's camera -> (x', y') in the history's image and d_exp; false: no reprojection
PT_DEV bool tm_reproject(const TemporalArgs& a, uint32_t x, uint32_t y, float d, double& xr, double& yr, double& dexp) {
    const double* o = a.cur; const double* l = a.cur + 3; const double* hz = a.cur + 6; const double* vt = a.cur + 9;
    const double* o2 = a.prev; const double* l2 = a.prev + 3; const double* hz2 = a.prev + 6; const double* vt2 = a.prev + 9;
    const double W1 = (double)(a.dn.width - 1u), H1 = (double)(a.dn.height - 1u);
    const double s = ((double)x + 0.5) / W1, t = ((double)(a.dn.height - 1u - y) + 0.5) / H1;      // camera.rs:139-147, world.rs:299
    double D[3], P[3], c[3], r[3], bc[3], rc[3], br[3];
    for (int k = 0; k < 3; ++k) D[k] = l[k] + s * hz[k] + t * vt[k] - o[k];
    const double inv_len = 1.0 / __builtin_sqrt(tm_dot(D, D));
    for (int k = 0; k < 3; ++k) {
        P[k] = o[k] + (double)d * (D[k] * inv_len);
        c[k] = o2[k] - P[k];                 // -(P - o')
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
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal(TemporalArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.dn.width || y >= a.dn.height) return;
    const int W = (int)a.dn.width, H = (int)a.dn.height;
    const size_t p = (size_t)y * a.dn.width + x;
    const float4 f0p = a.dn.feat[2 * p], f1p = a.dn.feat[2 * p + 1];
    const float3 uc = dn_demod(a.dn, p);
    const float Lc = dn_lum(uc.x, uc.y, uc.z);
    // the valid-weighted history of the 2 x 2 bilinear taps around (x', y')
    float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hm1 = 0.0f, hm2 = 0.0f, hn = 0.0f;
    if (a.hist_src && f1p.w > 0.0f) {
        double xr = x, yr = y, dexp = f1p.w;
        const bool ok = a.same_camera || tm_reproject(a, x, y, f1p.w, xr, yr, dexp);
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
                    if (!(f1p.x * h2.x + f1p.y * h2.y + f1p.z * h2.z >= a.normal_tol)) continue;
                    const float4 h1 = a.hist_src[3 * q + 1];
                    if (em != (h1.z > 0.0f)) continue;
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
        const float al = fmaxf(a.alpha, 1.0f / n);
        u = make_float3(ur + al * (uc.x - ur), ug + al * (uc.y - ug), ub + al * (uc.z - ub));
        m1 = um1 + al * (Lc - um1);
        m2 = um2 + al * (Lc * Lc - um2);
    }
    const float var = n >= 4.0f ? fmaxf(0.0f, m2 - m1 * m1) : dn_spatial_var(a.dn, x, y);
    a.hist_dst[3 * p] = make_float4(u.x, u.y, u.z, m1);
    a.hist_dst[3 * p + 1] = make_float4(m2, n, f0p.w, 0.0f);
    a.hist_dst[3 * p + 2] = f1p;
    if (a.dn.finalize) dn_store(a.dn, p, u.x, u.y, u.z, f0p);
    else a.dn.dst[p] = make_float4(u.x, u.y, u.z, var);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_denoise_temporal(const TemporalArgs& a, hipStream_t st) {
    const dim3 g((a.dn.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.dn.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy),
        b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal, g, b, 0, st, a);
}
}  // namespace ptk

// ------------------------------------------------------------------ ... that follows moving objects (pt_denoise_temporal_motion_device)
// Rules 1', 2', 3' and 7' of include/pathtrace_amd.h and DESIGN.md 5d.  k_denoise_temporal with three additions: the pixel's
// point goes back along its object's motion map (f64) before the camera reprojection, the normal gate takes the normal
// carried by that map, and a tap of another object's history is taken only when neither object moved.  A pixel whose map
// is the identity runs k_denoise_temporal's statements in their order: with the unknown ids that kernel stores, or in a
// scene where nothing moved, the two kernels write the same bits.  The functions are this kernel's own copies.
namespace PTK_IMPL {
// tm_reproject with P carried to the history pose by mp first (mp null: the identity, P as it is)
PT_DEV bool tmm_reproject(const TemporalArgs& a, const MotionMap* mp, uint32_t x, uint32_t y, float d, double& xr, double& yr, double& dexp) {
    const double* o = a.cur; const double* l = a.cur + 3; const double* hz = a.cur + 6; const double* vt = a.cur + 9;
    const double* o2 = a.prev; const double* l2 = a.prev + 3; const double* hz2 = a.prev + 6; const double* vt2 = a.prev + 9;
    const double W1 = (double)(a.dn.width - 1u), H1 = (double)(a.dn.height - 1u);
    const double s = ((double)x + 0.5) / W1, t = ((double)(a.dn.height - 1u - y) + 0.5) / H1;
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
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal_motion(TemporalMotionArgs m) {
    const TemporalArgs& a = m.t;
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.dn.width || y >= a.dn.height) return;
    const int W = (int)a.dn.width, H = (int)a.dn.height;
    const size_t p = (size_t)y * a.dn.width + x;
    const float4 f0p = a.dn.feat[2 * p], f1p = a.dn.feat[2 * p + 1];
    const float3 uc = dn_demod(a.dn, p);
    const float Lc = dn_lum(uc.x, uc.y, uc.z);
    // the caller's id: checked against the scene before it indexes the maps
    const int32_t id = m.ids[p];
    const bool known = id >= 0 && (uint32_t)id < m.n_objs;
    const uint32_t flags = known ? m.maps[id].flags : 2u;
    const bool ident = flags == 1u;
    const float idf = known ? (float)(id + 1) : 0.0f;       // n_objs <= 2^24 - 2: exact
    float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hm1 = 0.0f, hm2 = 0.0f, hn = 0.0f;
    if (a.hist_src && f1p.w > 0.0f && !(flags & 2u)) {
        double xr = x, yr = y, dexp = f1p.w;
        float nx = f1p.x, ny = f1p.y, nz = f1p.z;
        bool ok = true;
        if (!(ident && a.same_camera)) {
            const MotionMap* mp = ident ? nullptr : m.maps + id;
            ok = tmm_reproject(a, mp, x, y, f1p.w, xr, yr, dexp);
            if (mp) {                         // n_h = A n_p, normalised in f64 (n_p when its length is 0)
                double v[3];
                for (int k = 0; k < 3; ++k) v[k] = mp->a[3 * k] * (double)f1p.x + mp->a[3 * k + 1] * (double)f1p.y + mp->a[3 * k + 2] * (double)f1p.z;
                const double len = __builtin_sqrt(tm_dot(v, v));
                if (len > 0.0) { nx = (float)(v[0] / len); ny = (float)(v[1] / len); nz = (float)(v[2] / len); }
            }
        }
        if (ok && xr > -1.0 && xr < (double)W && yr > -1.0 && yr < (double)H) {
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
                    if (h1.w != 0.0f && h1.w != idf) {       // another object's history: only when neither object moved
                        if (!ident || !(h1.w >= 1.0f && h1.w <= (float)m.n_objs)) continue;
                        if (m.maps[(uint32_t)h1.w - 1u].flags != 1u) continue;
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
        const float al = fmaxf(a.alpha, 1.0f / n);
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
}  // namespace PTK_IMPL
namespace ptk {
void launch_denoise_temporal_motion(const TemporalMotionArgs& a, hipStream_t st) {
    const dim3 g((a.t.dn.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.t.dn.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy),
        b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal_motion, g, b, 0, st, a);
}
}  // namespace ptk

// ------------------------------------------------------------------ device-side BVH refit (pt_scene_refit)
// The rule is ptbvh::refit (pt_bvh.h / pt_bvh.cpp) and DESIGN.md 5e; these kernels reproduce its arrays bit for bit.  That is a
// requirement: the grid comes from the HOST's boxes and the quantisation clamps to it, so a device box one ulp outside the
// host's would be quantised to a box that no longer encloses it.  Hence f64 + - * / sqrt floor ceil (correctly rounded on the
// device as on the host), no contraction, the host's compare-and-step outward rounding, and fmaf for the decode as there.
// None of it depends on the arithmetic mode.
#include "pt_bvh.h"
namespace PTK_IMPL {
// ptbvh's down() / up(): the f32 at or below / at or above v
PT_DEV float refit_down(double v) {
    float f = (float)v;
    if ((double)f > v) {                       // step to the next f32 below (nextafterf(f, -inf))
        const uint32_t b = __float_as_uint(f);
        f = f > 0.0f ? __uint_as_float(b - 1u) : f == 0.0f ? __uint_as_float(0x80000001u) : __uint_as_float(b + 1u);
    }
    return f;
}
PT_DEV float refit_up(double v) {
    float f = (float)v;
    if ((double)f < v) {                       // nextafterf(f, +inf)
        const uint32_t b = __float_as_uint(f);
        f = f < 0.0f ? __uint_as_float(b - 1u) : f == 0.0f ? __uint_as_float(0x00000001u) : __uint_as_float(b + 1u);
    }
    return f;
}
// ptbvh::primitive_box for a finite primitive (the host drops the tree before any launch when an object is not finite)
PT_DEV void refit_primitive_box(const float4& r0, const float4& r1, const float4& r2, bool tri, float lo[3], float hi[3]) {
#pragma clang fp contract(off)
    if (!tri) {
        const float r2f = r0.w * r0.w;
        const double r = __builtin_sqrt((double)r2f) * (1.0 + 1e-7);
        const double c[3] = {r0.x, r0.y, r0.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = refit_down(c[k] - r); hi[k] = refit_up(c[k] + r); }
    } else {
        const double v0[3] = {r0.x, r0.y, r0.z}, e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = v0[k], b = v0[k] + e1[k], c = v0[k] + e2[k];
            const double mn_bc = c < b ? c : b, mx_bc = b < c ? c : b;      // std::min / std::max
            lo[k] = refit_down(mn_bc < a ? mn_bc : a);
            hi[k] = refit_up(a < mx_bc ? mx_bc : a);
        }
    }
}
// Box::grow
PT_DEV void refit_grow(float lo[3], float hi[3], const float4& blo, const float4& bhi) {
    lo[0] = blo.x < lo[0] ? blo.x : lo[0]; lo[1] = blo.y < lo[1] ? blo.y : lo[1]; lo[2] = blo.z < lo[2] ? blo.z : lo[2];
    hi[0] = hi[0] < bhi.x ? bhi.x : hi[0]; hi[1] = hi[1] < bhi.y ? bhi.y : hi[1]; hi[2] = hi[2] < bhi.z ? bhi.z : hi[2];
}
// quantise()'s q_lo / q_hi: the grid plane at or below / at or above v, by the decode the traversal evaluates
PT_DEV uint32_t refit_q_lo(float v, float gmin, float cell) {
#pragma clang fp contract(off)
    long long q = (long long)__builtin_floor(((double)v - (double)gmin) / (double)cell);
    q = q < 0 ? 0 : q > 65535 ? 65535 : q;
    while (q > 0 && __builtin_fmaf((float)(uint32_t)q, cell, gmin) > v) --q;
    return (uint32_t)q;
}
PT_DEV uint32_t refit_q_hi(float v, float gmin, float cell) {
#pragma clang fp contract(off)
    long long q = (long long)__builtin_ceil(((double)v - (double)gmin) / (double)cell);
    q = q < 0 ? 0 : q > 65535 ? 65535 : q;
    while (q < 65535 && __builtin_fmaf((float)(uint32_t)q, cell, gmin) < v) ++q;
    return (uint32_t)q;
}

// One thread per leaf slot: the slot's scan records (make_leaf's) and the primitive's f32 box.  Padding slots keep their zeros.
__global__ void __launch_bounds__(kBlock) k_bvh_refit_leaves(BvhRefitArgs a) {
    if (blockIdx.x == 0u && threadIdx.x < 3u) a.cost[threadIdx.x] = 0ull;      // the level launches add to them
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= a.n_slots) return;
    const uint32_t w = a.ids[slot];
    if (w == ptbvh::kDone) return;
    const uint32_t o = w & ~ptbvh::kTriangleBit;
    const bool tri = (w & ptbvh::kTriangleBit) != 0u;
    const float4 r0 = a.shape[3 * (size_t)o], r1 = a.shape[3 * (size_t)o + 1], r2 = a.shape[3 * (size_t)o + 2];
    float4 rec[3];
    if (tri) {
        ptbvh::triangle_scan_record(r0, r1, r2, rec);
    } else {
        rec[0] = make_float4(r0.x, r0.y, r0.z, r0.w * r0.w);                   // (c, r^2)
        rec[1] = make_float4(0.f, 0.f, 0.f, 0.f); rec[2] = rec[1];
    }
    a.rec[3 * (size_t)slot] = rec[0]; a.rec[3 * (size_t)slot + 1] = rec[1]; a.rec[3 * (size_t)slot + 2] = rec[2];
    a.lead[slot] = rec[0];
    float lo[3], hi[3];
    refit_primitive_box(r0, r1, r2, tri, lo, hi);
    a.slot_box[2 * (size_t)slot] = make_float4(lo[0], lo[1], lo[2], 0.f);
    a.slot_box[2 * (size_t)slot + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

// The nodes order[first, first + count) -- one height --, four lanes per node, one per child slot.  A lane forms its child's
// f32 box (a leaf: the union of its slots' boxes; a node: that node's stored union, written by an earlier launch), the four
// lanes' union is stored for the parent, each lane quantises its box, and the twelve box words are regrouped across the
// four lanes into the node's three 16-byte stores.  The cost terms are summed over the wave before one 64-bit atomic add
// per sum and wave: integer sums, so the result does not depend on the order.
__global__ void __launch_bounds__(kBlock) k_bvh_refit_level(BvhRefitArgs a, uint32_t first, uint32_t count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x, pos = t >> 2, c = t & 3u;
    const uint32_t lane = threadIdx.x & 63u;
    const bool node_ok = pos < count;
    uint32_t k = 0u, code = ptbvh::kDone;
    uint4 codes = make_uint4(ptbvh::kDone, ptbvh::kDone, ptbvh::kDone, ptbvh::kDone);
    if (node_ok) {
        k = a.order[first + pos];
        codes = a.nodes[4 * (size_t)k + 3];
        code = c == 0u ? codes.x : c == 1u ? codes.y : c == 2u ? codes.z : codes.w;
    }
    const bool used = code != ptbvh::kDone;    // the builder fills the child slots from 0 and gives the rest the sentinel
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    if (used) {
        if (code & ptbvh::kLeafBit) {
            const uint32_t s0 = code & 0x0FFFFFFFu, cnt = ((code >> 28) & 7u) + 1u;
            for (uint32_t i = s0; i < s0 + cnt && i < a.n_slots; ++i) refit_grow(lo, hi, a.slot_box[2 * (size_t)i], a.slot_box[2 * (size_t)i + 1]);
        } else {
            refit_grow(lo, hi, a.node_box[2 * (size_t)code], a.node_box[2 * (size_t)code + 1]);
        }
    }
    // the node's own union (an unused slot's box is empty: it changes nothing)
    float ulo[3], uhi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ulo[d] = fminf(lo[d], __shfl_xor(lo[d], 1)); ulo[d] = fminf(ulo[d], __shfl_xor(ulo[d], 2));
        uhi[d] = fmaxf(hi[d], __shfl_xor(hi[d], 1)); uhi[d] = fmaxf(uhi[d], __shfl_xor(uhi[d], 2));
    }
    if (node_ok && c == 0u) {
        a.node_box[2 * (size_t)k] = make_float4(ulo[0], ulo[1], ulo[2], 0.f);
        a.node_box[2 * (size_t)k + 1] = make_float4(uhi[0], uhi[1], uhi[2], 0.f);
    }
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u;        // unused slot: zero words
    unsigned long long sxy = 0ull, syz = 0ull, szx = 0ull;
    if (used) {
        const uint32_t lx = refit_q_lo(lo[0], a.grid_min[0], a.grid_cell[0]), ly = refit_q_lo(lo[1], a.grid_min[1], a.grid_cell[1]),
                       lz = refit_q_lo(lo[2], a.grid_min[2], a.grid_cell[2]);
        const uint32_t hx = refit_q_hi(hi[0], a.grid_min[0], a.grid_cell[0]), hy = refit_q_hi(hi[1], a.grid_min[1], a.grid_cell[1]),
                       hz = refit_q_hi(hi[2], a.grid_min[2], a.grid_cell[2]);
        w0 = lx | (ly << 16); w1 = lz | (hx << 16); w2 = hy | (hz << 16);
        const unsigned long long dx = hx - lx, dy = hy - ly, dz = hz - lz;
        sxy = dx * dy; syz = dy * dz; szx = dz * dx;
    }
    // word j of the node (j < 12) = word j % 3 of child j / 3; lane c < 3 stores uint4 c = words 4c .. 4c + 3, which lie in
    // children c and c + 1: (w0 w1 w2 | w0'), (w1 w2 | w0' w1'), (w2 | w0' w1' w2')
    const uint32_t base = lane & ~3u, src_a = base + (c < 3u ? c : 0u), src_b = base + (c < 3u ? c + 1u : 0u);
    const uint32_t a0 = __shfl(w0, src_a), a1 = __shfl(w1, src_a), a2 = __shfl(w2, src_a);
    const uint32_t b0 = __shfl(w0, src_b), b1 = __shfl(w1, src_b), b2 = __shfl(w2, src_b);
    if (node_ok && c < 3u) {
        const uint4 v = c == 0u ? make_uint4(a0, a1, a2, b0) : c == 1u ? make_uint4(a1, a2, b0, b1) : make_uint4(a2, b0, b1, b2);
        a.nodes[4 * (size_t)k + c] = v;
    }
    if (node_ok && c == 3u) a.nodes[4 * (size_t)k + 3] = codes;                 // the code word, carried over
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sxy += __shfl_xor(sxy, off); syz += __shfl_xor(syz, off); szx += __shfl_xor(szx, off);
    }
    if (lane == 0u && (sxy | syz | szx) != 0ull) {
        atomicAdd(a.cost, sxy); atomicAdd(a.cost + 1, syz); atomicAdd(a.cost + 2, szx);
    }
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_bvh_refit_leaves(const BvhRefitArgs& a, hipStream_t st) {
    if (a.n_slots) hipLaunchKernelGGL(PTK_IMPL::k_bvh_refit_leaves, dim3((a.n_slots + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_bvh_refit_level(const BvhRefitArgs& a, uint32_t first, uint32_t count, hipStream_t st) {
    if (count) hipLaunchKernelGGL(PTK_IMPL::k_bvh_refit_level, dim3((uint32_t)(((uint64_t)count * 4u + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, first, count);
}
}  // namespace ptk

// ------------------------------------------------------------------ device-side BVH build (pt_scene_rebuild)
// The rule is ptbvh::build_morton (pt_bvh.h) and DESIGN.md 5f.  The topology is a function of the object count and comes from
// the host once; what these kernels decide is the order of the objects: (Morton key, index) ascending.  The key is the host's
// expression on the host's boxes (refit_primitive_box) and the host's grid, in correctly rounded f64; the order is total, so a
// correct sort reproduces the host's leaf_ids bit for bit.
namespace PTK_IMPL {
static_assert(kBlock == 256 && kSortDigits == kBlock, "one thread per digit");
constexpr uint32_t kSortRounds = kSortTile / kBlock;
constexpr uint32_t kSortWaves = kBlock / 64;
constexpr uint32_t kScanBlock = 1024;      // k_bvh_sort_scan: one workgroup, four words per thread and step

// digit of a pass: the pair as one 64-bit key, .x the low word (shift is a multiple of 8: a digit lies in one word)
PT_DEV uint32_t sort_digit(const uint2& kv, uint32_t shift) {
    return ((shift < 32u ? kv.x >> shift : kv.y >> (shift - 32u))) & (kSortDigits - 1u);
}

__global__ void __launch_bounds__(kBlock) k_bvh_morton(BvhBuildArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 r0 = a.shape[3 * (size_t)i], r1 = a.shape[3 * (size_t)i + 1], r2 = a.shape[3 * (size_t)i + 2];
    float lo[3], hi[3];
    refit_primitive_box(r0, r1, r2, a.tags[i] != 0u, lo, hi);
    const float gmin[3] = {a.grid_min[0], a.grid_min[1], a.grid_min[2]}, cell[3] = {a.grid_cell[0], a.grid_cell[1], a.grid_cell[2]};
    a.pairs[0][i] = make_uint2(ptbvh::morton_key(lo, hi, gmin, cell), i);
}

// One pass of the sort, part 1: how many keys of tile blockIdx.x carry each value of the pass's digit -> hist[digit * tiles + tile]
__global__ void __launch_bounds__(kBlock) k_bvh_sort_hist(const uint2* __restrict__ in, uint32_t* __restrict__ hist, uint32_t n, uint32_t tiles, uint32_t shift) {
    __shared__ uint32_t h[kSortDigits];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (uint32_t r = 0; r < kSortRounds; ++r) {
        const uint32_t i = base + r * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&h[sort_digit(in[i], shift)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// Part 2: the exclusive prefix sum over hist as one array (digit-major: all tiles of digit 0, then of digit 1, ...), in place:
// afterwards hist[digit * tiles + tile] is where that tile's first key with that digit goes.  One workgroup walks the array
// with a running carry; `total` = 256 * tiles is a multiple of 4 and the array is 16-byte aligned.
__global__ void __launch_bounds__(kScanBlock) k_bvh_sort_scan(uint32_t* hist, uint32_t total) {
    __shared__ uint32_t wsum[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < total; base += 4u * kScanBlock) {
        const uint32_t i = base + 4u * threadIdx.x;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < total) v = *reinterpret_cast<const uint4*>(hist + i);
        const uint32_t s = v.x + v.y + v.z + v.w;
        uint32_t x = s;                                          // inclusive scan over the wave
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kScanBlock / 64; ++w) { const uint32_t t = wsum[w]; before += w < wave ? t : 0u; all += t; }
        if (i < total) {
            const uint32_t e = carry + before + x - s;
            *reinterpret_cast<uint4*>(hist + i) = make_uint4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
        }
        carry += all;
        __syncthreads();
    }
}

// Part 3: every key of the tile to its place.  The tile is taken in rounds of one key per thread, in index order.  Within a
// round a key's rank among the keys with the same digit is: the lanes below it in its wave with that digit (the lanes that
// agree on all eight digit bits, by eight ballots) + the counts of that digit in the waves before (through LDS); base[digit]
// then moves on by the round's count.  Input order is kept among equal digits: the pass is stable.
__global__ void __launch_bounds__(kBlock) k_bvh_sort_scatter(const uint2* __restrict__ in, uint2* __restrict__ out, const uint32_t* __restrict__ hist, uint32_t n,
                                                             uint32_t tiles, uint32_t shift) {
    __shared__ uint32_t base[kSortDigits];
    __shared__ uint32_t wcnt[kSortWaves][kSortDigits];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    base[tid] = hist[(size_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) wcnt[w][tid] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kSortTile;
    for (uint32_t r = 0; r < kSortRounds; ++r) {
        if (first + r * kBlock >= n) break;                      // (the same for every thread of the workgroup)
        const uint32_t i = first + r * kBlock + tid;
        const bool valid = i < n;
        const uint2 kv = valid ? in[i] : make_uint2(0u, 0u);
        const uint32_t d = sort_digit(kv, shift);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = ((d >> b) & 1u) != 0u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)), cnt = (uint32_t)__popcll(same);
        if (valid && rank == 0u) wcnt[wave][d] = cnt;            // one lane per digit present in the wave
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
#pragma unroll
            for (uint32_t w = 0; w < kSortWaves; ++w) pos += w < wave ? wcnt[w][d] : 0u;
            if (pos < n) out[pos] = kv;
        }
        __syncthreads();
        uint32_t add = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; ++w) { add += wcnt[w][tid]; wcnt[w][tid] = 0u; }
        base[tid] += add;
        __syncthreads();
    }
}

// One thread per leaf slot: the object of sorted position p (pairs == nullptr: object p) with its triangle bit; the padding
// slots behind the last object get the sentinel and zero records, as build() leaves them.
__global__ void __launch_bounds__(kBlock) k_bvh_write_ids(BvhBuildArgs a, const uint2* pairs) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n_slots) return;
    uint32_t w = ptbvh::kDone;
    if (p < a.n) {
        const uint32_t o = pairs ? pairs[p].y : p;
        if (o < a.n) w = o | (a.tags[o] != 0u ? ptbvh::kTriangleBit : 0u);
    }
    a.ids[p] = w;
    if (w == ptbvh::kDone) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        a.rec[3 * (size_t)p] = z; a.rec[3 * (size_t)p + 1] = z; a.rec[3 * (size_t)p + 2] = z;
        a.lead[p] = z;
    }
}

// The child codes of the cached topology into the code words of the node array
__global__ void __launch_bounds__(kBlock) k_bvh_codes(uint4* nodes, const uint4* __restrict__ codes, uint32_t n_nodes) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < n_nodes) nodes[4 * (size_t)k + 3] = codes[k];
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_bvh_morton(const BvhBuildArgs& a, hipStream_t st) {
    if (a.n) hipLaunchKernelGGL(PTK_IMPL::k_bvh_morton, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
// `passes` stable passes over the digits from bit 0 upward, from pairs[src]; returns the buffer that holds the result
static uint32_t bvh_sort_passes(const BvhBuildArgs& a, uint32_t src, uint32_t passes, hipStream_t st) {
    const uint32_t tiles = bvh_sort_tiles(a.n);
    for (uint32_t pass = 0; pass < passes; ++pass, src ^= 1u) {
        const uint2* in = a.pairs[src];
        uint2* out = a.pairs[src ^ 1u];
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_sort_hist, dim3(tiles), dim3(kBlock), 0, st, in, a.hist, a.n, tiles, 8u * pass);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_sort_scan, dim3(1), dim3(PTK_IMPL::kScanBlock), 0, st, a.hist, kSortDigits * tiles);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_sort_scatter, dim3(tiles), dim3(kBlock), 0, st, in, out, (const uint32_t*)a.hist, a.n, tiles, 8u * pass);
    }
    return src;
}
void launch_bvh_sort(const BvhBuildArgs& a, hipStream_t st) {
    if (a.n) bvh_sort_passes(a, 0u, 4u, st);                     // the 32-bit key; an even number of passes: the result is in pairs[0]
}
void launch_bvh_write_ids(const BvhBuildArgs& a, bool sorted, hipStream_t st) {
    if (a.n_slots) hipLaunchKernelGGL(PTK_IMPL::k_bvh_write_ids, dim3((a.n_slots + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a, sorted ? (const uint2*)a.pairs[0] : (const uint2*)nullptr);
}
void launch_bvh_codes(uint4* nodes, const uint4* codes, uint32_t n_nodes, hipStream_t st) {
    if (n_nodes) hipLaunchKernelGGL(PTK_IMPL::k_bvh_codes, dim3((n_nodes + kBlock - 1) / kBlock), dim3(kBlock), 0, st, nodes, codes, n_nodes);
}
}  // namespace ptk

// ------------------------------------------------------------------ device-side BVH build, median order (pt_scene_rebuild_ordered)
// The rule is ptbvh::build_median (pt_bvh.h) and DESIGN.md 5i.  Every step orders its positions by (cell on the step's axis,
// object index), a total order: whatever sorts correctly reproduces the host's leaf_ids bit for bit.  Steps above T positions
// go through the radix sort, level by level; a step of at most T positions and everything beneath it is one workgroup's work.
namespace PTK_IMPL {
constexpr uint32_t kMedianT = ptbvh::kMedianTile;
constexpr uint32_t kMedianBlock = 1024;
constexpr uint32_t kMedianPer = kMedianT / kMedianBlock;     // positions per thread
constexpr uint32_t kMedianMaxSteps = 512;                    // a tile has at most T / 4 leaves, so fewer steps than that
static_assert(kMedianT % kMedianBlock == 0 && kMedianT / 4 <= kMedianMaxSteps && kMedianT < 65536, "tile steps are 16-bit offsets");
struct MedianCell { float c[3]; };

__global__ void __launch_bounds__(kBlock) k_bvh_cells(BvhBuildArgs a, uint2* __restrict__ cells) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 r0 = a.shape[3 * (size_t)i], r1 = a.shape[3 * (size_t)i + 1], r2 = a.shape[3 * (size_t)i + 2];
    float lo[3], hi[3];
    refit_primitive_box(r0, r1, r2, a.tags[i] != 0u, lo, hi);
    const float gmin[3] = {a.grid_min[0], a.grid_min[1], a.grid_min[2]}, cell[3] = {a.grid_cell[0], a.grid_cell[1], a.grid_cell[2]};
    const uint32_t g0 = ptbvh::grid_coord(lo, hi, gmin, cell, 0), g1 = ptbvh::grid_coord(lo, hi, gmin, cell, 1), g2 = ptbvh::grid_coord(lo, hi, gmin, cell, 2);
    cells[i] = make_uint2(g0 | (g1 << 16), g2);
    a.pairs[0][i] = make_uint2(i, 0u);
}

// the group of position p: the last one that starts at or before it (the first group starts at 0)
PT_DEV uint32_t median_group(const uint32_t* __restrict__ gs, uint32_t groups, uint32_t p) {
    uint32_t lo = 0u, hi = groups;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((gs[mid] & 0x7FFFFFFFu) <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// the rule's axis from the six bound words of a step
PT_DEV uint32_t median_axis(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t mx, uint32_t my, uint32_t mz, const MedianCell& cell) {
#pragma clang fp contract(off)
    // n* = 65535 - minimum: maximum - minimum = m + n - 65535
    const double wx = (double)(mx + nx - 65535u) * (double)cell.c[0], wy = (double)(my + ny - 65535u) * (double)cell.c[1],
                 wz = (double)(mz + nz - 65535u) * (double)cell.c[2];
    uint32_t axis = 0u;
    double widest = wx;
    if (wy > widest) { widest = wy; axis = 1u; }
    if (wz > widest) axis = 2u;
    return axis;
}

__global__ void __launch_bounds__(kBlock) k_bvh_median_bounds(const uint2* __restrict__ pairs, const uint2* __restrict__ cells, const uint32_t* __restrict__ gs,
                                                              uint32_t groups, uint32_t* bounds, uint32_t n, uint32_t mask) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = p < n;
    const uint32_t grp = median_group(gs, groups, valid ? p : n - 1u);
    const bool step = (gs[grp] >> 31) != 0u;
    uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};                     // 0 changes no maximum
    if (valid && step) {
        const uint32_t o = pairs[p].x & mask;
        if (o < n) {
            const uint2 c = cells[o];
            const uint32_t g0 = c.x & 0xFFFFu, g1 = c.x >> 16, g2 = c.y & 0xFFFFu;
            v[0] = 65535u - g0; v[1] = 65535u - g1; v[2] = 65535u - g2; v[3] = g0; v[4] = g1; v[5] = g2;
        }
    }
    const uint32_t grp0 = __builtin_amdgcn_readfirstlane(grp);
    if (__ballot(grp != grp0) == 0ull) {                         // one group in the wave: six atomics for all of it
#pragma unroll
        for (int k = 0; k < 6; ++k)
            for (int off = 32; off > 0; off >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v[k], off); v[k] = w > v[k] ? w : v[k]; }
        if ((threadIdx.x & 63u) == 0u && step)
            for (int k = 0; k < 6; ++k) atomicMax(&bounds[6 * (size_t)grp + k], v[k]);
    } else if (valid && step) {
        for (int k = 0; k < 6; ++k) atomicMax(&bounds[6 * (size_t)grp + k], v[k]);
    }
}

__global__ void __launch_bounds__(kBlock) k_bvh_median_keys(uint2* pairs, const uint2* __restrict__ cells, const uint32_t* __restrict__ gs, uint32_t groups,
                                                            const uint32_t* __restrict__ bounds, MedianCell cell, uint32_t n, uint32_t index_bits, uint32_t mask) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t o = pairs[p].x & mask;
    const uint32_t grp = median_group(gs, groups, p);
    const uint32_t start = gs[grp];
    uint32_t v = p - (start & 0x7FFFFFFFu);                      // no step: the position stays (a group has at most 65536)
    if ((start >> 31) != 0u) {
        const uint32_t* b = bounds + 6 * (size_t)grp;
        const uint32_t axis = median_axis(b[0], b[1], b[2], b[3], b[4], b[5], cell);
        const uint2 c = cells[o < n ? o : 0u];
        v = axis == 0u ? c.x & 0xFFFFu : axis == 1u ? c.x >> 16 : c.y & 0xFFFFu;
    }
    const unsigned long long key = ((unsigned long long)grp << (16u + index_bits)) | ((unsigned long long)(v & 0xFFFFu) << index_bits) | o;
    pairs[p] = make_uint2((uint32_t)key, (uint32_t)(key >> 32));
}

__global__ void __launch_bounds__(kBlock) k_bvh_median_unpack(const uint2* __restrict__ in, uint2* __restrict__ out, uint32_t n, uint32_t mask) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) out[p] = make_uint2(0u, in[p].x & mask);
}

// One workgroup per tile.  The tile's objects (cells and index) stand in LDS in position order; level by level every step of
// the tile takes its bounds (LDS atomics), its axis, and then every position its rank among the keys (cell << 32 | index) of
// its step -- the keys differ, so the ranks are the new positions.  Positions no step of a level covers stay.
__global__ void __launch_bounds__(kMedianBlock) k_bvh_median_tile(const uint2* __restrict__ in, uint2* __restrict__ out, const uint2* __restrict__ cells,
                                                                  const uint4* __restrict__ tiles, const uint2* __restrict__ tile_steps, MedianCell cell,
                                                                  uint32_t n, uint32_t mask) {
    __shared__ uint32_t e_g01[kMedianT], e_g2[kMedianT], e_obj[kMedianT];
    __shared__ unsigned long long key[kMedianT];
    __shared__ uint2 steps[kMedianMaxSteps];
    __shared__ uint32_t bnd[6 * kMedianMaxSteps];
    __shared__ uint32_t axis_of[kMedianMaxSteps];
    const uint32_t tid = threadIdx.x;
    const uint4 tl = tiles[blockIdx.x];
    const uint32_t p0 = tl.x;
    if (tl.y > n || tl.y <= p0) return;                          // (uniform; the plan never says so)
    const uint32_t size = tl.y - p0 < kMedianT ? tl.y - p0 : kMedianT;
    const uint32_t n_steps = tl.w < kMedianMaxSteps ? tl.w : kMedianMaxSteps;
    for (uint32_t s = tid; s < n_steps; s += kMedianBlock) steps[s] = tile_steps[tl.z + s];
    for (uint32_t p = tid; p < size; p += kMedianBlock) {
        uint32_t o = in[p0 + p].x & mask;
        o = o < n ? o : 0u;
        const uint2 c = cells[o];
        e_g01[p] = c.x; e_g2[p] = c.y & 0xFFFFu; e_obj[p] = o;
    }
    __syncthreads();
    for (uint32_t s0 = 0u; s0 < n_steps;) {
        const uint32_t level = steps[s0].x >> 16;
        uint32_t s1 = s0 + 1u;
        while (s1 < n_steps && (steps[s1].x >> 16) == level) ++s1;
        const uint32_t cnt = s1 - s0;
        for (uint32_t k = tid; k < 6u * cnt; k += kMedianBlock) bnd[k] = 0u;
        __syncthreads();
        // the step of each of this thread's positions: the last one of the level that starts at or before it, if it reaches it
        uint32_t mine[kMedianPer];
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e) {
            const uint32_t p = tid + e * kMedianBlock;
            mine[e] = 0xFFFFFFFFu;
            if (p < size && (steps[s0].x & 0xFFFFu) <= p) {
                uint32_t lo = s0, hi = s1;
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((steps[mid].x & 0xFFFFu) <= p) lo = mid; else hi = mid;
                }
                if (p < steps[lo].y && steps[lo].y <= size) {
                    mine[e] = lo - s0;
                    const uint32_t g01 = e_g01[p], g0 = g01 & 0xFFFFu, g1 = g01 >> 16, g2 = e_g2[p];
                    uint32_t* b = bnd + 6u * mine[e];
                    atomicMax(b, 65535u - g0); atomicMax(b + 1, 65535u - g1); atomicMax(b + 2, 65535u - g2);
                    atomicMax(b + 3, g0); atomicMax(b + 4, g1); atomicMax(b + 5, g2);
                }
            }
        }
        __syncthreads();
        for (uint32_t k = tid; k < cnt; k += kMedianBlock) {
            const uint32_t* b = bnd + 6u * k;
            axis_of[k] = median_axis(b[0], b[1], b[2], b[3], b[4], b[5], cell);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e) {
            const uint32_t p = tid + e * kMedianBlock;
            if (mine[e] != 0xFFFFFFFFu) {
                const uint32_t axis = axis_of[mine[e]], g01 = e_g01[p];
                const uint32_t v = axis == 0u ? g01 & 0xFFFFu : axis == 1u ? g01 >> 16 : e_g2[p];
                key[p] = ((unsigned long long)v << 32) | e_obj[p];
            }
        }
        __syncthreads();
        uint32_t to[kMedianPer], m_g01[kMedianPer], m_g2[kMedianPer], m_obj[kMedianPer];
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e) {
            const uint32_t p = tid + e * kMedianBlock;
            to[e] = 0xFFFFFFFFu; m_g01[e] = 0u; m_g2[e] = 0u; m_obj[e] = 0u;
            if (mine[e] != 0xFFFFFFFFu) {
                const uint2 st = steps[s0 + mine[e]];
                const uint32_t first = st.x & 0xFFFFu, last = st.y;
                const unsigned long long mk = key[p];
                uint32_t rank = 0u;
                for (uint32_t j = first; j < last; ++j) rank += key[j] < mk ? 1u : 0u;
                to[e] = first + rank;                            // < last: the position's own key is not below itself
                m_g01[e] = e_g01[p]; m_g2[e] = e_g2[p]; m_obj[e] = e_obj[p];
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e)
            if (to[e] < size) { e_g01[to[e]] = m_g01[e]; e_g2[to[e]] = m_g2[e]; e_obj[to[e]] = m_obj[e]; }
        __syncthreads();
        s0 = s1;
    }
    for (uint32_t p = tid; p < size; p += kMedianBlock) out[p0 + p] = make_uint2(0u, e_obj[p]);
}
}  // namespace PTK_IMPL
namespace ptk {
uint32_t launch_bvh_median(const BvhMedianArgs& a, const BvhMedianLevel* levels, uint32_t n_levels, hipStream_t st) {
    const BvhBuildArgs& b = a.b;
    if (!b.n) return 0u;
    const dim3 grid((b.n + kBlock - 1) / kBlock), block(kBlock);
    const uint32_t mask = a.index_bits >= 32u ? 0xFFFFFFFFu : (1u << a.index_bits) - 1u;
    const PTK_IMPL::MedianCell cell = {{b.grid_cell[0], b.grid_cell[1], b.grid_cell[2]}};
    hipLaunchKernelGGL(PTK_IMPL::k_bvh_cells, grid, block, 0, st, b, a.cells);
    uint32_t cur = 0u;
    for (uint32_t l = 0; l < n_levels; ++l) {
        const BvhMedianLevel& lv = levels[l];
        const uint32_t* gs = a.group_start + lv.first;
        (void)hipMemsetAsync(a.bounds, 0, 6 * (size_t)lv.groups * sizeof(uint32_t), st);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_bounds, grid, block, 0, st, (const uint2*)b.pairs[cur], (const uint2*)a.cells, gs, lv.groups, a.bounds, b.n, mask);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_keys, grid, block, 0, st, b.pairs[cur], (const uint2*)a.cells, gs, lv.groups, (const uint32_t*)a.bounds, cell, b.n,
                           a.index_bits, mask);
        cur = bvh_sort_passes(b, cur, (a.index_bits + 16u + lv.bits + 7u) / 8u, st);
    }
    hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_unpack, grid, block, 0, st, (const uint2*)b.pairs[cur], b.pairs[cur ^ 1u], b.n, mask);
    if (a.n_tiles)
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_tile, dim3(a.n_tiles), dim3(PTK_IMPL::kMedianBlock), 0, st, (const uint2*)b.pairs[cur], b.pairs[cur ^ 1u],
                           (const uint2*)a.cells, a.tiles, a.tile_steps, cell, b.n, mask);
    return cur ^ 1u;
}
}  // namespace ptk

// ------------------------------------------------------------------ temporal gradients (pt_temporal_gradient_device)
// The rule is pt_gradient.h and DESIGN.md 5h: one gradient pixel per 3 x 3 stratum, re-traced in the current scene with the
// previous frame's samples (a pixel-list render between k_gradient_list and k_gradient_strata), its change of luminance
// spread over a window of strata into every pixel's blend weight.  f64 + - * / and comparisons only: the same bits as the
// host compiler's.
#include "pt_gradient.h"
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
// goes through tm_reproject (f64, the temporal kernel's own lookup) to the previous-image pixel whose stratum measured it.
// One float4 of features, the solve, then the window of 16-byte records; NaN where there is nothing to look up.
__global__ void __launch_bounds__(kDnBx * kDnBy) k_gradient_alpha_camera(GradientArgs a, TemporalArgs t) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    uint32_t xi = x, yi = y;
    bool ok = true;
    if (!t.same_camera) {
        const float d = t.dn.feat[2 * p + 1].w;
        double xr = 0.0, yr = 0.0, dexp = 0.0;
        ok = d > 0.0f && tm_reproject(t, x, y, d, xr, yr, dexp) && ptgr::lookup_pixel(xr, yr, a.width, a.height, &xi, &yi);
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
    const dim3 g((a.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_gradient_alpha, g, b, 0, st, a);
}
void launch_gradient_alpha_camera(const GradientArgs& a, const TemporalArgs& t, hipStream_t st) {
    const dim3 g((a.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_gradient_alpha_camera, g, b, 0, st, a, t);
}
}  // namespace ptk

// ------------------------------------------------------------------ ... and the temporal accumulation that takes them (pt_denoise_temporal_alpha_device)
// k_denoise_temporal_motion with one change: rule 4's least blend weight is alpha[p] where that entry is finite and in
// [0, 1], t.alpha elsewhere.  The other statements are that kernel's, in its order (the kernel's own text, as
// k_denoise_temporal_motion has its own copy of k_denoise_temporal's): with a plane that holds no usable entry, or one
// constant c against t.alpha = c, the two kernels write the same bits.
namespace PTK_IMPL {
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal_alpha(TemporalAlphaArgs g) {
    const TemporalMotionArgs& m = g.m;
    const TemporalArgs& a = m.t;
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.dn.width || y >= a.dn.height) return;
    const int W = (int)a.dn.width, H = (int)a.dn.height;
    const size_t p = (size_t)y * a.dn.width + x;
    const float4 f0p = a.dn.feat[2 * p], f1p = a.dn.feat[2 * p + 1];
    const float3 uc = dn_demod(a.dn, p);
    const float Lc = dn_lum(uc.x, uc.y, uc.z);
    // the caller's id: checked against the scene before it indexes the maps
    const int32_t id = m.ids[p];
    const bool known = id >= 0 && (uint32_t)id < m.n_objs;
    const uint32_t flags = known ? m.maps[id].flags : 2u;
    const bool ident = flags == 1u;
    const float idf = known ? (float)(id + 1) : 0.0f;       // n_objs <= 2^24 - 2: exact
    float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hm1 = 0.0f, hm2 = 0.0f, hn = 0.0f;
    if (a.hist_src && f1p.w > 0.0f && !(flags & 2u)) {
        double xr = x, yr = y, dexp = f1p.w;
        float nx = f1p.x, ny = f1p.y, nz = f1p.z;
        bool ok = true;
        if (!(ident && a.same_camera)) {
            const MotionMap* mp = ident ? nullptr : m.maps + id;
            ok = tmm_reproject(a, mp, x, y, f1p.w, xr, yr, dexp);
            if (mp) {                         // n_h = A n_p, normalised in f64 (n_p when its length is 0)
                double v[3];
                for (int k = 0; k < 3; ++k) v[k] = mp->a[3 * k] * (double)f1p.x + mp->a[3 * k + 1] * (double)f1p.y + mp->a[3 * k + 2] * (double)f1p.z;
                const double len = __builtin_sqrt(tm_dot(v, v));
                if (len > 0.0) { nx = (float)(v[0] / len); ny = (float)(v[1] / len); nz = (float)(v[2] / len); }
            }
        }
        if (ok && xr > -1.0 && xr < (double)W && yr > -1.0 && yr < (double)H) {
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
                    if (h1.w != 0.0f && h1.w != idf) {       // another object's history: only when neither object moved
                        if (!ident || !(h1.w >= 1.0f && h1.w <= (float)m.n_objs)) continue;
                        if (m.maps[(uint32_t)h1.w - 1u].flags != 1u) continue;
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
        const float ap = g.alpha[p];
        const float al = fmaxf(ap >= 0.0f && ap <= 1.0f ? ap : a.alpha, 1.0f / n);      // (NaN fails both comparisons)
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
}  // namespace PTK_IMPL
namespace ptk {
void launch_denoise_temporal_alpha(const TemporalAlphaArgs& a, hipStream_t st) {
    const dim3 g((a.m.t.dn.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.m.t.dn.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy),
        b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal_alpha, g, b, 0, st, a);
}
}  // namespace ptk

// ------------------------------------------------------------------ auto-exposure and tone mapping (pt_tonemap_device)
// The rule is pt_tonemap.h and DESIGN.md 5k.  k_film_histogram reads the film once (12 B per pixel), k_exposure_meter is one
// wave, k_tonemap reads 12 B and writes 4 (+ 12 with the float plane) per pixel.  The exposure never visits the host: the
// meter leaves it in device words and k_tonemap reads it there.
#include "pt_tonemap.h"
namespace PTK_IMPL {
constexpr uint32_t kHistBlock = 1024;          // one workgroup per compute unit: few workgroups, few flushes
constexpr uint32_t kHistBatch = 4;             // pixels per thread whose loads are in flight together
constexpr uint32_t kHistRounds = 4;            // in-wave reduction: bins settled by one LDS add of a lane count before the rest add singly
// One word per lane and pixel into the workgroup's LDS histogram.  A wave's pixels fall into a few words on most films (a
// wall, the black background): in each of the first kHistRounds rounds the first lane still waiting broadcasts its word, the
// lanes that hold the same word are counted by a ballot and that lane adds the count; what is left after them -- a wave
// whose lanes all differ -- adds singly, without conflicts.  Integer counts: no order to depend on.
PT_DEV void hist_add(uint32_t* s_hist, bool have, uint32_t w, uint32_t lane) {
    unsigned long long todo = __ballot(have);
    for (uint32_t r = 0; r < kHistRounds && todo != 0ull; ++r) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t wf = (uint32_t)__shfl((int)w, first);
        const unsigned long long same = __ballot(have && w == wf);
        if (lane == (uint32_t)first) atomicAdd(&s_hist[wf], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&s_hist[w], 1u);
}
__global__ void __launch_bounds__(kHistBlock) k_film_histogram(const float* __restrict__ lin, uint32_t np, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[ptone::kWords];
    for (uint32_t k = threadIdx.x; k < ptone::kWords; k += kHistBlock) s_hist[k] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
    // (the loop's bounds are the workgroup's: every lane of a wave takes every ballot)
    for (uint64_t base = (uint64_t)blockIdx.x * kHistBlock; base < np; base += kHistBatch * stride) {
        uint32_t w[kHistBatch];
        bool have[kHistBatch];
#pragma unroll
        for (uint32_t k = 0; k < kHistBatch; ++k) {
            const uint64_t p = base + k * stride + threadIdx.x;
            have[k] = p < np;
            w[k] = 0u;
            if (have[k]) w[k] = ptone::word(ptone::lum(lin[3 * p], lin[3 * p + 1], lin[3 * p + 2]));
        }
#pragma unroll
        for (uint32_t k = 0; k < kHistBatch; ++k) hist_add(s_hist, have[k], w[k], lane);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < ptone::kWords; k += kHistBlock)
        if (s_hist[k] != 0u) atomicAdd(&hist[k], s_hist[k]);
}

// One wave: lane i holds bins 4 i .. 4 i + 3.  The ranks in front of a lane's bins come from an inclusive scan of the lane
// sums (integers, exact); the window sums are ptone::meter_lane per lane and six butterfly steps -- the order ptone::meter
// restates on the host --, and lane 0 writes the state.
__global__ void __launch_bounds__(64) k_exposure_meter(ExposureArgs a) {
    const uint32_t lane = threadIdx.x;
    uint32_t n[ptone::kBinsPerLane];
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t j = 0; j < ptone::kBinsPerLane; ++j) { n[j] = a.hist[ptone::kBinsPerLane * lane + j]; mine += n[j]; }
    uint32_t incl = mine;                          // (the words add up to W H <= 2^30: no overflow)
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    const double lo = (double)a.pct_lo * (double)total, hi = (double)a.pct_hi * (double)total;
    double s, w;
    uint32_t point;
    ptone::meter_lane(n, ptone::kBinsPerLane * lane, (uint64_t)(incl - mine), lo, hi, &s, &w, &point);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off); w += __shfl_xor(w, off);
        const uint32_t other = (uint32_t)__shfl_xor((int)point, off);
        point = other < point ? other : point;
    }
    if (lane != 0u) return;
    const ExposureState old = *a.state;
    const bool fresh = old.valid == 0u || old.width != a.width || old.height != a.height;
    ExposureState next{};
    next.log2E = ptone::adapt(total, s, w, point, a.key, a.log2_min, a.log2_max, a.adapt, fresh, old.log2E);
    next.E = ptone::exposure(next.log2E);
    next.valid = 1u; next.width = a.width; next.height = a.height;
    *a.state = next;
}

// One thread per pixel: curve and transfer.  The pixel's three floats are read before any is written: out_linear may be linear.
__global__ void __launch_bounds__(kBlock) k_tonemap(TonemapArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.np) return;
    const float E = a.e_dev ? *a.e_dev : a.e_manual;
    const float c[3] = {a.linear[3 * (size_t)p], a.linear[3 * (size_t)p + 1], a.linear[3 * (size_t)p + 2]};
    float y[3];
    ptone::curve(a.curve, E, a.white, c, y);
    if (a.out_linear) { a.out_linear[3 * (size_t)p] = y[0]; a.out_linear[3 * (size_t)p + 1] = y[1]; a.out_linear[3 * (size_t)p + 2] = y[2]; }
    *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * (size_t)p) = ptone::rgba8(a.transfer, y);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_film_histogram(const float* linear, uint32_t np, uint32_t* hist, uint32_t n_cus, hipStream_t st) {
    const uint32_t need = (np + PTK_IMPL::kHistBlock - 1) / PTK_IMPL::kHistBlock;
    if (np) hipLaunchKernelGGL(PTK_IMPL::k_film_histogram, dim3(need < n_cus ? need : n_cus), dim3(PTK_IMPL::kHistBlock), 0, st, linear, np, hist);
}
void launch_exposure_meter(const ExposureArgs& a, hipStream_t st) { hipLaunchKernelGGL(PTK_IMPL::k_exposure_meter, dim3(1), dim3(64), 0, st, a); }
void launch_tonemap(const TonemapArgs& a, hipStream_t st) {
    if (a.np) hipLaunchKernelGGL(PTK_IMPL::k_tonemap, dim3((a.np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
}  // namespace ptk
