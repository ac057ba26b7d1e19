// pt_film_cascade.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_cascade.h"

// ------------------------------------------------------------------ brightness cascade (pt_render_cascade_device, rule: pt_cascade.h)
// The rule is pt_cascade.h and DESIGN.md 5n.  k_resolve_cascade stands in for k_resolve: the same reads of the sample buffer, the
// plain sums P beside the K layer sums.  k_cascade_reweight reads a pixel's sums once and the counts of its 3 x 3 block out of LDS.
namespace PTK_IMPL {
PT_DEV ptcas::Levels cascade_levels(const double (&B)[8], double kappa, uint32_t K) {
    ptcas::Levels lv;
#pragma unroll
    for (int k = 0; k < 8; ++k) lv.B[k] = B[k];
    lv.kappa = kappa; lv.K = K;
    return lv;
}

// One thread per pixel; the state is planar (plane 3 k + c = S_k.c, planes 3 K + c = P.c; np doubles each), so a wave's loads and
// stores are whole lines.  The layer a sample goes to is data-dependent: the sums are held in registers and every layer takes a
// predicated add (ptcas::add_sample, K a compile-time constant), so nothing is indexed by a run-time value and the kernel has
// no scratch.
template <uint32_t K>
__global__ void __launch_bounds__(kBlock) k_resolve_cascade(CascadeResolveArgs a) {
    if (blockIdx.x == 0u && a.zero_words)
        for (uint32_t k = threadIdx.x; k < a.n_zero; k += kBlock) a.zero_words[k] = 0u;
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.np) return;
    const ptcas::Levels lv = cascade_levels(a.B, a.kappa, K);
    const size_t np = a.np;
    double S[K][3], P[3];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k)
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) S[k][c] = a.load ? a.state[(3 * k + c) * np + p] : 0.0;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) P[c] = a.load ? a.state[(3 * K + c) * np + p] : 0.0;
    uint32_t s = 0;
    for (; s + 4u <= a.nb; s += 4u) {              // four samples' loads in flight before the ordered additions (as k_resolve)
        Rgb v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = a.lsamp[(size_t)(s + k) * np + p];
#pragma unroll
        for (int k = 0; k < 4; ++k) ptcas::add_sample<K>(lv, v[k].r, v[k].g, v[k].b, S, P);
    }
    for (; s < a.nb; ++s) {
        const Rgb v = a.lsamp[(size_t)s * np + p];
        ptcas::add_sample<K>(lv, v.r, v.g, v.b, S, P);
    }
#pragma unroll
    for (uint32_t k = 0; k < K; ++k)
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) a.state[(3 * k + c) * np + p] = S[k][c];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) a.state[(3 * K + c) * np + p] = P[c];
    if (!a.finalize) return;
    double lum[K];
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) lum[k] = ptcas::layer_luminance(S[k][0], S[k][1], S[k][2]);
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) a.cnt[k * np + p] = ptcas::count(lv, lum, k);
}

// One workgroup per 16 x 16 pixel tile; the K count planes of the tile and a one-pixel halo (18 x 18 each) go through LDS.
constexpr uint32_t kCasTile = 16, kCasHalo = kCasTile + 2;
__global__ void __launch_bounds__(kCasTile * kCasTile) k_cascade_reweight(CascadeReweightArgs a) {
    __shared__ double s_cnt[ptcas::kMaxLayers][kCasHalo][kCasHalo];
    const uint32_t W = a.width, H = a.height;
    const size_t np = (size_t)W * H;
    const int x0 = (int)(blockIdx.x * kCasTile) - 1, y0 = (int)(blockIdx.y * kCasTile) - 1;
    for (uint32_t i = threadIdx.x; i < a.K * kCasHalo * kCasHalo; i += kCasTile * kCasTile) {
        const uint32_t j = i / (kCasHalo * kCasHalo), rem = i - j * (kCasHalo * kCasHalo), ty = rem / kCasHalo, tx = rem - ty * kCasHalo;
        const int gx = x0 + (int)tx, gy = y0 + (int)ty;
        const bool in = gx >= 0 && gy >= 0 && gx < (int)W && gy < (int)H;
        s_cnt[j][ty][tx] = in ? a.cnt[j * np + (size_t)gy * W + (uint32_t)gx] : 0.0;      // (a tap outside the image is never read)
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % kCasTile, ly = threadIdx.x / kCasTile;
    const uint32_t x = blockIdx.x * kCasTile + lx, y = blockIdx.y * kCasTile + ly;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const ptcas::Levels lv = cascade_levels(a.B, a.kappa, a.K);
    const double dn = (double)a.n_total;
    double acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < a.K; ++j) {
        double sum = 0.0;
        uint32_t taps = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int gx = (int)x + dx - 1, gy = (int)y + dy - 1;
                if (gx >= 0 && gy >= 0 && gx < (int)W && gy < (int)H) { sum += s_cnt[j][ly + dy][lx + dx]; ++taps; }
            }
        const double w = ptcas::weight(lv, j, s_cnt[j][ly + 1u][lx + 1u], sum / (double)taps);
        if (a.out_weights) a.out_weights[j * np + p] = (float)w;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) acc[c] += w * a.state[(3 * j + c) * np + p];
    }
    uint32_t q8 = 0xFF000000u;                                                    // alpha 255, world.rs:331
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        const double m = acc[c] / dn;
        a.out_linear[3 * p + c] = (float)m;
        q8 |= ptcas::byte8(m) << (8 * c);
        if (a.out_plain) a.out_plain[3 * p + c] = (float)(a.state[(3 * a.K + c) * np + p] / dn);
    }
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * p) = q8;
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_resolve_cascade(const CascadeResolveArgs& a, hipStream_t st) {
    if (!a.np) return;
    const dim3 g((a.np + kBlock - 1) / kBlock), b(kBlock);
    switch (a.K) {
    case 2: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<2>, g, b, 0, st, a); break;
    case 3: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<3>, g, b, 0, st, a); break;
    case 4: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<4>, g, b, 0, st, a); break;
    case 5: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<5>, g, b, 0, st, a); break;
    case 6: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<6>, g, b, 0, st, a); break;
    case 7: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<7>, g, b, 0, st, a); break;
    default: hipLaunchKernelGGL(PTK_IMPL::k_resolve_cascade<8>, g, b, 0, st, a); break;
    }
}
void launch_cascade_reweight(const CascadeReweightArgs& a, hipStream_t st) {
    const dim3 g((a.width + PTK_IMPL::kCasTile - 1) / PTK_IMPL::kCasTile, (a.height + PTK_IMPL::kCasTile - 1) / PTK_IMPL::kCasTile);
    hipLaunchKernelGGL(PTK_IMPL::k_cascade_reweight, g, dim3(PTK_IMPL::kCasTile * PTK_IMPL::kCasTile), 0, st, a);
}
}  // namespace ptk
