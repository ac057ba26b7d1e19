// pt_film_filter.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_filter.h"

// ------------------------------------------------------------------ reconstruction filter (pt_render_filtered_device, rule: pt_filter.h)
// The rule is pt_filter.h and DESIGN.md 5o.  k_resolve_filter<M> stands in for k_resolve: an output pixel gathers the samples
// of the (2 M + 1)^2 pixels around it, each weighted by the filter at the sample's own position, which is recomputed from the
// Philox block the camera ray took its jitter from.
static_assert(PT_PHILOX_ROUNDS == ptflt::kPhiloxRounds, "pt_filter.h restates the camera block of pt_device.h");
namespace PTK_IMPL {
constexpr uint32_t kFltTile = 16;
// samples staged together: what keeps a workgroup's LDS under 40 KiB, so that four of them share a CU (28 / 38 / 36 KiB)
template <int M> struct FltDepth { static constexpr uint32_t value = M == 0 ? 4u : (M == 1 ? 2u : 1u); };

PT_DEV ptflt::Rule filter_rule(const FilterResolveArgs& a) {
    ptflt::Rule r;
    r.kind = a.kind; r.m = a.m; r.R = a.R; r.alpha = a.alpha; r.gR = a.gR;
    r.a3 = a.a3; r.a2 = a.a2; r.a0 = a.a0; r.b3 = a.b3; r.b2 = a.b2; r.b1 = a.b1; r.b0 = a.b0;
    return r;
}

// One workgroup per 16 x 16 output tile, one thread per output pixel.  Per staged sample the (16 + 2 M)^2 pixels the tile reads
// go through LDS: the RGB record as f32 (planar) and, evaluated ONCE per sample here, its 2 (2 M + 1) one-dimensional factors
// as f64 (planar by factor index, so that a wave's reads of one factor are consecutive doubles).  A tap is then two factor
// reads, one product and the record.  A halo pixel outside the image is never read: its factors are staged as 0, and a weight
// of exactly 0 is skipped by the rule's own select.  The state is planar (7 planes of np doubles).  Every thread reaches every
// barrier; threads of a partial tile outside the image only help staging.
template <int M>
__global__ void __launch_bounds__(kFltTile * kFltTile) k_resolve_filter(FilterResolveArgs a) {
    constexpr uint32_t T = kFltTile + 2 * M, TT = T * T, F = 2 * M + 1, S = FltDepth<M>::value, NT = kFltTile * kFltTile;
    __shared__ float s_rgb[S][3][TT];
    __shared__ double s_fx[S][F][TT];
    __shared__ double s_fy[S][F][TT];
    if (blockIdx.x == 0u && blockIdx.y == 0u && a.zero_words)
        for (uint32_t k = threadIdx.x; k < a.n_zero; k += NT) a.zero_words[k] = 0u;
    const ptflt::Rule rule = filter_rule(a);
    const uint32_t W = a.width, H = a.height;
    const size_t np = (size_t)W * H;
    const uint32_t lx = threadIdx.x % kFltTile, ly = threadIdx.x / kFltTile;
    const uint32_t x = blockIdx.x * kFltTile + lx, y = blockIdx.y * kFltTile + ly;
    const bool active = x < W && y < H;
    const size_t q = active ? (size_t)y * W + x : 0;
    const int x0 = (int)(blockIdx.x * kFltTile) - M, y0 = (int)(blockIdx.y * kFltTile) - M;
    double A[3] = {0.0, 0.0, 0.0}, Wt = 0.0, P[3] = {0.0, 0.0, 0.0};
    if (active && a.load) {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) { A[c] = a.state[c * np + q]; P[c] = a.state[(4 + c) * np + q]; }
        Wt = a.state[3 * np + q];
    }
    for (uint32_t s0 = 0; s0 < a.nb; s0 += S) {
        const uint32_t ns = a.nb - s0 < S ? a.nb - s0 : S;
        for (uint32_t i = threadIdx.x; i < ns * TT; i += NT) {
            const uint32_t ss = i / TT, rem = i - ss * TT, hy = rem / T, hx = rem - hy * T;
            const int gx = x0 + (int)hx, gy = y0 + (int)hy;
            const bool in = gx >= 0 && gy >= 0 && gx < (int)W && gy < (int)H;
            Rgb v{0.0f, 0.0f, 0.0f};
            double fx[F], fy[F];
#pragma unroll
            for (uint32_t k = 0; k < F; ++k) { fx[k] = 0.0; fy[k] = 0.0; }
            if (in) {
                v = a.lsamp[(size_t)(s0 + ss) * np + (size_t)gy * W + (uint32_t)gx];
                double ox, oy;
                ptflt::offsets((uint32_t)gx, (uint32_t)gy, a.first_sample + s0 + ss, &ox, &oy);
                ptflt::factors<M>(rule, ox, oy, fx, fy);
            }
            s_rgb[ss][0][rem] = v.r; s_rgb[ss][1][rem] = v.g; s_rgb[ss][2][rem] = v.b;
#pragma unroll
            for (uint32_t k = 0; k < F; ++k) { s_fx[ss][k][rem] = fx[k]; s_fy[ss][k][rem] = fy[k]; }
        }
        __syncthreads();
        for (uint32_t ss = 0; ss < ns; ++ss) {
#pragma unroll
            for (uint32_t jj = 0; jj < F; ++jj)
#pragma unroll
                for (uint32_t kk = 0; kk < F; ++kk) {
                    const uint32_t h = (ly + jj) * T + lx + kk;                 // the tap's pixel: px - qx = kk - M, py - qy = jj - M
                    const double w = s_fx[ss][kk][h] * s_fy[ss][jj][h];
                    ptflt::add_tap(w, s_rgb[ss][0][h], s_rgb[ss][1][h], s_rgb[ss][2][h], A, Wt);
                }
            const uint32_t own = (ly + M) * T + lx + M;
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) P[c] += (double)s_rgb[ss][c][own];
        }
        __syncthreads();
    }
    if (!active) return;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) { a.state[c * np + q] = A[c]; a.state[(4 + c) * np + q] = P[c]; }
    a.state[3 * np + q] = Wt;
    if (!a.finalize) return;
    const double dn = (double)a.n_total;
    uint32_t q8 = 0xFF000000u;                                                    // alpha 255, world.rs:331
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        const double m = ptflt::mean(A[c], Wt, P[c], dn);
        a.out_linear[3 * q + c] = (float)m;
        q8 |= ptcas::byte8(m) << (8 * c);
        if (a.out_plain) a.out_plain[3 * q + c] = (float)(P[c] / dn);
    }
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * q) = q8;
    if (a.out_wsum) a.out_wsum[q] = Wt;
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_resolve_filter(const FilterResolveArgs& a, hipStream_t st) {
    if (!a.width || !a.height) return;
    const dim3 g((a.width + PTK_IMPL::kFltTile - 1) / PTK_IMPL::kFltTile, (a.height + PTK_IMPL::kFltTile - 1) / PTK_IMPL::kFltTile);
    const dim3 b(PTK_IMPL::kFltTile * PTK_IMPL::kFltTile);
    switch (a.m) {
    case 0: hipLaunchKernelGGL(PTK_IMPL::k_resolve_filter<0>, g, b, 0, st, a); break;
    case 1: hipLaunchKernelGGL(PTK_IMPL::k_resolve_filter<1>, g, b, 0, st, a); break;
    default: hipLaunchKernelGGL(PTK_IMPL::k_resolve_filter<2>, g, b, 0, st, a); break;
    }
}
}  // namespace ptk
