// pt_film_bake.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_bake.h"

// ------------------------------------------------------------------ light baking: what follows the render (rule: pt_bake.h)
//   k_bake_mask   one thread per texel: an EMPTY texel's 12 bytes of the linear plane become +0.0 and its RGBA8 word the black
//                 pixel of every resolve (alpha 255); the other texels are not touched.  The texel is read as three 8-byte words.
//   k_probe_sh    one wave per probe.  Lane j adds the terms of directions j, j + 64, ... to its 27 f64 sums (9 coefficients x
//                 RGB), the direction recomputed from the rule in exact arithmetic (ptbake::Exact: nothing in it depends on this
//                 unit's arithmetic mode), then sh_wave_tree.  No LDS.
//   sh_wave_tree  the rule's tree over the 64 lanes' sums through cross-lane moves, for k_probe_sh and k_probe_update
//                 (pt_film_probe_update.h): after the step of width h lane j < h holds v[j] + v[j + h], which is all the next step
//                 reads; lane 0 ends with S.  The whole wave calls it.
namespace PTK_IMPL {
PT_DEV void sh_wave_tree(double acc[27]) {
#pragma unroll
    for (uint32_t h = ptbake::kLanes / 2; h >= 1u; h /= 2u) {
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = acc[k] + __shfl_down(acc[k], h, (int)ptbake::kLanes);
    }
}
__global__ void __launch_bounds__(kBlock) k_bake_mask(const float* __restrict__ texels6, uint32_t n, float* __restrict__ out_linear,
                                                      uint8_t* __restrict__ out_rgba) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float2* __restrict__ r = reinterpret_cast<const float2*>(texels6) + 3 * (size_t)i;
    const float2 r0 = r[0], r1 = r[1], r2 = r[2];
    const float t[6] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
    if (!ptbake::empty(t)) return;
    out_linear[3 * (size_t)i] = 0.0f; out_linear[3 * (size_t)i + 1] = 0.0f; out_linear[3 * (size_t)i + 2] = 0.0f;
    if (out_rgba) *reinterpret_cast<uint32_t*>(out_rgba + 4 * (size_t)i) = 0xFF000000u;
}
__global__ void __launch_bounds__(ptbake::kLanes) k_probe_sh(uint32_t rays_per_probe, const float* __restrict__ radiance,
                                                             float* __restrict__ sh27) {
    const uint32_t p = blockIdx.x, lane = threadIdx.x;
    double acc[27];
    ptbake::sh_lane(lane, rays_per_probe, radiance + 3 * (size_t)p * rays_per_probe, acc);
    sh_wave_tree(acc);
    if (lane != 0u) return;
#pragma unroll
    for (int k = 0; k < 27; ++k) sh27[27 * (size_t)p + k] = ptbake::sh_finish(acc[k], rays_per_probe);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_bake_mask(const float* texels6, uint32_t n, float* out_linear, uint8_t* out_rgba, hipStream_t st) {
    if (n) hipLaunchKernelGGL(PTK_IMPL::k_bake_mask, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, texels6, n, out_linear, out_rgba);
}
void launch_probe_sh(uint32_t n_probes, uint32_t rays_per_probe, const float* radiance, float* sh27, hipStream_t st) {
    if (n_probes && rays_per_probe)
        hipLaunchKernelGGL(PTK_IMPL::k_probe_sh, dim3(n_probes), dim3(ptbake::kLanes), 0, st, rays_per_probe, radiance, sh27);
}
}  // namespace ptk
