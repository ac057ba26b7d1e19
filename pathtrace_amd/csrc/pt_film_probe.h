// pt_film_probe.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_film_denoise.h"      // the pixel tile (kDnBx x kDnBy) and dn_grid
#include "pt_probe_grid.h"

// ------------------------------------------------------------------ irradiance volume (rule: pt_probe_grid.h)
//   k_probe_positions   one thread per probe: the f32 position of the rule, 12 bytes.
//   k_probe_shade       one thread per pixel, the denoiser's tile.  The record is two 16-byte loads; a lit pixel gathers the 27
//                       floats of its cell's eight corners straight from global memory (neighbouring pixels share a cell, so a
//                       wave's loads fall on a few cache lines) into 27 f64 sums, an unlit one reads its fallback pixel and no
//                       probe.  The fallback may be the output plane: a thread reads its own 12 bytes before it writes them.
//                       (A form that staged the table in LDS first was no faster: docs/EXPERIMENTS.md "Irradiance volume".)
namespace PTK_IMPL {
__global__ void __launch_bounds__(kBlock) k_probe_positions(ptgrid::Grid g, uint32_t n, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    float v[3];
    ptgrid::position(g, p, v);
    out[3 * (size_t)p] = v[0]; out[3 * (size_t)p + 1] = v[1]; out[3 * (size_t)p + 2] = v[2];
}
__global__ void __launch_bounds__(kDnBx * kDnBy) k_probe_shade(ProbeShadeArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float4 f0 = a.feat[2 * p], f1 = a.feat[2 * p + 1];
    const float rec[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
    float v[3];
    if (!ptgrid::shade(a.grid, a.normal_bias, a.weight, a.width, a.height, x, y, rec, a.cam, a.sh27, v)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = a.fallback ? a.fallback[3 * p + k] : 0.0f;
    }
    a.out_linear[3 * p] = v[0]; a.out_linear[3 * p + 1] = v[1]; a.out_linear[3 * p + 2] = v[2];
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * p) = ptgrid::rgba8(v);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_probe_positions(const ptgrid::Grid& g, uint32_t n, float* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(PTK_IMPL::k_probe_positions, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, g, n, out);
}
void launch_probe_shade(const ProbeShadeArgs& a, hipStream_t st) {
    const dim3 g = dn_grid(a.width, a.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_probe_shade, g, b, 0, st, a);
}
}  // namespace ptk
