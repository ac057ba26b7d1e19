// pt_film_upsample.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_film_denoise.h"
#include "pt_upsample.h"

// ------------------------------------------------------------------ feature-guided upsampling (pt_upsample_device)
// The rule is pt_upsample.h and DESIGN.md 5l.  One thread per full-size pixel in the a-trous block shape: a wave covers 32 x 2
// output pixels, whose taps lie in two or three rows of at most 32 / r + 2 low pixels.  Per output pixel 32 B of its own record
// in (two 16-byte loads), 12 B + 4 B out (the RGBA8 word as one store); per tap two 16-byte loads of the low record and the
// three floats of the low film, straight from the caches -- neighbouring threads share them, no LDS stage.
// The position is f64 (ptup::position), everything after it f32.
namespace PTK_IMPL {
__global__ void __launch_bounds__(kDnBx * kDnBy) k_upsample(UpsampleArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const ptup::Shape s{a.width, a.height, a.lo_width, a.lo_height};
    const ptup::Rec Fp = reinterpret_cast<const ptup::Rec*>(a.feat)[p];
    float c[3];
    ptup::pixel(s, a.lo_linear, reinterpret_cast<const ptup::Rec*>(a.lo_feat), Fp, x, y, a.sigma_n, a.sigma_d, c);
    a.out_linear[3 * p] = c[0]; a.out_linear[3 * p + 1] = c[1]; a.out_linear[3 * p + 2] = c[2];
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * p) = ptup::rgba8(c);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_upsample(const UpsampleArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(PTK_IMPL::k_upsample, dn_grid(a.width, a.height), dim3(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy), 0, st, a);
}
}  // namespace ptk
