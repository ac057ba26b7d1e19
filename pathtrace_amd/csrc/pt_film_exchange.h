// pt_film_exchange.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"

// ------------------------------------------------------------------ multi-GPU film exchange (pt_multi.cpp)
namespace PTK_IMPL {
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
}  // namespace PTK_IMPL
namespace ptk {
void launch_film_pack(const float* lin, const uint8_t* rgba, uint32_t np, void* packed, hipStream_t st) {
    if (np) hipLaunchKernelGGL(PTK_IMPL::k_film_pack, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, lin, rgba, np, (uint4*)packed);
}
void launch_film_unpack(const void* recv, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_dev, uint32_t max_rows, float* lin,
                        uint8_t* rgba, hipStream_t st) {
    if (W * H) hipLaunchKernelGGL(PTK_IMPL::k_film_unpack, dim3((W * H + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint4*)recv, W, H,
                                  band_rows, n_dev, max_rows, lin, rgba);
}
}  // namespace ptk
