// pt_film_bloom.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_bloom.h"

// ------------------------------------------------------------------ bloom (pt_bloom_device)
// The rule is pt_bloom.h and DESIGN.md 5p: a pyramid of the film's bright part, reduced level by level, collected back up and added
// to the film.  Bandwidth-bound and small: a 1024 x 1024 film reads 12 MB, writes 12 MB, and every level costs a quarter of the
// one above.  All grids are one-dimensional (tile = blockIdx.x; tiles_x tiles per row): a long thin image has more tile rows than a
// grid's y extent takes.
namespace PTK_IMPL {
constexpr uint32_t kBloomTile = 16;                            // k_bloom_reduce: destination tile side
constexpr uint32_t kBloomSrc = 2 * kBloomTile + 2;             // 34: source tile side, the one-texel halo on each side included
constexpr uint32_t kBloomHalf = kBloomSrc / 2;                 // 17 even rows, 17 odd rows
constexpr uint32_t kBloomPitch = kBloomSrc + 1;                // 35: odd
constexpr uint32_t kBloomExpW = 32, kBloomExpH = 8;            // k_bloom_expand: destination tile
constexpr uint32_t kBloomCoarseW = kBloomExpW / 2 + 2, kBloomCoarseH = kBloomExpH / 2 + 2;   // 18 x 6
constexpr uint32_t kBloomTailBlock = 1024;

PT_DEV pbloom::Rule bloom_rule(const BloomRule& r) {
    pbloom::Rule o;
    o.T = r.T; o.k = r.k; o.clamp = r.clamp; o.s = r.s; o.oms = r.oms; o.intensity = r.intensity;
    return o;
}
// source index v - 1 clamped to [0, n - 1] (v = the index shifted up by one, so that the halo's -1 is 0)
PT_DEV uint32_t bloom_clamp1(uint32_t v, uint32_t n) { return v == 0u ? 0u : (v - 1u < n ? v - 1u : n - 1u); }

// One workgroup per 16 x 16 destination tile.  LDS layout of the 34 x 34 source tile, per channel: the rows DE-INTERLEAVED -- the
// 17 even tile rows first, then the 17 odd ones (slot(r) = (r & 1) 17 + (r >> 1)) -- at a pitch of 35 floats.  The banks of the
// 32-lane halves (b32 accesses, bank = dword address mod 32):
//   horizontal pass   item j = (slot j >> 4, x = j & 15) reads s_src[slot 35 + 2 x + k]: a half covers two adjacent slots, whose
//                     addresses differ by an odd number -- one slot on the even banks, one on the odd; writes s_h[j]: linear
//   vertical pass     thread (tx, ty) reads tile rows 2 ty + k = slots ty, 17 + ty, ty + 1, 18 + ty: s_h[tid + const], linear
// Staging walks the slots in storage order (address = i + slot): linear but for the +1 per slot, at most one two-way pair in a half
// that straddles two slots.
template <bool FIRST>
__global__ void __launch_bounds__(kBlock) k_bloom_reduce(BloomReduceArgs a) {
    static_assert(kBlock == kBloomTile * kBloomTile, "one thread per destination texel");
    __shared__ float s_src[3][kBloomSrc * kBloomPitch];
    __shared__ float s_h[3][kBloomSrc * kBloomTile];
    const uint32_t tid = threadIdx.x;
    const uint32_t X0 = (blockIdx.x % a.tiles_x) * kBloomTile, Y0 = (blockIdx.x / a.tiles_x) * kBloomTile;
    const pbloom::Rule rule = bloom_rule(a.r);
    for (uint32_t i = tid; i < kBloomSrc * kBloomSrc; i += kBlock) {
        const uint32_t slot = i / kBloomSrc, col = i % kBloomSrc;
        const uint32_t row = slot < kBloomHalf ? 2u * slot : 2u * (slot - kBloomHalf) + 1u;
        const uint32_t sx = bloom_clamp1(2u * X0 + col, a.sw), sy = bloom_clamp1(2u * Y0 + row, a.sh);     // in [0, sw) x [0, sh)
        const size_t p = (size_t)sy * a.sw + sx;
        float v[3];
        if (FIRST) {
            pbloom::bright(rule, a.src[3 * p], a.src[3 * p + 1], a.src[3 * p + 2], v);
        } else {
            v[0] = a.src[p]; v[1] = a.src[a.src_stride + p]; v[2] = a.src[2 * a.src_stride + p];
        }
        const uint32_t at = slot * kBloomPitch + col;
        s_src[0][at] = v[0]; s_src[1][at] = v[1]; s_src[2][at] = v[2];
    }
    __syncthreads();
    for (uint32_t j = tid; j < kBloomSrc * kBloomTile; j += kBlock) {
        const uint32_t at = (j / kBloomTile) * kBloomPitch + 2u * (j % kBloomTile);
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) s_h[c][j] = pbloom::reduce4(s_src[c][at], s_src[c][at + 1], s_src[c][at + 2], s_src[c][at + 3]);
    }
    __syncthreads();
    const uint32_t X = X0 + tid % kBloomTile, Y = Y0 + tid / kBloomTile;
    if (X >= a.dw || Y >= a.dh) return;
    const size_t q = (size_t)Y * a.dw + X;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c)
        a.dst[c * a.dst_stride + q] = pbloom::reduce4(s_h[c][tid], s_h[c][kBloomHalf * kBloomTile + tid], s_h[c][kBloomTile + tid],
                                                      s_h[c][(kBloomHalf + 1u) * kBloomTile + tid]);
}

// One workgroup per 32 x 8 destination tile; its 16 x 4 coarse texels and a one-texel halo (18 x 6, clamped at the plane's edges) go
// through LDS.  A half-wave is one destination row: lanes 2 m and 2 m + 1 read the same coarse texel (a broadcast) and neighbours
// that lie 2 apart -- no two lanes of a half on one bank with different addresses.  Every thread reads only its own texel of D_i
// (or its own film pixel) before it writes it: U_i goes over D_i, and out may be the film.
template <bool LAST>
__global__ void __launch_bounds__(kBlock) k_bloom_expand(BloomExpandArgs a) {
    static_assert(kBlock == kBloomExpW * kBloomExpH, "one thread per destination texel");
    __shared__ float s_c[3][kBloomCoarseW * kBloomCoarseH];
    const uint32_t tid = threadIdx.x;
    const uint32_t X0 = (blockIdx.x % a.tiles_x) * kBloomExpW, Y0 = (blockIdx.x / a.tiles_x) * kBloomExpH;
    const uint32_t CX0 = X0 / 2u, CY0 = Y0 / 2u;               // the tile's first coarse texel; the LDS tile starts one before it
    if (tid < kBloomCoarseW * kBloomCoarseH) {
        const uint32_t cx = bloom_clamp1(CX0 + tid % kBloomCoarseW, a.cw), cy = bloom_clamp1(CY0 + tid / kBloomCoarseW, a.ch);
        const size_t p = (size_t)cy * a.cw + cx;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) s_c[c][tid] = a.coarse[c * a.coarse_stride + p];
    }
    __syncthreads();
    const uint32_t X = X0 + tid % kBloomExpW, Y = Y0 + tid / kBloomExpW;
    if (X >= a.w || Y >= a.h) return;
    uint32_t ix, nx, iy, ny;
    pbloom::expand_src(X, a.cw, &ix, &nx);
    pbloom::expand_src(Y, a.ch, &iy, &ny);
    // coarse index g -> LDS column g - CX0 + 1: g lies in [CX0 - 1, CX0 + 16] and inside the plane, where the staging did not clamp
    ix = ix + 1u - CX0; nx = nx + 1u - CX0; iy = (iy + 1u - CY0) * kBloomCoarseW; ny = (ny + 1u - CY0) * kBloomCoarseW;
    const pbloom::Rule rule = bloom_rule(a.r);
    const size_t q = (size_t)Y * a.w + X;
    float up[3];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c)
        up[c] = pbloom::expand2(pbloom::expand2(s_c[c][iy + ix], s_c[c][iy + nx]), pbloom::expand2(s_c[c][ny + ix], s_c[c][ny + nx]));
    if (LAST) {
        const float f[3] = {a.film[3 * q], a.film[3 * q + 1], a.film[3 * q + 2]};
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) a.out[3 * q + c] = pbloom::combine(rule, f[c], up[c]);
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) a.fine[c * a.fine_stride + q] = pbloom::collect(rule, a.fine[c * a.fine_stride + q], up[c]);
    }
}

// One workgroup for every level from the first of at most 32 x 32 texels on: their planes live in LDS back to back (fewer than
// pbloom::kTailTexels texels per channel), reduced down and collected back up with the functions the host runs (pbloom::reduce_at,
// expand_at), so the bits are those of the per-level kernels.  The loops over the levels are unrolled: a.w[l], a.h[l] are read at
// fixed offsets of the argument block.
__global__ void __launch_bounds__(kBloomTailBlock) k_bloom_tail(BloomTailArgs a) {
    __shared__ float s_l[3][pbloom::kTailTexels];
    const uint32_t tid = threadIdx.x;
    const pbloom::Rule rule = bloom_rule(a.r);
    const uint32_t n0 = a.w[0] * a.h[0];
    if (a.src) {
        for (uint32_t t = tid; t < n0; t += kBloomTailBlock) {
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                const float* plane = a.src + c * a.src_stride;
                const uint32_t sw = a.sw;
                s_l[c][t] = pbloom::reduce_at([plane, sw](uint32_t x, uint32_t y) { return plane[(size_t)y * sw + x]; }, a.sw, a.sh, t % a.w[0], t / a.w[0]);
            }
        }
    } else {
        for (uint32_t t = tid; t < n0; t += kBloomTailBlock) {
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) s_l[c][t] = a.dst[c * a.dst_stride + t];
        }
    }
    __syncthreads();
    uint32_t off = 0u;                                         // the first texel of level l - 1
#pragma unroll
    for (uint32_t l = 1; l < pbloom::kMaxLevels; ++l) {
        if (l < a.n) {                                         // (uniform: every thread takes every barrier)
            const uint32_t pw = a.w[l - 1], ph = a.h[l - 1], w = a.w[l], h = a.h[l], to = off + pw * ph;
            for (uint32_t t = tid; t < w * h; t += kBloomTailBlock) {
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) {
                    const float* plane = &s_l[c][off];
                    s_l[c][to + t] = pbloom::reduce_at([plane, pw](uint32_t x, uint32_t y) { return plane[y * pw + x]; }, pw, ph, t % w, t / w);
                }
            }
            off = to;
            __syncthreads();
        }
    }
    // off = the first texel of level n - 1, which is U_(n-1) as it stands
#pragma unroll
    for (uint32_t l = pbloom::kMaxLevels - 1u; l-- > 0u;) {
        if (l + 1u < a.n) {
            const uint32_t w = a.w[l], h = a.h[l], cw = a.w[l + 1], ch = a.h[l + 1], to = off - w * h;
            for (uint32_t t = tid; t < w * h; t += kBloomTailBlock) {
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) {
                    const float* plane = &s_l[c][off];
                    const float up = pbloom::expand_at([plane, cw](uint32_t x, uint32_t y) { return plane[y * cw + x]; }, cw, ch, t % w, t / w);
                    s_l[c][to + t] = pbloom::collect(rule, s_l[c][to + t], up);
                }
            }
            off = to;
            __syncthreads();
        }
    }
    for (uint32_t t = tid; t < n0; t += kBloomTailBlock) {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) a.dst[c * a.dst_stride + t] = s_l[c][t];
    }
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_bloom_reduce(const BloomReduceArgs& a, uint32_t tiles, hipStream_t st) {
    if (a.first) hipLaunchKernelGGL(PTK_IMPL::k_bloom_reduce<true>, dim3(tiles), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(PTK_IMPL::k_bloom_reduce<false>, dim3(tiles), dim3(kBlock), 0, st, a);
}
void launch_bloom_expand(const BloomExpandArgs& a, uint32_t tiles, hipStream_t st) {
    if (a.last) hipLaunchKernelGGL(PTK_IMPL::k_bloom_expand<true>, dim3(tiles), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(PTK_IMPL::k_bloom_expand<false>, dim3(tiles), dim3(kBlock), 0, st, a);
}
void launch_bloom_tail(const BloomTailArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(PTK_IMPL::k_bloom_tail, dim3(1), dim3(PTK_IMPL::kBloomTailBlock), 0, st, a);
}
}  // namespace ptk
