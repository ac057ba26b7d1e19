// pt_bloom.h -- the bloom stage of the display chain (pt_bloom_device), written once for the kernels (k_bloom_reduce,
// k_bloom_expand, k_bloom_tail in pt_film_bloom.h) and the host (pt_bloom_host in pt_bloom.cpp).  Build with -ffp-contract=off, like
// pt_tonemap.h.  Every plane and every operation is f32: + - * /, comparisons and selects; no libm.
//
// Film c of W x H pixels (3 floats each), parameters PtBloom {levels, threshold T, knee k, clamp, scatter s, intensity}.
// 1. Plan.  Level 0 is ceil(W/2) x ceil(H/2), level i is ceil(w_(i-1)/2) x ceil(h_(i-1)/2); level i >= 1 exists while i < levels and
//    max(w_(i-1), h_(i-1)) > 1.  n = the number of levels.  The TAIL starts at the first level with w <= 32 and h <= 32 (n when there
//    is none): one workgroup holds it and everything below it in LDS.  The plan depends on (W, H, levels) alone.
// 2. Bright pass of a pixel: L = ptone::lum(c).  L or a channel NaN or +-inf, or L <= 0: b = 0.  Else d = L - T, q = min(max(d + k, 0),
//    2 k), soft = k > 0 ? (q q) / (4 k) : 0, g = min(max(max(soft, d), 0), clamp), b_ch = max(c_ch, 0) (g / L).  min and max are
//    selects (a < b ? a : b, a > b ? a : b).
// 3. Reduce (the film under the bright pass -> level 0; level i -> level i + 1), separable, the horizontal pass first:
//    r(a, b, c, d) = ((0.125 a + 0.375 b) + 0.375 c) + 0.125 d on the source indices 2 x - 1 .. 2 x + 2, clamped to [0, w - 1].
// 4. Expand, up(P), to the next finer size or to the film, separable, the horizontal pass first: destination index j takes the source
//    i = min(j >> 1, w_c - 1) and its neighbour i - 1 (j even) or i + 1 (j odd), clamped: e(p, q) = 0.75 p + 0.25 q.  By the plan
//    j >> 1 <= w_c - 1 always (w_c = ceil(w / 2)).
// 5. Collect: U_(n-1) = D_(n-1);  U_i = (1 - s) D_i + s up(U_(i+1)), 1 - s rounded once, the two products rounded, then the sum.
// 6. Combine: a = intensity up(U_0);  out_ch = a_ch == 0 ? c_ch : c_ch + a_ch.
// A pass keeps f32 values between its halves, so running the horizontal pass of the rows a texel needs in registers gives the bits a
// stored intermediate plane gives.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_tonemap.h"

namespace pbloom {

constexpr uint32_t kMaxLevels = 8;
constexpr uint32_t kTailSide = 32;                 // the tail starts at the first level of at most kTailSide x kTailSide texels
constexpr uint32_t kTailTexels = 2048;             // ... and its levels together hold fewer texels than this (32 x 32 + 16 x 16 + ..)

struct Rule {                 // PtBloom as the passes take it
    float T, k, clamp, s, oms, intensity;          // oms = 1 - s
};
PT_AD_HD Rule rule(float T, float k, float clamp, float s, float intensity) {
    Rule r;
    r.T = T; r.k = k; r.clamp = clamp; r.s = s; r.oms = 1.0f - s; r.intensity = intensity;
    return r;
}

// rule 1.  off: the first float of a level in the pyramid buffer; a level is three planes of `stride` floats (R, G, B), stride a
// multiple of 4: every plane starts 16-byte aligned.
struct Plan {
    uint32_t n, first_tail;
    uint32_t w[kMaxLevels], h[kMaxLevels];
    size_t off[kMaxLevels], stride[kMaxLevels], total;
};
PT_AD_HD uint32_t half_up(uint32_t v) { return v / 2u + (v & 1u); }
PT_AD_HD Plan plan(uint32_t W, uint32_t H, uint32_t levels) {
    Plan p;
    p.n = 0; p.total = 0;
    uint32_t w = W, h = H;
    for (uint32_t i = 0; i < kMaxLevels; ++i) {
        p.w[i] = p.h[i] = 0u; p.off[i] = p.stride[i] = 0;
        if (i >= levels || (i >= 1u && w <= 1u && h <= 1u)) continue;
        w = half_up(w); h = half_up(h);
        p.w[i] = w; p.h[i] = h;
        p.stride[i] = (((size_t)w * h + 3u) / 4u) * 4u;
        p.off[i] = p.total;
        p.total += 3u * p.stride[i];
        p.n = i + 1u;
    }
    p.first_tail = p.n;
    for (uint32_t i = p.n; i-- > 0u;)
        if (p.w[i] <= kTailSide && p.h[i] <= kTailSide) p.first_tail = i;
    return p;
}

PT_AD_HD bool finite(float v) { return v - v == 0.0f; }       // false for NaN and +-inf
PT_AD_HD float fmin_sel(float a, float b) { return a < b ? a : b; }
PT_AD_HD float fmax_sel(float a, float b) { return a > b ? a : b; }

// rule 2
PT_AD_HD void bright(const Rule& r, float c0, float c1, float c2, float* b) {
    const float L = ptone::lum(c0, c1, c2);
    b[0] = b[1] = b[2] = 0.0f;
    if (!(finite(L) && finite(c0) && finite(c1) && finite(c2) && L > 0.0f)) return;
    const float d = L - r.T;
    const float q = fmin_sel(fmax_sel(d + r.k, 0.0f), 2.0f * r.k);
    const float soft = r.k > 0.0f ? (q * q) / (4.0f * r.k) : 0.0f;
    const float g = fmin_sel(fmax_sel(fmax_sel(soft, d), 0.0f), r.clamp);
    const float f = g / L;
    b[0] = fmax_sel(c0, 0.0f) * f;
    b[1] = fmax_sel(c1, 0.0f) * f;
    b[2] = fmax_sel(c2, 0.0f) * f;
}

// rules 3 to 6: the arithmetic of one tap row, one collect, one combine
PT_AD_HD float reduce4(float a, float b, float c, float d) { return 0.125f * a + 0.375f * b + 0.375f * c + 0.125f * d; }
PT_AD_HD float expand2(float p, float q) { return 0.75f * p + 0.25f * q; }
PT_AD_HD float collect(const Rule& r, float d, float up) { return r.oms * d + r.s * up; }
PT_AD_HD float combine(const Rule& r, float c, float up) {
    const float a = r.intensity * up;
    return a == 0.0f ? c : c + a;
}

// the clamped source index of tap k (0 .. 3) of destination x of a reduce over a plane of width w
PT_AD_HD uint32_t reduce_src(uint32_t x, uint32_t k, uint32_t w) {
    const uint32_t i = 2u * x + k;                 // 2 x - 1 + k, shifted by one
    return i == 0u ? 0u : (i - 1u < w ? i - 1u : w - 1u);
}
// the two source indices of destination j of an expand from a plane of width wc
PT_AD_HD void expand_src(uint32_t j, uint32_t wc, uint32_t* i, uint32_t* nb) {
    const uint32_t last = wc - 1u;
    const uint32_t c = (j >> 1) < last ? (j >> 1) : last;
    *i = c;
    *nb = (j & 1u) ? (c < last ? c + 1u : last) : (c > 0u ? c - 1u : 0u);
}

// One texel of a reduce / an expand of a plane read through `at(x, y)`: the form the host and k_bloom_tail run, and the one the tiled
// kernels restate over their LDS tiles with the same reduce4 / expand2 calls.
template <class At> PT_AD_HD float reduce_at(const At& at, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
    float row[4];
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t sy = reduce_src(y, j, h);
        row[j] = reduce4(at(reduce_src(x, 0u, w), sy), at(reduce_src(x, 1u, w), sy), at(reduce_src(x, 2u, w), sy), at(reduce_src(x, 3u, w), sy));
    }
    return reduce4(row[0], row[1], row[2], row[3]);
}
template <class At> PT_AD_HD float expand_at(const At& at, uint32_t wc, uint32_t hc, uint32_t x, uint32_t y) {
    uint32_t ix, nx, iy, ny;
    expand_src(x, wc, &ix, &nx);
    expand_src(y, hc, &iy, &ny);
    return expand2(expand2(at(ix, iy), at(nx, iy)), expand2(at(ix, ny), at(nx, ny)));
}

}  // namespace pbloom
