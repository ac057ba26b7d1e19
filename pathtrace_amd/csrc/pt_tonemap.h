// pt_tonemap.h -- the display transform of pt_tonemap_device, written once for the kernels (k_film_histogram,
// k_exposure_meter, k_tonemap in pt_film_tonemap.h), the host (pt_tonemap.cpp) and the host compilers of the CPU tests
// (tests/test_tonemap_cpu.py).  Build with -ffp-contract=off, like pt_adaptive.h: no compiler fuses what the rule writes apart.
//
// Image W x H, c the linear film (3 floats per pixel).
//   L(c) = (0.2126f r + 0.7152f g) + 0.0722f b in f32, three products and two sums, left to right (the a-trous kernels' dn_lum).
//
// 1. Histogram, 258 uint32 words: [0, 256) the bins, [256] dark, [257] invalid.  With b = bits(L) as uint32:
//      invalid   L is NaN or +-inf                     (b & 0x7F800000) == 0x7F800000
//      dark      L < 2^-16: 0, negatives, denormals    sign bit set, or b < bits(2^-16) = 0x37800000
//      bin       min((b >> 20) - (0x37800000 >> 20), 255): 8 bins per octave over [2^-16, 2^16), L >= 2^16 in bin 255
//    Integer arithmetic alone; the words add up to W H.
// 2. Metering, f64.  N = the sum of the 256 bins, lo = pct_lo N, hi = pct_hi N (pct widened to f64 first).  Bin k holds the
//    ranks [B_k, B_k + n_k) with B_k the sum of the bins before it; its part inside the window is
//      in_k = max(0, min(B_k + n_k, hi) - max(B_k, lo))                                     (a real number)
//    and its centre, in log2 units, z_k = -16 + (k + 0.5) / 8.  m = sum in_k z_k / sum in_k.  A window without width (pct_lo ==
//    pct_hi, sum in_k == 0): m = z_k of the first bin with n_k > 0 and B_k + n_k >= lo.
//    The sums are formed as the metering wave forms them: lane i of 64 adds its bins 4 i .. 4 i + 3 in ascending order, then
//    six butterfly steps v_i += v_(i xor s), s = 32, 16, .., 1.  meter() below is that order on the host.
//    Target: t = clamp(log2(key) - m, log2_min, log2_max).  N == 0 (a black frame): t = the previous exposure, 0 when there is none.
// 3. Adaptation.  The state: log2E (f64), E (f32), valid, and the image size of the frame that wrote it.  A frame is FRESH when
//    the state is not valid or its size differs.  log2E = t when fresh, else log2E + adapt (t - log2E).  E = (float)exp2(log2E).
// 4. Manual mode: E = (float)exp2((double)ev); no histogram, the state untouched.
// 5. Curve, f32, per pixel, x = E c per channel:
//      clamp      y = x
//      Reinhard   Lx = L(x);  y = x (1 + Lx / white^2) / (1 + Lx)
//      ACES       x' = min(x, 2^60) (the quotient has long reached its limit there, and x'^2 stays finite);
//                 y = x' (2.51 x' + 0.03) / (x' (2.43 x' + 0.59) + 0.14)
//    A channel whose y is NaN -- a NaN in the film, inf / inf in a curve -- is 0 on both planes.
// 6. Transfer, y -> u8:
//      sqrt       g = sqrt((double)y), clamp to [0, 1] keeping NaN, q = 255 g, `as u8` (truncation, NaN -> 0): the steps of k_resolve
//      sRGB       g = 0 for y <= 0, 1 for y >= 1, 12.92 y for y <= 0.0031308, else 1.055 exp2(log2(y) / 2.4) - 0.055, in f32;
//                 then the same clamp, q = 255 g in f64 and `as u8`
//    Alpha is 255.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pt_adaptive.h"

namespace ptone {

constexpr uint32_t kBins = 256, kDark = 256, kInvalid = 257, kWords = 258;
constexpr uint32_t kFirstBits = 0x37800000u;       // bits(2^-16)
constexpr unsigned kLanes = 64, kBinsPerLane = kBins / kLanes;

// mode / curve / transfer of PtTonemap (include/pathtrace_amd.h)
constexpr uint32_t kAuto = 0, kManual = 1, kCurveClamp = 0, kCurveReinhard = 1, kCurveAces = 2, kTransferSqrt = 0, kTransferSrgb = 1;

PT_AD_HD float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

PT_AD_HD uint32_t float_bits(float v) {
    union { float f; uint32_t u; } w;
    w.f = v;
    return w.u;
}

// rule 1: the histogram word of a pixel of luminance L
PT_AD_HD uint32_t word(float L) {
    const uint32_t b = float_bits(L);
    if ((b & 0x7F800000u) == 0x7F800000u) return kInvalid;
    if ((b >> 31) != 0u || b < kFirstBits) return kDark;
    const uint32_t k = (b >> 20) - (kFirstBits >> 20);
    return k < kBins - 1u ? k : kBins - 1u;
}

PT_AD_HD double centre(uint32_t k) { return -16.0 + ((double)k + 0.5) / 8.0; }

// rule 2, one lane's part: its kBinsPerLane bins from `first`, `before` = the sum of the bins before them.  Adds to s
// (sum in_k z_k) and w (sum in_k); *point = the lane's first bin with n_k > 0 and B_k + n_k >= lo, kBins when it has none.
PT_AD_HD void meter_lane(const uint32_t* n, uint32_t first, uint64_t before, double lo, double hi, double* s, double* w, uint32_t* point) {
    double ls = 0.0, lw = 0.0;
    uint32_t pt = kBins;
    for (unsigned j = 0; j < kBinsPerLane; ++j) {
        const double b0 = (double)before, b1 = (double)(before + n[j]);
        const double top = b1 < hi ? b1 : hi, bot = b0 > lo ? b0 : lo;
        const double in = top - bot > 0.0 ? top - bot : 0.0;
        ls += in * centre(first + j);
        lw += in;
        if (pt == kBins && n[j] > 0u && b1 >= lo) pt = first + j;
        before += n[j];
    }
    *s = ls; *w = lw; *point = pt;
}

// rules 2 and 3 from the reduced sums: the new log2E.  total = N, point = the least of the lanes' points.
PT_AD_HD double adapt(uint64_t total, double s, double w, uint32_t point, float key, float log2_min, float log2_max, float adapt_rate,
                      bool fresh, double log2E_prev) {
    double t = fresh ? 0.0 : log2E_prev;
    if (total > 0u) {
        const double m = w > 0.0 ? s / w : centre(point < kBins ? point : kBins - 1u);
        t = ::log2((double)key) - m;
        t = t < (double)log2_min ? (double)log2_min : t;
        t = t > (double)log2_max ? (double)log2_max : t;
    }
    return fresh ? t : log2E_prev + (double)adapt_rate * (t - log2E_prev);
}

PT_AD_HD float exposure(double log2E) { return (float)::exp2(log2E); }

// rule 5: y of the three channels of c under exposure E
PT_AD_HD void curve(uint32_t which, float E, float white, const float* c, float* y) {
    const float x[3] = {E * c[0], E * c[1], E * c[2]};
    if (which == kCurveReinhard) {
        const float Lx = lum(x[0], x[1], x[2]);
        const float num = 1.0f + Lx / (white * white), den = 1.0f + Lx;
        for (int k = 0; k < 3; ++k) y[k] = x[k] * num / den;
    } else if (which == kCurveAces) {
        for (int k = 0; k < 3; ++k) {
            const float v = x[k] < 1152921504606846976.0f ? x[k] : (x[k] != x[k] ? x[k] : 1152921504606846976.0f);   // min(x, 2^60), NaN kept
            y[k] = v * (2.51f * v + 0.03f) / (v * (2.43f * v + 0.59f) + 0.14f);
        }
    } else {
        for (int k = 0; k < 3; ++k) y[k] = x[k];
    }
    for (int k = 0; k < 3; ++k) y[k] = y[k] != y[k] ? 0.0f : y[k];
}

// rule 6: clamp keeping NaN, 255 g, `as u8` -- the statements of k_resolve behind its sqrt (world.rs:324-331)
PT_AD_HD uint32_t unorm8(double g) {
    const double cl = g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g);
    const double q = cl * 255.0;
    return (q != q) ? 0u : (uint32_t)(uint8_t)q;
}
PT_AD_HD uint32_t transfer_sqrt(float y) { return unorm8(__builtin_sqrt((double)y)); }
PT_AD_HD uint32_t transfer_srgb(float y) {
    float g;
    if (!(y > 0.0f)) g = 0.0f;
    else if (y >= 1.0f) g = 1.0f;
    else if (y <= 0.0031308f) g = 12.92f * y;
    else g = 1.055f * ::exp2f(::log2f(y) / 2.4f) - 0.055f;
    return unorm8((double)g);
}
PT_AD_HD uint32_t rgba8(uint32_t transfer, const float* y) {
    uint32_t q8 = 0xFF000000u;
    for (int k = 0; k < 3; ++k) q8 |= (transfer == kTransferSrgb ? transfer_srgb(y[k]) : transfer_sqrt(y[k])) << (8 * k);
    return q8;
}

// The metering wave on the host: 64 lanes' parts, the butterfly sums, adapt().  hist: the 258 words.
inline double meter(const uint32_t* hist, float pct_lo, float pct_hi, float key, float log2_min, float log2_max, float adapt_rate, bool fresh,
                    double log2E_prev) {
    uint64_t before[kLanes], total = 0;
    for (unsigned i = 0; i < kLanes; ++i) {
        before[i] = total;
        for (unsigned j = 0; j < kBinsPerLane; ++j) total += hist[kBinsPerLane * i + j];
    }
    const double lo = (double)pct_lo * (double)total, hi = (double)pct_hi * (double)total;
    double s[kLanes], w[kLanes];
    uint32_t point = kBins;
    for (unsigned i = 0; i < kLanes; ++i) {
        uint32_t pt;
        meter_lane(hist + kBinsPerLane * i, kBinsPerLane * i, before[i], lo, hi, &s[i], &w[i], &pt);
        point = pt < point ? pt : point;
    }
    for (unsigned step = kLanes / 2; step > 0; step >>= 1) {
        double s2[kLanes], w2[kLanes];
        for (unsigned i = 0; i < kLanes; ++i) { s2[i] = s[i] + s[i ^ step]; w2[i] = w[i] + w[i ^ step]; }
        for (unsigned i = 0; i < kLanes; ++i) { s[i] = s2[i]; w[i] = w2[i]; }
    }
    return adapt(total, s[0], w[0], point, key, log2_min, log2_max, adapt_rate, fresh, log2E_prev);
}

}  // namespace ptone
