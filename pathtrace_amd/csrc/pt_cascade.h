// pt_cascade.h -- the rule of the brightness cascade (pt_render_cascade_device), written once for the kernels
// (pt_film_cascade.h) and for the host (pt_cascade.cpp, the CPU tests).  A firefly-robust film after Zirr, Hanika and
// Dachsbacher, "Re-weighting firefly samples for improved finite-sample Monte Carlo estimates" (2018): every sample is split
// between two layers of a per-pixel cascade by its luminance, and a layer keeps its energy in full only where enough samples
// of that brightness landed in the pixel or its 3 x 3 neighbourhood.
//
// Everything is f64 and uses only + - * /, comparisons and selects; build with -ffp-contract=off so that no compiler fuses a
// multiply into an add.  No pow, exp or log: the host forms the levels by repeated multiplication (levels()) and hands the table
// to the kernels, so host and device are bit-identical.
//
//   levels     B_0 = (double)start, B_{j+1} = B_j * (double)base, K = layers of them
//   split      a sample v = (r, g, b) (f32) with L = ptad::luminance(r, g, b):  j = the largest index in [0, K-2] with B_j <= L
//              (none -- L below B_0, or NaN --: j = 0);
//                !(L > B_j)         w_lo = 1, w_hi = 0                       (NaN, negatives, L <= B_0)
//                L < B_{j+1}        q = B_j / B_{j+1},  w_lo = (B_j / L - q) / (1 - q),  w_hi = 1 - w_lo
//                otherwise          w_lo = 0, w_hi = 1                       (L >= B_{K-1}, +inf)
//              S_j += w_lo * (double)v.c and S_{j+1} += w_hi * (double)v.c per channel, each ONLY when its weight is not exactly 0
//              (a select: an infinite sample puts no NaN into the lower layer); beside them the plain sums P += (double)v.c.
//              Samples in sample order.
//   count      lum_j = 0.2126 S_j.r + 0.7152 S_j.g + 0.0722 S_j.b;  T_j = lum_{j-1} + lum_j + lum_{j+1} added left to right, an
//              absent layer 0.0;  cnt_j = T_j / B_j
//   re-weight  wide_j(p) = the sum of cnt_j over the in-image taps of the 3 x 3 block around p, row-major, divided by their number;
//              r = cnt_j(p) > wide_j(p) ? cnt_j(p) : wide_j(p)  (NaN when either is: the block holds p);
//              w_j = 1 when j = 0, kappa = 0, r is NaN or r >= kappa, else r / kappa
//   film       m.c = (sum over j ascending, from 0.0, of w_j * S_j.c) / n in f64; the linear plane is (float)m.c, the RGBA8 plane m.c
//              through the sqrt, clamp and `as u8` steps of every render (k_resolve: they start from the f64 mean); plain = P / n
//
// Out of scope: lens, adaptive, progressive and multi-GPU forms, and feeding the layers to the denoiser -- the cascade film is an
// ordinary linear film and can be handed to pt_denoise_device as it is.
#pragma once
#include <stdint.h>
#include <cstring>
#include <vector>

#include "pt_adaptive.h"

#if defined(__clang__)
#define PT_CAS_UNROLL _Pragma("unroll")
#else
#define PT_CAS_UNROLL
#endif

namespace ptcas {

constexpr uint32_t kMinLayers = 2, kMaxLayers = 8;

struct Levels {
    double B[kMaxLayers];     // B[k] for k < K; the rest unused
    double kappa;
    uint32_t K;
};

PT_AD_HD bool finite(double v) { return v - v == 0.0; }

// The level table; false when a parameter is out of range or a level is not finite.
PT_AD_HD bool levels(uint32_t layers, float start, float base, float kappa, Levels* out) {
    if (layers < kMinLayers || layers > kMaxLayers) return false;
    const double s = (double)start, b = (double)base, k = (double)kappa;
    if (!finite(s) || !(s > 0.0) || !finite(b) || !(b >= 2.0) || !finite(k) || !(k >= 0.0)) return false;
    out->K = layers; out->kappa = k;
    double v = s;
    for (uint32_t j = 0; j < kMaxLayers; ++j) {
        out->B[j] = j < layers ? v : 0.0;
        if (j < layers && !finite(v)) return false;
        v = v * b;
    }
    return true;
}

// split: the lower layer j and the two weights of a luminance
PT_AD_HD void split(const Levels& lv, double L, uint32_t* j_out, double* w_lo, double* w_hi) {
    uint32_t j = 0;
    double bj = lv.B[0], bn = lv.B[1];         // (the table is indexed by constants only: it stays in registers on the device)
    PT_CAS_UNROLL
    for (uint32_t k = 1; k + 1 < kMaxLayers; ++k)
        if (k + 1 < lv.K && lv.B[k] <= L) { j = k; bj = lv.B[k]; bn = lv.B[k + 1]; }
    double lo, hi;
    if (!(L > bj)) { lo = 1.0; hi = 0.0; }
    else if (L < bn) {
        const double q = bj / bn;
        lo = (bj / L - q) / (1.0 - q);
        hi = 1.0 - lo;
    } else { lo = 0.0; hi = 1.0; }
    *j_out = j; *w_lo = lo; *w_hi = hi;
}

// split + accumulate for a thread or a host loop that holds the sums as S[layer][channel] and P[channel]; `K` layers are
// touched by compile-time index only (the kernels keep them in registers)
template <uint32_t K>
PT_AD_HD void add_sample(const Levels& lv, float r, float g, float b, double (&S)[K][3], double (&P)[3]) {
    const double v[3] = {(double)r, (double)g, (double)b};
    uint32_t j;
    double lo, hi;
    split(lv, ptad::luminance(r, g, b), &j, &lo, &hi);
    for (uint32_t c = 0; c < 3; ++c) P[c] += v[c];
    PT_CAS_UNROLL
    for (uint32_t k = 0; k < K; ++k) {
        const double w = k == j ? lo : (k == j + 1u ? hi : 0.0);
        for (uint32_t c = 0; c < 3; ++c) {
            const double t = S[k][c] + w * v[c];
            S[k][c] = w != 0.0 ? t : S[k][c];
        }
    }
}

PT_AD_HD double layer_luminance(double r, double g, double b) { return 0.2126 * r + 0.7152 * g + 0.0722 * b; }

// count: cnt_j from the luminances of the pixel's layers
PT_AD_HD double count(const Levels& lv, const double* lum, uint32_t j) {
    double t = (j > 0u ? lum[j - 1u] : 0.0) + lum[j];
    t = t + (j + 1u < lv.K ? lum[j + 1u] : 0.0);
    return t / lv.B[j];
}

// re-weight: w_j from the pixel's own count and the mean count of its block
PT_AD_HD double weight(const Levels& lv, uint32_t j, double cnt, double wide) {
    const double r = cnt > wide ? cnt : wide;
    if (j == 0u || lv.kappa == 0.0 || r != r || r >= lv.kappa) return 1.0;
    return r / lv.kappa;
}

// the RGBA8 byte of a channel's f64 mean: the statements of k_resolve (world.rs:322-331)
PT_AD_HD uint32_t byte8(double m) {
    const double gm = __builtin_sqrt(m);
    const double cl = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);        // clamp keeps NaN
    const double q = cl * 255.0;
    return (uint32_t)((q != q) ? (uint8_t)0 : (uint8_t)q);           // `as u8`: truncation, NaN -> 0
}

// The whole rule on host planes (pt_cascade_host): samples n * np RGB floats, [s * np + p]; out_linear np * 3 floats; out_rgba
// np * 4 bytes, out_plain np * 3 floats, out_layers K * np * 3 doubles and out_weights K * np floats may be null.
inline void host_film(const Levels& lv, uint32_t width, uint32_t height, uint32_t n, const float* samples, float* out_linear,
                      uint8_t* out_rgba, float* out_plain, double* out_layers, float* out_weights) {
    const size_t np = (size_t)width * height;
    const uint32_t K = lv.K;
    std::vector<double> own_layers, plain(3 * np), cnt((size_t)K * np);
    if (!out_layers) { own_layers.resize((size_t)K * np * 3); out_layers = own_layers.data(); }
    for (size_t p = 0; p < np; ++p) {
        double S[kMaxLayers][3] = {}, P[3] = {0.0, 0.0, 0.0}, lum[kMaxLayers];
        for (uint32_t s = 0; s < n; ++s) {
            const float* v = samples + ((size_t)s * np + p) * 3;
            add_sample<kMaxLayers>(lv, v[0], v[1], v[2], S, P);
        }
        for (uint32_t k = 0; k < K; ++k) {
            for (uint32_t ch = 0; ch < 3; ++ch) out_layers[((size_t)k * np + p) * 3 + ch] = S[k][ch];
            lum[k] = layer_luminance(S[k][0], S[k][1], S[k][2]);
        }
        for (uint32_t k = 0; k < K; ++k) cnt[(size_t)k * np + p] = count(lv, lum, k);
        for (uint32_t ch = 0; ch < 3; ++ch) plain[3 * p + ch] = P[ch];
    }
    const double dn = (double)n;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            double acc[3] = {0.0, 0.0, 0.0};
            for (uint32_t j = 0; j < K; ++j) {
                double sum = 0.0;
                uint32_t taps = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int gx = (int)x + dx, gy = (int)y + dy;
                        if (gx >= 0 && gy >= 0 && gx < (int)width && gy < (int)height) { sum += cnt[(size_t)j * np + (size_t)gy * width + gx]; ++taps; }
                    }
                const double w = weight(lv, j, cnt[(size_t)j * np + p], sum / (double)taps);
                if (out_weights) out_weights[(size_t)j * np + p] = (float)w;
                for (uint32_t ch = 0; ch < 3; ++ch) acc[ch] += w * out_layers[((size_t)j * np + p) * 3 + ch];
            }
            uint32_t q8 = 0xFF000000u;
            for (uint32_t ch = 0; ch < 3; ++ch) {
                const double m = acc[ch] / dn;
                out_linear[3 * p + ch] = (float)m;
                q8 |= byte8(m) << (8 * ch);
                if (out_plain) out_plain[3 * p + ch] = (float)(plain[3 * p + ch] / dn);
            }
            if (out_rgba) std::memcpy(out_rgba + 4 * p, &q8, 4);
        }
}

}  // namespace ptcas
