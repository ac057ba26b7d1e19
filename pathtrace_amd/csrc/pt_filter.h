// pt_filter.h -- the rule of the film's reconstruction filters (pt_render_filtered_device), written once for the
// kernel (pt_film_filter.h) and for the host (pt_filter.cpp, the CPU tests).  Every render resolves the film as the plain mean
// of the samples that started inside a pixel -- a box filter of radius 0.5; here a pixel takes the samples of its neighbours
// too, each weighted by a separable filter of the distance between the sample's position on the film and the pixel's centre.
// No path kernel stores that position: it is recomputed from the Philox block the camera ray drew its jitter from.
//
// Everything is f64 and uses only + - * /, comparisons and selects; build with -ffp-contract=off so that no compiler fuses a
// multiply into an add.  No libm: exp_neg below is + and * only.  Host and device are bit-identical.
//
//   jitter     sample s of image pixel (x, y) (y = film row, top-down; s counts from spp_offset): w = the Philox4x32-7 block of
//              ctr (x, y, s, 0xFFFFFFFF), key (0, 0) -- camera_ray's --;  ox = (2 (w0 >> 9) + 1) / 2^24, oy the same of w1
//   position   in pixel-pitch units the sample lies at (x + ox, y - oy) (camera_ray flips y: a larger oy moves the sample up);
//              the centre of pixel q is (qx + 0.5, qy - 0.5)
//   offsets    a sample of pixel p seen from output pixel q:  tx = (px - qx) + (ox - 0.5),  ty = (py - qy) - (oy - 0.5)  (exact)
//   weight     w = f(|tx|) * f(|ty|).  R = (double)radius.  f(t) = 0 for t >= R; for t < R
//                box        1
//                tent       1 - t / R
//                gaussian   exp_neg(alpha * (t * t)) - gR,  gR = exp_neg(alpha * (R * R)),  alpha = (double)a
//                mitchell   B = (double)a, C = (double)b, z = (2 t) / R;
//                             z < 1:  h = a3 z + a2;  h = h z;  h = h z;  h = h + a0;  f = h / 6
//                                     a3 = (12 - 9 B) - 6 C,  a2 = (-18 + 12 B) + 6 C,  a0 = 6 - 2 B
//                             z < 2:  h = b3 z + b2;  h = h z + b1;  h = h z + b0;  f = h / 6
//                                     b3 = (-B) - 6 C,  b2 = 6 B + 30 C,  b1 = (-12 B) - 48 C,  b0 = 8 B + 24 C
//                             else 0 (2 t / R may round up to 2)
//   exp_neg    e in [0, 100] -> exp(-e):  x = e * 2^-8;  p = c_15;  p = p x + c_i for i = 14 .. 0, c_i = (-1)^i (1 / i!) (the
//              quotient of the two exactly representable integers, rounded once);  then p = p p eight times
//   taps       m = the largest integer < R + 0.5 (0 for R = 0.5, 1 up to 1.5, 2 up to 2.5); q takes the samples of the in-image
//              pixels p with |px - qx| <= m and |py - qy| <= m
//   sums       per output pixel and channel A_c += w * (double)v_c (the product rounded, then added), Wt += w, each tap ONLY
//              when w is not exactly 0 (a select: an infinite sample outside the support puts no NaN in); beside them the plain
//              sums P_c += (double)v_c of the pixel's own samples, exactly as the ordinary resolve forms them.  Samples
//              ascending; inside a sample py - qy ascending, then px - qx ascending.  The sums carry over sample batches.
//   film       Wt > 0 (false for NaN): m_c = A_c / Wt, else m_c = P_c / n.  The linear plane is (float)m_c -- under Mitchell it
//              MAY BE NEGATIVE (the filter has negative lobes) and is kept as it is; the RGBA8 plane is m_c through the sqrt,
//              clamp and `as u8` steps of every render (a negative mean gives NaN gives 0); plain = P / n
//
// Box with R = 0.5 has m = 0, w = 1 and Wt = n exactly: the filtered film is pt_render_device's bit for bit.
// No filtered form: row bands, lens, adaptive, progressive and multi-GPU renders, and the brightness cascade with a filter.
#pragma once
#include <stdint.h>
#include <cstring>
#include <vector>

#include "pt_adaptive.h"      // PT_AD_HD
#include "pt_cascade.h"       // ptcas::byte8: the RGBA8 statements of every render

#if defined(__clang__)
#define PT_FLT_UNROLL _Pragma("unroll")
#else
#define PT_FLT_UNROLL
#endif

namespace ptflt {

enum : uint32_t { kBox = 0, kTent = 1, kGaussian = 2, kMitchell = 3, kKinds = 4 };
constexpr uint32_t kMaxM = 2;
constexpr int kPhiloxRounds = 7;              // the ABI's (pt_device.h)
constexpr uint32_t kDepthCamera = 0xFFFFFFFFu;

// What the host makes of a PtFilter once (rule()) and the kernel receives: nothing here is evaluated per sample.
struct Rule {
    uint32_t kind, m;
    double R;
    double alpha, gR;                         // gaussian
    double a3, a2, a0, b3, b2, b1, b0;        // mitchell
};

PT_AD_HD bool finite(double v) { return v - v == 0.0; }

// exp(-e) for e in [0, 100]: + and * only
PT_AD_HD double exp_neg(double e) {
    const double x = e * (1.0 / 256.0);
    double p = -(1.0 / 1307674368000.0);
    p = p * x; p = p + (1.0 / 87178291200.0);
    p = p * x; p = p + -(1.0 / 6227020800.0);
    p = p * x; p = p + (1.0 / 479001600.0);
    p = p * x; p = p + -(1.0 / 39916800.0);
    p = p * x; p = p + (1.0 / 3628800.0);
    p = p * x; p = p + -(1.0 / 362880.0);
    p = p * x; p = p + (1.0 / 40320.0);
    p = p * x; p = p + -(1.0 / 5040.0);
    p = p * x; p = p + (1.0 / 720.0);
    p = p * x; p = p + -(1.0 / 120.0);
    p = p * x; p = p + (1.0 / 24.0);
    p = p * x; p = p + -(1.0 / 6.0);
    p = p * x; p = p + (1.0 / 2.0);
    p = p * x; p = p + -1.0;
    p = p * x; p = p + 1.0;
    p = p * p; p = p * p; p = p * p; p = p * p;
    p = p * p; p = p * p; p = p * p; p = p * p;
    return p;
}

// The parameters as the kernel wants them; false when one is out of range (the refusals of the entries).
PT_AD_HD bool rule(uint32_t kind, float radius, float a, float b, Rule* out) {
    if (kind >= kKinds) return false;
    const double R = (double)radius;
    if (!finite(R) || !(R >= 0.5) || !(R <= 2.5)) return false;
    Rule r;
    r.kind = kind; r.R = R;
    r.m = R + 0.5 > 2.0 ? 2u : (R + 0.5 > 1.0 ? 1u : 0u);      // the largest integer < R + 0.5
    r.alpha = 0.0; r.gR = 0.0;
    r.a3 = r.a2 = r.a0 = r.b3 = r.b2 = r.b1 = r.b0 = 0.0;
    if (kind == kGaussian) {
        const double al = (double)a;
        if (!finite(al) || !(al > 0.0) || !(al <= 16.0)) return false;
        r.alpha = al;
        const double rr = R * R;
        r.gR = exp_neg(al * rr);
    }
    if (kind == kMitchell) {
        const double B = (double)a, C = (double)b;
        if (!finite(B) || !(B >= 0.0) || !(B <= 1.0) || !finite(C) || !(C >= 0.0) || !(C <= 1.0)) return false;
        const double B9 = 9.0 * B, B12 = 12.0 * B, B2 = 2.0 * B, B6 = 6.0 * B, B8 = 8.0 * B;
        const double C6 = 6.0 * C, C30 = 30.0 * C, C48 = 48.0 * C, C24 = 24.0 * C;
        r.a3 = (12.0 - B9) - C6;
        r.a2 = (-18.0 + B12) + C6;
        r.a0 = 6.0 - B2;
        r.b3 = (-B) - C6;
        r.b2 = B6 + C30;
        r.b1 = (-B12) - C48;
        r.b0 = B8 + C24;
    }
    *out = r;
    return true;
}

// f(t), t >= 0
PT_AD_HD double weight1(const Rule& r, double t) {
    if (!(t < r.R)) return 0.0;
    if (r.kind == kBox) return 1.0;
    if (r.kind == kTent) {
        const double q = t / r.R;
        return 1.0 - q;
    }
    if (r.kind == kGaussian) {
        const double tt = t * t;
        const double e = r.alpha * tt;
        return exp_neg(e) - r.gR;
    }
    const double t2 = 2.0 * t;
    const double z = t2 / r.R;
    if (z < 1.0) {
        double h = r.a3 * z;
        h = h + r.a2;
        h = h * z;
        h = h * z;
        h = h + r.a0;
        return h / 6.0;
    }
    if (z < 2.0) {
        double h = r.b3 * z;
        h = h + r.b2;
        h = h * z;
        h = h + r.b1;
        h = h * z;
        h = h + r.b0;
        return h / 6.0;
    }
    return 0.0;
}

// Words 0 and 1 of the camera block of (x, y, sample): Philox4x32-7, ctr (x, y, sample, kDepthCamera), key (0, 0); integer
// arithmetic only, the same statements on the host and in the kernel (pt_device.h's philox4x32_draw with its key folded in)
PT_AD_HD void camera_words(uint32_t x, uint32_t y, uint32_t sample, uint32_t* w0, uint32_t* w1) {
    uint32_t c0 = x, c1 = y, c2 = sample, c3 = kDepthCamera, k0 = 0u, k1 = 0u;
    PT_FLT_UNROLL
    for (int i = 0; i < kPhiloxRounds; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    *w0 = c0; *w1 = c1;
}

PT_AD_HD double u01(uint32_t w) { return (double)(2u * (w >> 9) + 1u) * (1.0 / 16777216.0); }

// ox, oy of sample `sample` of pixel (x, y)
PT_AD_HD void offsets(uint32_t x, uint32_t y, uint32_t sample, double* ox, double* oy) {
    uint32_t w0, w1;
    camera_words(x, y, sample, &w0, &w1);
    *ox = u01(w0); *oy = u01(w1);
}

// The 2 (2 M + 1) one-dimensional factors of one sample: fx[k + M] = f(|k + (ox - 0.5)|), fy[j + M] = f(|j - (oy - 0.5)|), for
// k = px - qx and j = py - qy in [-M, M]
template <int M>
PT_AD_HD void factors(const Rule& r, double ox, double oy, double (&fx)[2 * M + 1], double (&fy)[2 * M + 1]) {
    const double dx = ox - 0.5, dy = oy - 0.5;
    PT_FLT_UNROLL
    for (int k = -M; k <= M; ++k) {
        const double tx = (double)k + dx, ty = (double)k - dy;
        fx[k + M] = weight1(r, tx < 0.0 ? -tx : tx);
        fy[k + M] = weight1(r, ty < 0.0 ? -ty : ty);
    }
}

// one tap into the sums of an output pixel
PT_AD_HD void add_tap(double w, float vr, float vg, float vb, double (&A)[3], double& Wt) {
    const double pr = w * (double)vr, pg = w * (double)vg, pb = w * (double)vb;
    const double nr = A[0] + pr, ng = A[1] + pg, nb = A[2] + pb, nw = Wt + w;
    const bool on = w != 0.0;
    A[0] = on ? nr : A[0]; A[1] = on ? ng : A[1]; A[2] = on ? nb : A[2];
    Wt = on ? nw : Wt;
}

// film: the mean of a channel
PT_AD_HD double mean(double A, double Wt, double P, double dn) { return Wt > 0.0 ? A / Wt : P / dn; }

// The whole rule on host planes (pt_filter_host): samples n * np RGB floats, [s * np + p], sample s has the index first_sample +
// s; out_linear np * 3 floats; out_rgba np * 4 bytes, out_plain np * 3 floats and out_wsum np doubles may be null.
template <int M>
inline void host_film_m(const Rule& r, uint32_t width, uint32_t height, uint32_t n, uint32_t first_sample, const float* samples,
                        float* out_linear, uint8_t* out_rgba, float* out_plain, double* out_wsum) {
    constexpr int F = 2 * M + 1;
    const size_t np = (size_t)width * height;
    std::vector<double> A(3 * np, 0.0), Wt(np, 0.0), P(3 * np, 0.0), fx(F * np), fy(F * np);
    for (uint32_t s = 0; s < n; ++s) {
        const float* smp = samples + (size_t)s * np * 3;
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                double ox, oy, gx[F], gy[F];
                offsets(x, y, first_sample + s, &ox, &oy);
                factors<M>(r, ox, oy, gx, gy);
                const size_t p = (size_t)y * width + x;
                for (int k = 0; k < F; ++k) { fx[F * p + k] = gx[k]; fy[F * p + k] = gy[k]; }
            }
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                const size_t q = (size_t)y * width + x;
                double a[3] = {A[3 * q], A[3 * q + 1], A[3 * q + 2]}, wt = Wt[q];
                for (int j = -M; j <= M; ++j)
                    for (int k = -M; k <= M; ++k) {
                        const int px = (int)x + k, py = (int)y + j;
                        if (px < 0 || py < 0 || px >= (int)width || py >= (int)height) continue;
                        const size_t p = (size_t)py * width + px;
                        const double w = fx[F * p + (k + M)] * fy[F * p + (j + M)];
                        add_tap(w, smp[3 * p], smp[3 * p + 1], smp[3 * p + 2], a, wt);
                    }
                for (int c = 0; c < 3; ++c) { A[3 * q + c] = a[c]; P[3 * q + c] += (double)smp[3 * q + c]; }
                Wt[q] = wt;
            }
    }
    const double dn = (double)n;
    for (size_t q = 0; q < np; ++q) {
        uint32_t q8 = 0xFF000000u;
        for (uint32_t c = 0; c < 3; ++c) {
            const double mc = mean(A[3 * q + c], Wt[q], P[3 * q + c], dn);
            out_linear[3 * q + c] = (float)mc;
            q8 |= ptcas::byte8(mc) << (8 * c);
            if (out_plain) out_plain[3 * q + c] = (float)(P[3 * q + c] / dn);
        }
        if (out_rgba) std::memcpy(out_rgba + 4 * q, &q8, 4);
        if (out_wsum) out_wsum[q] = Wt[q];
    }
}

inline void host_film(const Rule& r, uint32_t width, uint32_t height, uint32_t n, uint32_t first_sample, const float* samples,
                      float* out_linear, uint8_t* out_rgba, float* out_plain, double* out_wsum) {
    if (r.m == 0u) host_film_m<0>(r, width, height, n, first_sample, samples, out_linear, out_rgba, out_plain, out_wsum);
    else if (r.m == 1u) host_film_m<1>(r, width, height, n, first_sample, samples, out_linear, out_rgba, out_plain, out_wsum);
    else host_film_m<2>(r, width, height, n, first_sample, samples, out_linear, out_rgba, out_plain, out_wsum);
}

}  // namespace ptflt
