// pt_upsample.h -- feature-guided upsampling (pt_upsample_device), written once for the kernel (k_upsample in
// pt_film_upsample.h), the host entry (pt_upsample_host in pt_upsample.cpp) and the host compilers of the CPU tests
// (tests/test_upsample_cpu.py).  Build with -ffp-contract=off, like pt_tonemap.h: no compiler fuses what the rule writes apart.
//
// Inputs: the low film c (w x h, 3 floats per pixel), the low feature records f (w x h x 8 floats: albedo rgb, emitter, normal
// xyz, depth -- what pt_render_features_device writes for the low camera, the full camera with width / height replaced) and
// the full-size records F (W x H x 8).  W, H, w, h >= 2, w <= W, h <= H; film row y is top-down.
//
// For a full-size pixel p = (x, y) with record {albedo A, emitter E, normal n, depth d}:
// 1. Position, f64, in this order (multiply, then divide):
//      X = ((x + 0.5) (w - 1)) / (W - 1) - 0.5        Y = h - 0.5 - ((H - 1 - y + 0.5) (h - 1)) / (H - 1)
//    the s / t mapping of the temporal rule; w = W and h = H give X = x, Y = y exactly.  X0 = floor(X), fx = X - X0; Y0, fy alike.
// 2. Taps: the low pixels (Y0, X0), (Y0, X0 + 1), (Y0 + 1, X0), (Y0 + 1, X0 + 1), in this order, with the bilinear weights b_q
//    formed in f64 and rounded to f32.  A tap outside the low image is skipped, and so is a tap with b_q = 0.
// 3. Class of a record: miss (depth = 0), else emitter (emitter > 0), else surface.  A tap of another class than p's has
//    w_q = 0.  Same class: miss or emitter w_q = b_q; surface
//      w_q = b_q max(0, n . n_q)^sigma_n exp(-|d - d_q| / (sigma_d r max(d, 1e-3) + 1e-10)),
//    r = max((W - 1) / (w - 1), (H - 1) / (h - 1)) in f32, w_q = 0 when n . n_q is <= 0 or NaN; formed as one exp2, as
//    k_denoise_step forms its weight.
// 4. Anchor a: the tap with the largest b_q among the taps of p's class; without one, the largest b_q among all taps not
//    skipped.  Ties go to the first tap in the order of 2.
// 5. Interpolation: u_q = c_q / max(albedo_q, 1e-3) per channel in f32 (the a-trous kernels' demodulation), then
//      u = u_a + sum_q w_q (u_q - u_a) / (sum_q w_q + 1e-6),
//    both sums over the taps with w_q > 0, in the order of 2, the quotient as a product with the reciprocal of (sum + 1e-6);
//    these few operations in f64 from the f32 values, u rounded to f32.  A tap with w_q = 0 or w_q NaN (a NaN in its record or
//    in p's) contributes nothing: its film value is not read, a NaN or an infinity included (0 x NaN would be NaN), as a tap
//    with w = 0 of the a-trous filter is not read.  A non-finite anchor still makes its pixel non-finite.  No threshold and no
//    branch on the sum: the value is continuous in the weights (a skipped term is +-0 on finite inputs: the same bits) and
//    falls back to the anchor when nothing agrees with p.  (Why f64: the anchor is the NEAREST tap of p's
//    class, not the heaviest.  Where its weight is small against the others' and its u_a large against the result -- a tap of
//    albedo 0 behind a normal edge -- the f32 sum cancels u_a against -u_a and keeps only ulp(u_a) of the result: 4e-4
//    relative on the crafted inputs of tests/upsample_ref.py.  A dozen f64 operations per pixel cost a streaming kernel nothing.)
// 6. c' = u max(A, 1e-3); the RGBA8 word is c' through sqrt / clamp / `as u8` (ptone::transfer_sqrt: the steps of every render).
//
// Consequences (tests/test_upsample_cpu.py, tests/test_gpu_upsample.py, tests/test_upsample_cases_cpu.py,
// tests/test_gpu_upsample_cases.py): with w = W, h = H and F = f the output is pt_denoise_device's with iterations = 0, bit for
// bit; a tap of another class never influences a pixel that has a tap of its own, whatever its film value holds.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_tonemap.h"

namespace ptup {

constexpr float kAlbedoFloor = 1e-3f, kEps = 1e-6f;
enum { kMiss = 0, kEmitter = 1, kSurface = 2 };

struct alignas(16) Rec { float albedo[3], emitter, normal[3], depth; };   // a feature record: two 16-byte loads
struct Shape { uint32_t W, H, w, h; };

PT_AD_HD int cls(const Rec& f) { return f.depth == 0.0f ? kMiss : (f.emitter > 0.0f ? kEmitter : kSurface); }
PT_AD_HD float albedo(float a) { return fmaxf(a, kAlbedoFloor); }                  // the a-trous kernels' dn_albedo
PT_AD_HD float ratio(const Shape& s) {
    const float rx = (float)(s.W - 1u) / (float)(s.w - 1u), ry = (float)(s.H - 1u) / (float)(s.h - 1u);
    return rx > ry ? rx : ry;
}

// rule 1: (X0, Y0) and (fx, fy) of the full-size pixel (x, y)
PT_AD_HD void position(const Shape& s, uint32_t x, uint32_t y, int* X0, int* Y0, double* fx, double* fy) {
    const double X = (((double)x + 0.5) * (double)(s.w - 1u)) / (double)(s.W - 1u) - 0.5;
    const double Y = (double)s.h - 0.5 - (((double)(s.H - 1u - y) + 0.5) * (double)(s.h - 1u)) / (double)(s.H - 1u);
    const double xf = __builtin_floor(X), yf = __builtin_floor(Y);
    *X0 = (int)xf; *Y0 = (int)yf; *fx = X - xf; *fy = Y - yf;
}

// rules 1-6 for the pixel (x, y) whose record is Fp: out = c' (3 floats)
PT_AD_HD void pixel(const Shape& s, const float* lo_linear, const Rec* lo_feat, const Rec& Fp, uint32_t x, uint32_t y, float sigma_n,
                    float sigma_d, float* out) {
    int X0, Y0;
    double fx, fy;
    position(s, x, y, &X0, &Y0, &fx, &fy);
    const int cp = cls(Fp);
    const float inv_d = 1.0f / (sigma_d * ratio(s) * fmaxf(Fp.depth, 1e-3f) + 1e-10f);
    float b[4], wq[4], u[4][3];
    bool live[4], same[4];
    for (int k = 0; k < 4; ++k) {
        const int i = k & 1, j = k >> 1, qx = X0 + i, qy = Y0 + j;
        b[k] = (float)((i ? fx : 1.0 - fx) * (j ? fy : 1.0 - fy));
        live[k] = qx >= 0 && qy >= 0 && qx < (int)s.w && qy < (int)s.h && b[k] != 0.0f;
        same[k] = false; wq[k] = 0.0f;
        u[k][0] = u[k][1] = u[k][2] = 0.0f;
        if (!live[k]) continue;
        const size_t q = (size_t)qy * s.w + (size_t)qx;
        const Rec fq = lo_feat[q];
        for (int ch = 0; ch < 3; ++ch) u[k][ch] = lo_linear[3 * q + ch] / albedo(fq.albedo[ch]);
        same[k] = cls(fq) == cp;
        if (!same[k]) continue;
        if (cp != kSurface) { wq[k] = b[k]; continue; }
        const float nd = Fp.normal[0] * fq.normal[0] + Fp.normal[1] * fq.normal[1] + Fp.normal[2] * fq.normal[2];
        if (!(nd > 0.0f)) continue;
        const float ed = fabsf(Fp.depth - fq.depth) * inv_d;
        wq[k] = b[k] * ::exp2f(sigma_n * ::log2f(nd) - ed * 1.44269504f);      // b nd^sigma_n exp(-ed), as one exp2
    }
    // rule 4 in two passes over the taps; (ba, ua) follow the anchor, so no array is indexed by a value
    bool any = false;
    for (int k = 0; k < 4; ++k) any = any || (live[k] && same[k]);
    bool have = false;
    float ba = 0.0f, ua[3] = {0.0f, 0.0f, 0.0f};       // (every pixel has a tap that is not skipped: have ends true)
    for (int k = 0; k < 4; ++k)
        if (live[k] && (same[k] || !any) && (!have || b[k] > ba)) {
            have = true; ba = b[k];
            ua[0] = u[k][0]; ua[1] = u[k][1]; ua[2] = u[k][2];
        }
    double wsum = 0.0, num[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 4; ++k) {
        if (!live[k] || !(wq[k] > 0.0f)) continue;          // w_q = 0 or NaN: the tap is not read, whatever its film value holds
        wsum += (double)wq[k];
        for (int ch = 0; ch < 3; ++ch) num[ch] += (double)wq[k] * ((double)u[k][ch] - (double)ua[ch]);
    }
    const double inv = 1.0 / (wsum + (double)kEps);
    for (int ch = 0; ch < 3; ++ch) out[ch] = (float)((double)ua[ch] + num[ch] * inv) * albedo(Fp.albedo[ch]);
}

// rule 6: the RGBA8 word of c'
PT_AD_HD uint32_t rgba8(const float* c) { return ptone::rgba8(ptone::kTransferSqrt, c); }

}  // namespace ptup
