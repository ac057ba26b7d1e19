// pt_probe_grid.h -- the rule of the irradiance volume (pt_probe_grid_bake_device, pt_probe_shade_device, pt_render_probe_lit_device,
// DESIGN.md 5s), written once for the kernels (k_probe_positions and k_probe_shade in pt_film_probe.h), the host entries
// (pt_probe_grid.cpp) and the host compilers of the tests.  Build with -ffp-contract=off: no compiler fuses what the rule writes
// apart.  f64 with + - * /, square root, comparisons and selects in a fixed order; no libm.
//
// Grid: probe (ix, iy, iz) of counts (nx, ny, nz) has index p = (iz ny + iy) nx + ix and the position origin_a + i_a spacing_a,
// computed in f64 and rounded to f32 once: the format pt_bake_probes_* takes.  A grid is VALID when no count is 0, origin and
// spacing are finite, the spacing is > 0 on every axis with more than one probe, and nx ny nz <= 65535 (the bake's row limit).
//
// A pixel (x, y) of a W x H image: the feature record {albedo rgb, emitter, normal n, depth d} and the camera (o, l, hz, vt).
//   1. UNLIT when d is not > 0, emitter > 0, one of n, d, albedo is not finite, the f64 length of n is not > 0, or the point P of 2
//      is not finite (so W = 1 or H = 1: s and t divide by W - 1 and H - 1).  An unlit pixel reads no probe; its value is the
//      caller's (the fallback pixel, or +0.0).
//   2. s = (x + 0.5) / (W - 1), t = (H - 1 - y + 0.5) / (H - 1), D = l + s hz + t vt - o, P = o + d (D (1 / |D|)): the statements
//      of tm_reproject (pt_film_temporal.h) in its order, RESTATED here -- that function is device-only and stays as it is, so that
//      the temporal kernels keep their machine code.  nn = n / |n| in f64, Q = P + normal_bias nn.
//   3. per axis with more than one probe: g = (Q_a - origin_a) / spacing_a (NaN: unlit), clamped to [0, count - 1];
//      i = min(floor(g), count - 2), f = g - i.  An axis with one probe: i = 0, f = 0, the upper corner is the lower one, g is
//      never formed (its spacing may be 0).
//   4. corner j = 0..7 (bit 0 = x, bit 1 = y, bit 2 = z): w_j = (wx wy) wz, each f or 1 - f.  kFacing: v = pos_j - P from the f32
//      position, c = (v . nn) / |v| (1 when |v| = 0), w_j = w_j (((c + 1) / 2)^2 + 0.2) -- the backface weight of Majercik et al.
//      2019 without its visibility term.  (With it: pt_probe_vis.h, whose MomentMaps replaces the last statement through the
//      Visibility argument of shade_rule below; the two weights here go through NoVisibility and keep their arithmetic.)
//   5. every coefficient: C = C_0 + (sum_{j=1..7} w_j (C_j - C_0)) / (sum_{j=0..7} w_j), both sums from 0.0 with j ascending:
//      a constant field comes out exactly.
//   6. E_c = sum_k (A_l C[k][c]) Y_k(nn) from 0.0 with k ascending (sh_basis and A of pt_bake.h, the order of ptbake::sh_irradiance);
//      E_c < 0 becomes 0 (SH ringing; NaN stays NaN); out_c = (float)((a_c E_c) / pi) with a_c = albedo_c, 0 when albedo_c < 0.
// The RGBA8 word of a pixel is its linear value through ptone::transfer_sqrt, as everywhere.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_bake.h"          // ptbake::sh_basis, kPi; PT_AD_HD
#include "pt_probe_params.h"  // ptgrid::Grid
#include "pt_tonemap.h"       // ptone::transfer_sqrt

namespace ptgrid {

enum { kTrilinear = 0, kFacing = 1, kWeights = 2 };
constexpr uint32_t kMaxProbes = 65535u;

PT_AD_HD bool finite(double v) { return v - v == 0.0; }
PT_AD_HD bool finitef(float v) { return v - v == 0.0f; }
PT_AD_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the number of probes, 0 for an invalid grid
PT_AD_HD uint32_t count(const Grid& g) {
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) {
        if (g.counts[a] == 0u || g.counts[a] > kMaxProbes) return 0u;
        if (!finite(g.origin[a]) || !finite(g.spacing[a])) return 0u;
        if (g.counts[a] > 1u && !(g.spacing[a] > 0.0)) return 0u;
        n *= g.counts[a];
    }
    return n > kMaxProbes ? 0u : (uint32_t)n;
}

// coordinate a of the probe with index i on that axis
PT_AD_HD float coordinate(const Grid& g, int a, uint32_t i) { return (float)(g.origin[a] + (double)i * g.spacing[a]); }

// the position of probe p (p < count)
PT_AD_HD void position(const Grid& g, uint32_t p, float out[3]) {
    const uint32_t nx = g.counts[0], ny = g.counts[1];
    const uint32_t ix = p % nx, r = p / nx;
    out[0] = coordinate(g, 0, ix); out[1] = coordinate(g, 1, r % ny); out[2] = coordinate(g, 2, r / ny);
}

// The visibility term of step 4 is a type: NoVisibility here (the two weights above, nothing added to their arithmetic), and
// ptvis::MomentMaps of pt_probe_vis.h, whose factor(probe, Q, pos) is the Chebyshev weight of the probe's moment map
// towards the biased point Q and which replaces the last statement of kFacing by its own.
struct NoVisibility {
    static constexpr bool kOn = false;
    PT_AD_HD double weight(uint32_t, const double*, const double*, double tri, double) const { return tri; }
};

// One pixel: rec = the 8 floats of its feature record, cam = o3, l3, hz3, vt3, sh27 = float[count][9][3].  false: unlit (nothing
// read from sh27, out untouched).  Every loop unrolls: on the device the arrays live in registers.
template <class Visibility>
PT_AD_HD bool shade_rule(const Grid& g, float normal_bias, uint32_t weight, uint32_t W, uint32_t H, uint32_t x, uint32_t y, const float rec[8],
                         const double cam[12], const float* sh27, const Visibility& vis, float out[3]) {
    // 1
    const float d = rec[7];
    bool ok = d > 0.0f && finitef(d) && !(rec[3] > 0.0f);
    PT_BAKE_UNROLL
    for (int k = 0; k < 3; ++k) ok = ok && finitef(rec[k]) && finitef(rec[4 + k]);
    const double n[3] = {(double)rec[4], (double)rec[5], (double)rec[6]};
    const double len = __builtin_sqrt(dot3(n, n));
    ok = ok && len > 0.0;
    // 2
    const double* o = cam; const double* l = cam + 3; const double* hz = cam + 6; const double* vt = cam + 9;
    const double W1 = (double)(W - 1u), H1 = (double)(H - 1u);
    const double s = ((double)x + 0.5) / W1, t = ((double)(H - 1u - y) + 0.5) / H1;
    double D[3], P[3];
    PT_BAKE_UNROLL
    for (int k = 0; k < 3; ++k) D[k] = l[k] + s * hz[k] + t * vt[k] - o[k];
    const double inv_len = 1.0 / __builtin_sqrt(dot3(D, D));
    PT_BAKE_UNROLL
    for (int k = 0; k < 3; ++k) {
        P[k] = o[k] + (double)d * (D[k] * inv_len);
        ok = ok && finite(P[k]);
    }
    if (!ok) return false;
    double nn[3];
    PT_BAKE_UNROLL
    for (int k = 0; k < 3; ++k) nn[k] = n[k] / len;
    // 3
    uint32_t i0[3];
    double f[3];
    PT_BAKE_UNROLL
    for (int a = 0; a < 3; ++a) {
        i0[a] = 0u; f[a] = 0.0;
        if (g.counts[a] > 1u) {
            const double Q = P[a] + (double)normal_bias * nn[a];
            double q = (Q - g.origin[a]) / g.spacing[a];
            if (q != q) return false;
            const double top = (double)(g.counts[a] - 1u);
            q = q < 0.0 ? 0.0 : (q > top ? top : q);
            uint32_t i = (uint32_t)q;                         // floor: q >= 0
            if (i > g.counts[a] - 2u) i = g.counts[a] - 2u;
            i0[a] = i; f[a] = q - (double)i;
        }
    }
    // 4
    uint32_t idx[8];
    double w[8], den = 0.0;
    PT_BAKE_UNROLL
    for (int j = 0; j < 8; ++j) {
        uint32_t c[3];
        double wa[3];
        PT_BAKE_UNROLL
        for (int a = 0; a < 3; ++a) {
            const bool up = ((j >> a) & 1) != 0;
            wa[a] = up ? f[a] : 1.0 - f[a];
            c[a] = i0[a] + ((up && g.counts[a] > 1u) ? 1u : 0u);
        }
        double wj = wa[0] * wa[1];
        wj = wj * wa[2];
        if (Visibility::kOn || weight == (uint32_t)kFacing) {
            double v[3];
            PT_BAKE_UNROLL
            for (int a = 0; a < 3; ++a) v[a] = (double)coordinate(g, a, c[a]) - P[a];
            const double vlen = __builtin_sqrt(dot3(v, v));
            const double vn = dot3(v, nn);
            const double cs = vlen == 0.0 ? 1.0 : vn / vlen;
            const double h = (cs + 1.0) / 2.0;
            if (Visibility::kOn) {
                double Q[3], pos[3];
                PT_BAKE_UNROLL
                for (int a = 0; a < 3; ++a) { Q[a] = P[a] + (double)normal_bias * nn[a]; pos[a] = (double)coordinate(g, a, c[a]); }
                wj = vis.weight((c[2] * g.counts[1] + c[1]) * g.counts[0] + c[0], Q, pos, wj, h * h + 0.2);
            } else {
                wj = wj * (h * h + 0.2);
            }
        }
        idx[j] = (c[2] * g.counts[1] + c[1]) * g.counts[0] + c[0];
        w[j] = wj;
        den = den + wj;
    }
    // 5
    const float* c0 = sh27 + 27 * (size_t)idx[0];
    double base[27], acc[27];
    PT_BAKE_UNROLL
    for (int k = 0; k < 27; ++k) { base[k] = (double)c0[k]; acc[k] = 0.0; }
    PT_BAKE_UNROLL
    for (int j = 1; j < 8; ++j) {
        const float* cj = sh27 + 27 * (size_t)idx[j];
        PT_BAKE_UNROLL
        for (int k = 0; k < 27; ++k) acc[k] = acc[k] + w[j] * ((double)cj[k] - base[k]);
    }
    // 6
    double Y[9];
    ptbake::sh_basis(nn[0], nn[1], nn[2], Y);
    const double A[3] = {ptbake::kPi, 2.0 * ptbake::kPi / 3.0, ptbake::kPi / 4.0};
    double e[3] = {0.0, 0.0, 0.0};
    PT_BAKE_UNROLL
    for (int k = 0; k < 9; ++k)
        PT_BAKE_UNROLL
        for (int ch = 0; ch < 3; ++ch) {
            const double C = base[3 * k + ch] + acc[3 * k + ch] / den;
            e[ch] = e[ch] + (A[k == 0 ? 0 : (k < 4 ? 1 : 2)] * C) * Y[k];
        }
    PT_BAKE_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        const double E = e[ch] < 0.0 ? 0.0 : e[ch];
        const double a = (double)rec[ch] < 0.0 ? 0.0 : (double)rec[ch];
        out[ch] = (float)((a * E) / ptbake::kPi);
    }
    return true;
}
PT_AD_HD bool shade(const Grid& g, float normal_bias, uint32_t weight, uint32_t W, uint32_t H, uint32_t x, uint32_t y, const float rec[8],
                    const double cam[12], const float* sh27, float out[3]) {
    return shade_rule(g, normal_bias, weight, W, H, x, y, rec, cam, sh27, NoVisibility(), out);
}

// the RGBA8 word of a linear pixel
PT_AD_HD uint32_t rgba8(const float v[3]) {
    return 0xFF000000u | ptone::transfer_sqrt(v[0]) | (ptone::transfer_sqrt(v[1]) << 8) | (ptone::transfer_sqrt(v[2]) << 16);
}

}  // namespace ptgrid
