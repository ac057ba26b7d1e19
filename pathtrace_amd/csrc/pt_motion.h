// pt_motion.h -- the per-object motion maps of pt_denoise_temporal_motion_device, written once for the library
// (pt_denoise.cpp; pt_debug_motion_maps, pt_host.cpp) and for host compilers of tests.  Plain f64 host arithmetic, no device code; build
// with -ffp-contract=off like the rest of the library.
//
// For object k the affine map x -> A x + b carries a point of the object's CURRENT pose to the same material point of its
// HISTORY pose (the pose at the last temporal frame that stored a history):
//   sphere (c, r) now, (c', r') then:          A = (r'/r) I,  b = c' - (r'/r) c
//   triangle (v0, v1, v2) now, primed then:    e1 = v1 - v0, e2 = v2 - v0, n = (e1 x e2)/|e1 x e2|, E = [e1 e2 n] (columns),
//                                              A = E' E^-1,  b = v0' - A v0
// E^-1 in closed form: its rows are (e2 x n, n x e1, e1 x e2) / det E, and det E = e1 . (e2 x n) = |e1 x e2|.
// A map is INVALID when a radius is <= 0, a triangle has zero area, or an entry of (A, b) is not finite; it is the IDENTITY
// iff the nine f64 shape fields are bitwise equal now and then (decided on the fields, never on A), and then A = I, b = 0
// exactly.  Both flags may be set (an unchanged degenerate object).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace ptmo {

constexpr uint32_t kIdentity = 1u, kInvalid = 2u;

inline void cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
inline double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// e1, e2 and the unit normal of a triangle's nine fields -> E's columns; false: zero area (or not finite)
inline bool frame(const double* s, double* e1, double* e2, double* n, double* area2) {
    for (int k = 0; k < 3; ++k) { e1[k] = s[3 + k] - s[k]; e2[k] = s[6 + k] - s[k]; }
    cross(e1, e2, n);
    *area2 = std::sqrt(dot(n, n));
    if (!(*area2 > 0.0) || !std::isfinite(*area2)) return false;
    for (int k = 0; k < 3; ++k) n[k] /= *area2;
    return true;
}

// cur, hist: the nine shape fields of PtObject now and in the history.  out: A row-major (9), then b (3).  -> flags
inline uint32_t motion_map(uint32_t triangle, const double* cur, const double* hist, double* out) {
    uint32_t flags = std::memcmp(cur, hist, 9 * sizeof(double)) == 0 ? kIdentity : 0u;
    bool ok = true;
    for (int k = 0; k < 12; ++k) out[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    if (!triangle) {
        const double r = cur[3], r2 = hist[3];
        ok = r > 0.0 && r2 > 0.0;
        if (ok && !flags) {
            const double s = r2 / r;
            out[0] = out[4] = out[8] = s;
            for (int k = 0; k < 3; ++k) out[9 + k] = hist[k] - s * cur[k];
        }
    } else {
        double e1[3], e2[3], n[3], f1[3], f2[3], m[3], det, det2;
        ok = frame(cur, e1, e2, n, &det);
        ok = frame(hist, f1, f2, m, &det2) && ok;
        if (ok && !flags) {
            double r0[3], r1[3], r2[3];                       // rows of E^-1
            cross(e2, n, r0); cross(n, e1, r1); cross(e1, e2, r2);
            for (int j = 0; j < 3; ++j) { r0[j] /= det; r1[j] /= det; r2[j] /= det; }
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) out[3 * i + j] = f1[i] * r0[j] + f2[i] * r1[j] + m[i] * r2[j];
            for (int i = 0; i < 3; ++i) out[9 + i] = hist[i] - (out[3 * i] * cur[0] + out[3 * i + 1] * cur[1] + out[3 * i + 2] * cur[2]);
        }
    }
    for (int k = 0; k < (triangle ? 9 : 4); ++k) ok = ok && std::isfinite(cur[k]) && std::isfinite(hist[k]);
    for (int k = 0; k < 12; ++k) ok = ok && std::isfinite(out[k]);
    if (!ok) flags |= kInvalid;
    return flags;
}

}  // namespace ptmo
