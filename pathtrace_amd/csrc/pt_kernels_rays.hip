// pt_kernels_rays.hip -- the sources of first rays beside the path kernels' own pinhole camera, and the first-hit feature pass
// (pt_kernels_unit.h lists the units).  The path kernels know none of these sources: their rays reach them as path states in the
// queue form, which a launch with src_mode = 1 takes up as it takes up handed-over paths.
//
// A source is a rule struct with one device function, ray(src, x, y, sample, state): for film position (x, y) and sample `sample`
// the origin, the direction, two values only the debug form shows, and the initial throughput (state: the path's index among the
// render's states, which only the caller's rays ask for).  Over the rules stand three kernel templates, one instance per source
// that has the form:
//   k_source_paths<Source>          the rays of one sample batch as depth-0 path states, state i = s_local * np + tile pixel (the
//                                   pixel fastest): the four planes store_state writes, one 16-byte store per lane and plane
//   k_source_feature_rays<Source>   the rays of samples s_base .. s_base + nb - 1 of every image pixel, ray i = s_local * np + p, in
//                                   the rays6 form k_debug_hit reads
//   k_debug_source_rays<Source>     words[4] = x, y, sample, - -> out[kDebugFloats] = o3, d3 and, where there are 8, the two values
// A source of kinds (the projection, the bake) branches on its kind once, inside ray(); the kind is a kernel argument, the same
// for every lane, and a template argument of everything below the branch.
#include "pt_kernels_scan.h"
#include "pt_kernels_vertex.h"
#include "pt_lens.h"
#include "pt_projection.h"
#include "pt_bake.h"
#include "pt_probe_update.h"

namespace PTK_IMPL {
struct SourceRay {
    f3 o, d;
    float e0, e1;       // lens: the lens point dx, dy; projection: a, b
    f3 tp;              // initial throughput
};

// ------------------------------------------------------------------ pinhole camera (pt_render_features_device): camera_ray, the key,
// jitter draws and arithmetic of the path kernels
struct CameraSource {
    static PT_DEV SourceRay ray(const RaySourceF& s, uint32_t x, uint32_t y, uint32_t sample, size_t) {
        SourceRay r;
        camera_ray(s.cam, sample, x, y, r.o, r.d);
        r.e0 = r.e1 = 0.0f;
        r.tp = mk(1.0f, 1.0f, 1.0f);
        return r;
    }
};

// ------------------------------------------------------------------ thin-lens camera (pt_render_lens_device; rule: pt_lens.h)
// lens_ray: camera_ray with the lens point -- the same block of draws, the same statements up to `dir`, then pt_lens.h.
struct LensMath {
    static PT_DEV float div(float a, float b) { return pt_div(a, b); }
    static PT_DEV void sincos2pi(float u, float& s, float& c) { PTD_NS::sincos2pi(u, s, c); }
};
PT_DEV void lens_ray(const CameraF& cam, const LensF& lens, uint32_t sample, uint32_t px, uint32_t py, f3& o, f3& d, float& dx, float& dy) {
    uint32_t dc[4];
    philox4x32_draw(px, py, sample, kDepthCamera, BLK_SURFACE, 0u, dc);
    float ox = u01(dc[0]), oy = u01(dc[1]);
    float wm1 = (float)(cam.width - 1u), hm1 = (float)(cam.height - 1u);
    asm volatile("" : "+v"(wm1), "+v"(hm1));
    float u = pt_div((float)px + ox, wm1);
    float v = pt_div((float)(cam.height - 1u - py) + oy, hm1);
    const f3 cam_o = mk(cam.origin[0], cam.origin[1], cam.origin[2]);
    f3 dir = mk(cam.lower_left[0], cam.lower_left[1], cam.lower_left[2]) +
             mk(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]) * u +
             mk(cam.vertical[0], cam.vertical[1], cam.vertical[2]) * v - cam_o;
    ptlens::disc<LensMath>(u01(dc[2]), u01(dc[3]), &dx, &dy);
    ptlens::Setup L;
    for (int k = 0; k < 3; ++k) { L.lu[k] = lens.lu[k]; L.lv[k] = lens.lv[k]; }
    L.inv_phi = lens.inv_phi;
    const float o3[3] = {cam_o.x, cam_o.y, cam_o.z}, d3[3] = {dir.x, dir.y, dir.z};
    float oo[3], dd[3];
    ptlens::ray(L, o3, d3, dx, dy, oo, dd);
    o = mk(oo[0], oo[1], oo[2]);
    d = normalize(mk(dd[0], dd[1], dd[2]));
}
struct LensSource {
    static constexpr bool kTiled = true;            // y of ray() is the image row of the tile row (TileMap)
    static constexpr uint32_t kDebugFloats = 8;
    static PT_DEV SourceRay ray(const RaySourceF& s, uint32_t x, uint32_t y, uint32_t sample, size_t) {
        SourceRay r;
        lens_ray(s.cam, s.lens, sample, x, y, r.o, r.d, r.e0, r.e1);
        r.tp = mk(1.0f, 1.0f, 1.0f);
        return r;
    }
};

// ------------------------------------------------------------------ projections (pt_render_projection_device; rule: pt_projection.h,
// DESIGN.md 5q).  projection_ray: camera_ray's block of draws and its statements up to `dir` (ptproj::screen), then the kind's rule.
struct ProjMath {
    static PT_DEV float div(float a, float b) { return pt_div(a, b); }
    static PT_DEV float sqrt(float x) { return pt_sqrt(x); }
    static PT_DEV void sincos2pi(float u, float& s, float& c) { PTD_NS::sincos2pi(u, s, c); }
};
template <int KIND>
PT_DEV void projection_ray(const CameraF& cam, const ProjF& pj, uint32_t sample, uint32_t px, uint32_t py, f3& o, f3& d, float& a, float& b) {
    uint32_t dc[4];
    philox4x32_draw(px, py, sample, kDepthCamera, BLK_SURFACE, 0u, dc);
    float u, v, dir[3];
    ptproj::screen<ProjMath>(cam.origin, cam.lower_left, cam.horizontal, cam.vertical, cam.width, cam.height, px, py, u01(dc[0]), u01(dc[1]),
                             &u, &v, dir);
    ptproj::Setup P;
    for (int k = 0; k < 3; ++k) { P.u[k] = pj.u[k]; P.v[k] = pj.v[k]; P.w[k] = pj.w[k]; P.c[k] = pj.c[k]; }
    P.aspect = pj.aspect; P.fov720 = pj.fov720;
    float oo[3], dd[3];
    const bool unnormalised = ptproj::ray<ProjMath, KIND>(P, cam.origin, u, v, dir, oo, dd, &a, &b);
    o = mk(oo[0], oo[1], oo[2]);
    d = mk(dd[0], dd[1], dd[2]);
    if (unnormalised) d = normalize(d);
}
struct ProjectionSource {
    static constexpr bool kTiled = true;
    static constexpr uint32_t kDebugFloats = 8;
    static PT_DEV SourceRay ray(const RaySourceF& s, uint32_t x, uint32_t y, uint32_t sample, size_t) {
        SourceRay r;
        switch (s.proj.kind) {
        case ptproj::kOrthographic: projection_ray<ptproj::kOrthographic>(s.cam, s.proj, sample, x, y, r.o, r.d, r.e0, r.e1); break;
        case ptproj::kFisheye: projection_ray<ptproj::kFisheye>(s.cam, s.proj, sample, x, y, r.o, r.d, r.e0, r.e1); break;
        case ptproj::kEquirect: projection_ray<ptproj::kEquirect>(s.cam, s.proj, sample, x, y, r.o, r.d, r.e0, r.e1); break;
        default: projection_ray<ptproj::kPerspective>(s.cam, s.proj, sample, x, y, r.o, r.d, r.e0, r.e1); break;
        }
        r.tp = mk(1.0f, 1.0f, 1.0f);
        return r;
    }
};

// ------------------------------------------------------------------ light baking (pt_bake_lightmap_device, pt_bake_probes_device; rule:
// pt_bake.h).  bake_ray: the ray of film position (x, y) -- texel (x, y), or direction x of probe y -- and sample
// `sample` by the rule, in this unit's arithmetic (BakeMath: pt_device.h's own u01, sincos2pi, normalize and cosine_sample).  A
// texel lane reads its record's 24 bytes as three 8-byte words (the plane is 8-byte aligned) and draws camera_ray's block for its
// key.  The throughput of an empty texel's ray is 0.
struct BakeMath {
    static PT_DEV float u01(uint32_t w) { return PTD_NS::u01(w); }
    static PT_DEV float sqrt(float x) { return pt_sqrt(x); }
    static PT_DEV void sincos2pi(float u, float& s, float& c) { PTD_NS::sincos2pi(u, s, c); }
    static PT_DEV void normalize(float v[3]) {
        const f3 r = PTD_NS::normalize(mk(v[0], v[1], v[2]));
        v[0] = r.x; v[1] = r.y; v[2] = r.z;
    }
    static PT_DEV void cosine_sample(const float n[3], float r1, float r2, float d[3]) {
        const f3 r = PTD_NS::cosine_sample(mk(n[0], n[1], n[2]), r1, r2);
        d[0] = r.x; d[1] = r.y; d[2] = r.z;
    }
};
template <int KIND>
PT_DEV void bake_ray(const float* __restrict__ data, uint32_t width, uint32_t x, uint32_t y, uint32_t sample, float o[3], float d[3], float& tp) {
    if (KIND == ptbake::kTexel) {
        const float2* __restrict__ r = reinterpret_cast<const float2*>(data) + 3 * ((size_t)y * width + x);
        const float2 r0 = r[0], r1 = r[1], r2 = r[2];
        const float t[6] = {r0.x, r0.y, r1.x, r1.y, r2.x, r2.y};
        uint32_t dc[4];
        philox4x32_draw(x, y, sample, kDepthCamera, BLK_SURFACE, 0u, dc);
        ptbake::texel_ray<BakeMath>(t, dc[0], dc[1], o, d, &tp);
    } else {
        const float* __restrict__ p = data + 3 * (size_t)y;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        ptbake::probe_dir<BakeMath>(x, width, d);
        tp = 1.0f;
    }
}
struct BakeSource {
    static constexpr bool kTiled = false;           // the whole film: tile row = film row
    static constexpr uint32_t kDebugFloats = 6;
    static PT_DEV SourceRay ray(const RaySourceF& s, uint32_t x, uint32_t y, uint32_t sample, size_t) {
        float o[3], d[3], tp;
        if (s.bake.kind == (uint32_t)ptbake::kTexel) bake_ray<ptbake::kTexel>(s.bake.data, s.bake.width, x, y, sample, o, d, tp);
        else bake_ray<ptbake::kProbe>(s.bake.data, s.bake.width, x, y, sample, o, d, tp);
        SourceRay r;
        r.o = mk(o[0], o[1], o[2]); r.d = mk(d[0], d[1], d[2]);
        r.e0 = r.e1 = 0.0f;
        r.tp = mk(tp, tp, tp);
        return r;
    }
};

// ------------------------------------------------------------------ updates of a probe grid (pt_probe_grid_update_device; rule:
// pt_probe_update.h).  Film position (x, y) is direction x of slot y: the origin is the position of probe first + y stride
// by the grid's rule (f64, rounded once), the direction the bake's in this unit's arithmetic under the call's rotation (three
// fmas; the identity by a select).  Throughput 1; a sample index only chooses the path's continuation.
struct ProbeUpdateSource {
    static constexpr bool kTiled = false;           // the whole film: tile row = film row
    static constexpr uint32_t kDebugFloats = 6;
    static PT_DEV SourceRay ray(const RaySourceF& s, uint32_t x, uint32_t y, uint32_t, size_t) {
        const ptupd::Params& u = s.upd.rule;
        float o[3], d[3];
        ptgrid::position(s.upd.grid, u.first + y * u.stride, o);
        ptupd::dir<BakeMath>(x, u.rays_per_probe, u.rotation, ptupd::is_identity(u.rotation), d);
        SourceRay r;
        r.o = mk(o[0], o[1], o[2]); r.d = mk(d[0], d[1], d[2]);
        r.e0 = r.e1 = 0.0f;
        r.tp = mk(1.0f, 1.0f, 1.0f);
        return r;
    }
};

// ------------------------------------------------------------------ caller rays (pt_render_rays_device): float[n][6] in
// state order (sample-major, the pixel fastest), the directions taken as given (not normalised); weights3 (float[n][3], or null =
// 1): the initial throughput.  A lane reads its 24 bytes as three 8-byte words (rays6 is 8-byte aligned).
struct CallerSource {
    static constexpr bool kTiled = false;           // (the position is not read)
    static PT_DEV SourceRay ray(const RaySourceF& s, uint32_t, uint32_t, uint32_t, size_t state) {
        const float2* __restrict__ r = reinterpret_cast<const float2*>(s.rays.rays6) + 3 * state;
        const float2 r0 = r[0], r1 = r[1], r2 = r[2];
        float wx = 1.0f, wy = 1.0f, wz = 1.0f;
        if (s.rays.weights3) {
            const float* __restrict__ w = s.rays.weights3 + 3 * state;
            wx = w[0]; wy = w[1]; wz = w[2];
        }
        SourceRay out;
        out.o = mk(r0.x, r0.y, r1.x); out.d = mk(r1.y, r2.x, r2.y);
        out.e0 = out.e1 = 0.0f;
        out.tp = mk(wx, wy, wz);
        return out;
    }
};

// ------------------------------------------------------------------ the three forms
// a camera path before its first vertex: depth 0, pdf_prev 0, no radiance, eta 1
PT_DEV void store_camera_state(float4* const q[4], uint32_t i, uint32_t yl, uint32_t px, uint32_t s_local, const SourceRay& r) {
    q[0][i] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
    q[1][i] = make_float4(r.d.y, r.d.z, __uint_as_float((yl << 16) | px), __uint_as_float(s_local << 16));
    q[2][i] = make_float4(r.tp.x, r.tp.y, r.tp.z, 0.0f);
    q[3][i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}
template <class Source>
__global__ void __launch_bounds__(kBlock) k_source_paths(SourcePathsArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    uint32_t s_local, pix, yl, px;
    divmod_magic(i, a.np, a.np_magic, s_local, pix);
    divmod_magic(pix, a.src.cam.width, a.w_magic, yl, px);
    const SourceRay r = Source::ray(a.src, px, Source::kTiled ? image_row(a.tile, yl) : yl, a.s_base + s_local, (size_t)a.done * a.np + i);
    store_camera_state(a.q, i, yl, px, s_local, r);
}
template <class Source>
__global__ void __launch_bounds__(kBlock) k_source_feature_rays(RaySourceF src, uint32_t s_base, uint32_t nb, float* __restrict__ rays6) {
    const uint32_t np = src.cam.width * src.cam.height;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nb * np) return;
    const uint32_t s = i / np, p = i - s * np;
    const uint32_t y = p / src.cam.width, x = p - y * src.cam.width;
    const SourceRay q = Source::ray(src, x, y, s_base + s, i);
    float* r = rays6 + 6 * (size_t)i;
    r[0] = q.o.x; r[1] = q.o.y; r[2] = q.o.z; r[3] = q.d.x; r[4] = q.d.y; r[5] = q.d.z;
}
template <class Source>
__global__ void __launch_bounds__(kBlock) k_debug_source_rays(RaySourceF src, const uint32_t* __restrict__ words, uint32_t n, float* __restrict__ outs) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = words + 4 * (size_t)i;
    const SourceRay q = Source::ray(src, w[0], w[1], w[2], i);
    float* out = outs + Source::kDebugFloats * (size_t)i;
    out[0] = q.o.x; out[1] = q.o.y; out[2] = q.o.z; out[3] = q.d.x; out[4] = q.d.y; out[5] = q.d.z;
    if (Source::kDebugFloats == 8) { out[6] = q.e0; out[7] = q.e1; }
}

// ------------------------------------------------------------------ first-hit feature buffers (pt_render_features_device)
// k_feature_resolve maps the hits of one batch of feature rays to records (albedo rgb, emitter | normal xyz, depth) and adds them
// to the pixel's f32 sums in sample order; the sums of earlier batches wait in `out` (load), and the last batch divides by n_samples.
__global__ void __launch_bounds__(kBlock) k_feature_resolve(FeatureResolveArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.np) return;
    float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
    if (a.load) { f0 = a.out[2 * (size_t)p]; f1 = a.out[2 * (size_t)p + 1]; }
    for (uint32_t s = 0; s < a.nb; ++s) {
        const size_t i = (size_t)s * a.np + p;
        const int id = a.ids[i];
        float4 g0 = make_float4(1.f, 1.f, 1.f, 0.f), g1 = make_float4(0.f, 0.f, 0.f, 0.f);   // a miss
        if (id >= 0) {
            const Mat m = load_mat(a.mat, id);
            const float* rec = a.rec + 8 * i;
            if (m.tag == MAT_EMISSIVE) g0.w = 1.0f;
            else g0 = make_float4(fminf(fmaxf(m.color.x, 0.f), 1.f), fminf(fmaxf(m.color.y, 0.f), 1.f), fminf(fmaxf(m.color.z, 0.f), 1.f), 0.f);
            g1 = make_float4(rec[4], rec[5], rec[6], rec[0]);                         // face-forwarded normal, t
        }
        f0.x += g0.x; f0.y += g0.y; f0.z += g0.z; f0.w += g0.w;
        f1.x += g1.x; f1.y += g1.y; f1.z += g1.z; f1.w += g1.w;
    }
    if (a.finalize) {
        const float n = (float)a.n_samples;
        f0 = make_float4(pt_div(f0.x, n), pt_div(f0.y, n), pt_div(f0.z, n), pt_div(f0.w, n));
        f1 = make_float4(pt_div(f1.x, n), pt_div(f1.y, n), pt_div(f1.z, n), pt_div(f1.w, n));
    }
    a.out[2 * (size_t)p] = f0; a.out[2 * (size_t)p + 1] = f1;
}
}  // namespace PTK_IMPL

// The launchers pick the instance from the source's tag; false: the source has no instance of that form, nothing was launched.
namespace ptk {
using namespace PTK_IMPL;
template <class... Params, class... Args>
bool launch_per_item(void (*kernel)(Params...), uint32_t n, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, args...);
    return true;
}
bool PT_LAUNCH(launch_source_paths)(const SourcePathsArgs& a, hipStream_t st) {
    if (a.n == 0u) return true;
    switch (a.src.tag) {
    case kSrcLens: return launch_per_item(k_source_paths<LensSource>, a.n, st, a);
    case kSrcProjection: return launch_per_item(k_source_paths<ProjectionSource>, a.n, st, a);
    case kSrcBake: return launch_per_item(k_source_paths<BakeSource>, a.n, st, a);
    case kSrcRays: return launch_per_item(k_source_paths<CallerSource>, a.n, st, a);
    case kSrcProbeUpdate: return launch_per_item(k_source_paths<ProbeUpdateSource>, a.n, st, a);
    default: return false;
    }
}
bool PT_LAUNCH(launch_source_feature_rays)(const RaySourceF& src, uint32_t s_base, uint32_t nb, float* rays6, hipStream_t st) {
    const uint32_t n = nb * src.cam.width * src.cam.height;
    if (n == 0u) return true;
    switch (src.tag) {
    case kSrcCamera: return launch_per_item(k_source_feature_rays<CameraSource>, n, st, src, s_base, nb, rays6);
    case kSrcLens: return launch_per_item(k_source_feature_rays<LensSource>, n, st, src, s_base, nb, rays6);
    case kSrcProjection: return launch_per_item(k_source_feature_rays<ProjectionSource>, n, st, src, s_base, nb, rays6);
    case kSrcBake: return launch_per_item(k_source_feature_rays<BakeSource>, n, st, src, s_base, nb, rays6);
    case kSrcProbeUpdate: return launch_per_item(k_source_feature_rays<ProbeUpdateSource>, n, st, src, s_base, nb, rays6);
    default: return false;
    }
}
bool PT_LAUNCH(launch_debug_source_rays)(const RaySourceF& src, const uint32_t* words, uint32_t n, float* out, hipStream_t st) {
    if (n == 0u) return true;
    switch (src.tag) {
    case kSrcLens: return launch_per_item(k_debug_source_rays<LensSource>, n, st, src, words, n, out);
    case kSrcProjection: return launch_per_item(k_debug_source_rays<ProjectionSource>, n, st, src, words, n, out);
    case kSrcBake: return launch_per_item(k_debug_source_rays<BakeSource>, n, st, src, words, n, out);
    case kSrcProbeUpdate: return launch_per_item(k_debug_source_rays<ProbeUpdateSource>, n, st, src, words, n, out);
    default: return false;
    }
}
void PT_LAUNCH(launch_feature_resolve)(const FeatureResolveArgs& a, hipStream_t st) {
    if (a.np) hipLaunchKernelGGL(k_feature_resolve, dim3((a.np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
}  // namespace ptk
