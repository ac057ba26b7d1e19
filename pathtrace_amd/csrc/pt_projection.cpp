// pt_projection.cpp -- the host side of the projections and the caller's rays that is not the render driver's
// (pt_api.cpp: render_injected_impl and render_source_impl): the checks and the device's words (pt_projection.h), the defaults, the rule
// on the CPU, the debug entry, and the entries of the projection forms pt_denoise.cpp holds.  The entries' rule and the host
// render's staging: pt_entry.h.
#include "pt_entry.h"
#include "pt_filter.h"        // ptflt::camera_words: words 0 and 1 of the camera block, on the host
#include "pt_projection.h"

// The projection and the camera's frame checked (a check answers in the entry's name, who), the device's words in f32.  No context.
int projection_setup(const char* who, const PtCamera* cam, const PtProjection* proj, ptk::ProjF* out) {
    ptproj::Setup s;
    switch (ptproj::setup(cam->origin, cam->lower_left, cam->horizontal, cam->vertical, proj->kind, proj->reserved, proj->fov_degrees, &s)) {
    case ptproj::kOk: break;
    case ptproj::kBadKind: return fail(PT_ERR_INVALID_ARG, "%s: unknown projection kind %u", who, proj->kind);
    case ptproj::kBadReserved: return fail(PT_ERR_INVALID_ARG, "%s: the projection's reserved word must be 0", who);
    case ptproj::kBadFov: return fail(PT_ERR_INVALID_ARG, "%s: fisheye fov_degrees %g must be finite and in (0, 360]", who, proj->fov_degrees);
    default:
        return fail(PT_ERR_INVALID_ARG, "%s: degenerate camera (the view axis, horizontal and vertical must have a finite length > 0)", who);
    }
    for (int k = 0; k < 3; ++k) { out->u[k] = s.u[k]; out->v[k] = s.v[k]; out->w[k] = s.w[k]; out->c[k] = s.c[k]; }
    out->aspect = s.aspect; out->fov720 = s.fov720;
    out->kind = proj->kind;
    return PT_OK;
}

namespace {

// The render's exact arithmetic on the host: IEEE division and square root, and the statements of pt_device.h's sincos2pi in
// its exact form (the GPU tests hold the two together bit for bit: pt_debug_projection_rays against pt_projection_rays_host).
struct HostMath {
    static float div(float a, float b) { return a / b; }
    static float sqrt(float x) { return __builtin_sqrtf(x); }
    static void sincos2pi(float u, float& s, float& c) {
        const float k = __builtin_rintf(u * 4.0f);
        const float r = __builtin_fmaf(k, -0.25f, u);
        const float t = r * 6.28318530717958647692f;
        const float z = t * t;
        const float sp = __builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
        const float st = __builtin_fmaf(sp * z, t, t);
        const float cp = __builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
        const float ct = __builtin_fmaf(cp * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
        const int q = ((int)k) & 3;
        float ss = (q & 1) ? ct : st;
        float cc = (q & 1) ? st : ct;
        if (q == 1 || q == 2) cc = -cc;
        if (q == 2 || q == 3) ss = -ss;
        s = ss; c = cc;
    }
};
float host_u01(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * (1.0f / 16777216.0f); }      // exact: (2k + 1) / 2^24
// pt_device.h's normalize in exact arithmetic: the dot product's two FMAs, sqrt, one reciprocal, three products
void host_normalize(float d[3]) {
    const float len = __builtin_sqrtf(__builtin_fmaf(d[2], d[2], __builtin_fmaf(d[1], d[1], d[0] * d[0])));
    if (len > 0.0f) {
        const float inv = 1.0f / len;
        for (int k = 0; k < 3; ++k) d[k] = d[k] * inv;
    }
}
template <int KIND>
void host_ray(const ptproj::Setup& P, const ptk::CameraF& cf, uint32_t x, uint32_t y, uint32_t sample, float* out8) {
    uint32_t w0, w1;
    ptflt::camera_words(x, y, sample, &w0, &w1);
    float u, v, dir[3], a, b;
    ptproj::screen<HostMath>(cf.origin, cf.lower_left, cf.horizontal, cf.vertical, cf.width, cf.height, x, y, host_u01(w0), host_u01(w1), &u, &v,
                             dir);
    if (ptproj::ray<HostMath, KIND>(P, cf.origin, u, v, dir, out8, out8 + 3, &a, &b)) host_normalize(out8 + 3);
    out8[6] = a; out8[7] = b;
}

}  // namespace

extern "C" {

void pt_default_projection(PtProjection* out) {
    if (!out) return;
    out->kind = PT_PROJ_PERSPECTIVE;
    out->reserved = 0;
    out->fov_degrees = 180.0;
}

int pt_render_projection_device(PtContext* c, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* prm, float* d_linear,
                                uint8_t* d_rgba) {
    return render_source_impl("pt_render_projection_device", c, cam, {nullptr, proj}, prm, d_linear, d_rgba);
}

int pt_render_projection_host(PtContext* c, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* prm, float* out_linear,
                              uint8_t* out_rgba) {
    if (!c || !cam || !proj || !prm || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_projection_host: null argument");
    ptk::ProjF checked;
    if (int bad = projection_setup("pt_render_projection_host", cam, proj, &checked)) return bad;      // before the staging is touched
    const size_t np = (size_t)pt_tile_rows(cam->height, prm->band_rows, prm->band_index, prm->band_count ? prm->band_count : 1) * cam->width;
    if (np == 0) return render_source_impl("pt_render_projection_host", c, cam, {nullptr, proj}, prm, nullptr, nullptr);   // validates, renders nothing
    HIP_TRY(hipSetDevice(c->device));
    return render_staged(c, np * 3, out_rgba ? np * 4 : 0, [&](float* d_linear, uint8_t* d_rgba) {
        return render_source_impl("pt_render_projection_host", c, cam, {nullptr, proj}, prm, d_linear, d_rgba);
    }, [&] { return copy_back({{out_linear, c->host_lin.p, np * 3 * sizeof(float)}, {out_rgba, c->host_rgba.p, np * 4}}); });
}

int pt_render_features_projection_device(PtContext* c, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* prm,
                                         uint32_t n_samples, float* d_features) {
    if (!proj) return fail(PT_ERR_INVALID_ARG, "pt_render_features_projection_device: null argument");
    return features_source_device("pt_render_features_projection_device", c, cam, {nullptr, proj}, prm, n_samples, d_features);
}

int pt_render_projection_denoised(PtContext* c, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* prm,
                                  uint32_t feature_samples, const PtDenoise* dn, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                  float* out_features) {
    if (!proj) return fail(PT_ERR_INVALID_ARG, "pt_render_projection_denoised: null argument");
    return render_source_denoised_host("pt_render_projection_denoised", c, cam, {nullptr, proj}, prm, feature_samples, dn, out_linear, out_rgba,
                                       out_noisy, out_features);
}

int pt_render_rays_device(PtContext* c, uint32_t width, uint32_t height, const PtRenderParams* prm, const float* d_rays6, const float* d_weights3,
                          float* d_linear, uint8_t* d_rgba) {
    const char* const who = "pt_render_rays_device";
    if (!c || !prm || !d_rays6) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((uintptr_t)d_rays6 % 8u) return fail(PT_ERR_INVALID_ARG, "%s: d_rays6 must be 8-byte aligned", who);
    if ((uintptr_t)d_weights3 % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_weights3 must be 4-byte aligned", who);
    // a camera for the tile's geometry only (no camera ray is generated): the image size, and a frame nothing reads
    PtCamera cam{};
    cam.lower_left[0] = cam.lower_left[1] = cam.lower_left[2] = -1.0;
    cam.horizontal[0] = 2.0; cam.vertical[1] = 2.0;
    cam.width = width; cam.height = height;
    ptk::RaySourceF s{};
    s.tag = ptk::kSrcRays;
    s.cam = camera_f32(&cam);
    s.rays.rays6 = d_rays6; s.rays.weights3 = d_weights3;
    return render_injected_impl(who, c, &cam, prm, s, d_linear, d_rgba);
}

int pt_projection_setup_host(const PtCamera* cam, const PtProjection* proj, float* out11) {
    if (!cam || !proj || !out11) return fail(PT_ERR_INVALID_ARG, "pt_projection_setup_host: null argument");
    ptk::ProjF p;
    if (int rc = projection_setup("pt_projection_setup_host", cam, proj, &p)) return rc;
    for (int k = 0; k < 3; ++k) { out11[k] = p.u[k]; out11[3 + k] = p.v[k]; out11[6 + k] = p.w[k]; }
    out11[9] = p.aspect; out11[10] = p.fov720;
    return PT_OK;
}

int pt_projection_rays_host(const PtCamera* cam, const PtProjection* proj, const uint32_t* xys, uint32_t n, float* out8) {
    if (!cam || !proj || (n && (!xys || !out8))) return fail(PT_ERR_INVALID_ARG, "pt_projection_rays_host: null argument");
    ptk::ProjF p;
    int rc;
    if ((rc = projection_setup("pt_projection_rays_host", cam, proj, &p)) || (rc = check_camera_size(cam))) return rc;
    ptproj::Setup P;
    for (int k = 0; k < 3; ++k) { P.u[k] = p.u[k]; P.v[k] = p.v[k]; P.w[k] = p.w[k]; P.c[k] = p.c[k]; }
    P.aspect = p.aspect; P.fov720 = p.fov720;
    const ptk::CameraF cf = camera_f32(cam);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = xys[3 * i], y = xys[3 * i + 1], s = xys[3 * i + 2];
        float* out = out8 + 8 * i;
        switch (p.kind) {
        case PT_PROJ_ORTHOGRAPHIC: host_ray<ptproj::kOrthographic>(P, cf, x, y, s, out); break;
        case PT_PROJ_FISHEYE: host_ray<ptproj::kFisheye>(P, cf, x, y, s, out); break;
        case PT_PROJ_EQUIRECT: host_ray<ptproj::kEquirect>(P, cf, x, y, s, out); break;
        default: host_ray<ptproj::kPerspective>(P, cf, x, y, s, out); break;
        }
    }
    return PT_OK;
}

int pt_debug_projection_rays(PtContext* c, const PtCamera* cam, const PtProjection* proj, const uint32_t* xys, uint32_t n, uint32_t exact_math,
                             float* out8) {
    if (!c || !cam || !proj || (n && (!xys || !out8))) return fail(PT_ERR_INVALID_ARG, "pt_debug_projection_rays: null argument");
    ptk::ProjF p;
    int rc;
    if ((rc = projection_setup("pt_debug_projection_rays", cam, proj, &p)) || (rc = check_camera_size(cam))) return rc;
    ptk::RaySourceF s{};
    s.tag = ptk::kSrcProjection;
    s.cam = camera_f32(cam);
    s.proj = p;
    return debug_source_rays(c, s, xys, n, exact_math, 8, out8);
}

}  // extern "C"
