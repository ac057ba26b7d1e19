// pt_bake.cpp -- the host side of light baking: lightmaps and probe bakes as users of the injected-path driver
// (render_injected_impl, pt_api.cpp) with the bake as their ray source, the launches that follow the render (k_bake_mask, k_probe_sh),
// the rule on the CPU (pt_bake.h in exact arithmetic), the SH entries that need no device, and the debug entry.  The entries' rule,
// check_plane and the host entries' staging: pt_entry.h.
#include "pt_entry.h"
#include "pt_bake.h"
#include "pt_filter.h"        // ptflt::camera_words: words 0 and 1 of the camera block, on the host

namespace {

// The film of a bake: width x rows of texels, or directions x probes.  Checked before anything else looks at the context.
int check_film(const char* who, uint32_t kind, uint32_t width, uint32_t height) {
    if (kind >= (uint32_t)ptbake::kKinds) return fail(PT_ERR_INVALID_ARG, "%s: unknown bake kind %u", who, kind);
    if (kind == (uint32_t)ptbake::kTexel) {
        if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARG, "%s: lightmap %ux%u: a zero size", who, width, height);
        if (width > 65535u || height > 65535u) return fail(PT_ERR_INVALID_ARG, "%s: lightmap %ux%u: width and height must be < 65536", who, width, height);
    } else {
        if (height == 0) return fail(PT_ERR_INVALID_ARG, "%s: n_probes is 0: a zero size", who);
        if (width == 0) return fail(PT_ERR_INVALID_ARG, "%s: rays_per_probe must be > 0", who);
        if (width > 65535u || height > 65535u)
            return fail(PT_ERR_INVALID_ARG, "%s: %u probes of %u rays: n_probes and rays_per_probe must be < 65536", who, height, width);
    }
    return PT_OK;
}
int check_whole(const char* who, const PtRenderParams* prm) { return check_whole_image(who, " bakes", "", prm, /*band_index_too=*/false); }

// a camera for the film's geometry only (no camera ray is generated): the size, and a frame nothing reads
PtCamera film_camera(uint32_t width, uint32_t height) {
    PtCamera cam{};
    cam.lower_left[0] = cam.lower_left[1] = cam.lower_left[2] = -1.0;
    cam.horizontal[0] = 2.0; cam.vertical[1] = 2.0;
    cam.width = width; cam.height = height;
    return cam;
}

}  // namespace

ptk::RaySourceF bake_source(uint32_t kind, uint32_t width, uint32_t height, const float* d_data) {
    const PtCamera cam = film_camera(width, height);
    ptk::RaySourceF s{};
    s.tag = ptk::kSrcBake;
    s.cam = camera_f32(&cam);
    s.bake.data = d_data; s.bake.kind = kind; s.bake.width = width;
    return s;
}

namespace {

// The render of a bake: the planes checked by the caller; the bake's paths form fills the inject planes of every sample batch
int bake_render(const char* who, PtContext* c, uint32_t kind, uint32_t width, uint32_t height, const float* d_data, const PtRenderParams* prm,
                float* d_linear, uint8_t* d_rgba) {
    const PtCamera cam = film_camera(width, height);
    return render_injected_impl(who, c, &cam, prm, bake_source(kind, width, height, d_data), d_linear, d_rgba, /*no_camera=*/true);
}

int lightmap_impl(const char* who, PtContext* c, uint32_t width, uint32_t height, const float* d_texels6, const PtRenderParams* prm,
                  float* d_linear, uint8_t* d_rgba) {
    int rc;
    if ((rc = bake_render(who, c, ptbake::kTexel, width, height, d_texels6, prm, d_linear, d_rgba))) return rc;
    ptk::launch_bake_mask(d_texels6, width * height, d_linear, d_rgba, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}
int check_lightmap(const char* who, const void* c, uint32_t width, uint32_t height, const void* texels6, const PtRenderParams* prm, const void* linear,
                   const void* rgba, uint32_t in_align) {
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_film(who, ptbake::kTexel, width, height)) || (rc = check_whole(who, prm)) || (rc = check_plane(who, "texels6", texels6, in_align)) ||
        (rc = check_plane(who, "the linear output", linear, 4)) || (rc = check_plane(who, "the RGBA8 output", rgba, 4, true)))
        return rc;
    return PT_OK;
}

int probes_impl(const char* who, PtContext* c, const float* d_positions3, uint32_t n_probes, uint32_t rays_per_probe, const PtRenderParams* prm,
                float* d_radiance, float* d_sh27) {
    int rc;
    if ((rc = bake_render(who, c, ptbake::kProbe, rays_per_probe, n_probes, d_positions3, prm, d_radiance, nullptr))) return rc;
    if (d_sh27) {
        ptk::launch_probe_sh(n_probes, rays_per_probe, d_radiance, d_sh27, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return PT_OK;
}
int check_probes(const char* who, const void* c, const void* positions3, uint32_t n_probes, uint32_t rays_per_probe, const PtRenderParams* prm,
                 const void* radiance, const void* sh27) {
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_film(who, ptbake::kProbe, rays_per_probe, n_probes)) || (rc = check_whole(who, prm)) ||
        (rc = check_plane(who, "positions3", positions3, 4)) || (rc = check_plane(who, "the radiance output", radiance, 4)) ||
        (rc = check_plane(who, "sh27", sh27, 4, true)))
        return rc;
    return PT_OK;
}

// xys = n x (x, y, sample) inside the film
int check_xys(const char* who, uint32_t width, uint32_t height, const uint32_t* xys, uint32_t n) {
    for (size_t i = 0; i < n; ++i)
        if (xys[3 * i] >= width || xys[3 * i + 1] >= height)
            return fail(PT_ERR_INVALID_ARG, "%s: position (%u, %u) of entry %zu lies outside the %ux%u film", who, xys[3 * i], xys[3 * i + 1], i, width,
                        height);
    return PT_OK;
}
size_t data_floats(uint32_t kind, uint32_t width, uint32_t height) {
    return kind == (uint32_t)ptbake::kTexel ? 6 * (size_t)width * height : 3 * (size_t)height;
}

}  // namespace

extern "C" {

int pt_bake_lightmap_device(PtContext* c, uint32_t width, uint32_t height, const float* d_texels6, const PtRenderParams* prm, float* d_linear,
                            uint8_t* d_rgba) {
    if (int rc = check_lightmap("pt_bake_lightmap_device", c, width, height, d_texels6, prm, d_linear, d_rgba, 8)) return rc;
    return lightmap_impl("pt_bake_lightmap_device", c, width, height, d_texels6, prm, d_linear, d_rgba);
}

int pt_bake_lightmap_host(PtContext* c, uint32_t width, uint32_t height, const float* texels6, const PtRenderParams* prm, float* out_linear,
                          uint8_t* out_rgba) {
    const char* const who = "pt_bake_lightmap_host";
    if (int rc = check_lightmap(who, c, width, height, texels6, prm, out_linear, out_rgba, 4)) return rc;
    const size_t np = (size_t)width * height;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->bake_in.ensure(6 * np)) return rc;
    return render_staged(c, 3 * np, out_rgba ? 4 * np : 0, [&](float* d_linear, uint8_t* d_rgba) {
        HIP_TRY(hipStreamSynchronize(c->stream));      // (an earlier call may still read the staging)
        HIP_TRY(hipMemcpy(c->bake_in.p, texels6, 6 * np * sizeof(float), hipMemcpyHostToDevice));
        return lightmap_impl(who, c, width, height, c->bake_in.p, prm, d_linear, d_rgba);
    }, [&] { return copy_back({{out_linear, c->host_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np}}); });
}

int pt_bake_probes_device(PtContext* c, const float* d_positions3, uint32_t n_probes, uint32_t rays_per_probe, const PtRenderParams* prm,
                          float* d_radiance, float* d_sh27) {
    if (int rc = check_probes("pt_bake_probes_device", c, d_positions3, n_probes, rays_per_probe, prm, d_radiance, d_sh27)) return rc;
    return probes_impl("pt_bake_probes_device", c, d_positions3, n_probes, rays_per_probe, prm, d_radiance, d_sh27);
}

int pt_bake_probes_host(PtContext* c, const float* positions3, uint32_t n_probes, uint32_t rays_per_probe, const PtRenderParams* prm,
                        float* out_radiance, float* out_sh27) {
    const char* const who = "pt_bake_probes_host";
    if (int rc = check_probes(who, c, positions3, n_probes, rays_per_probe, prm, out_radiance, out_sh27)) return rc;
    const size_t np = (size_t)n_probes * rays_per_probe;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->bake_in.ensure(3 * (size_t)n_probes)) return rc;
    return render_staged(c, 3 * np, 0, [&](float* d_radiance, uint8_t*) {
        if (int rc = c->bake_sh.ensure(out_sh27 ? 27 * (size_t)n_probes : 0)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));      // (an earlier call may still read the staging)
        HIP_TRY(hipMemcpy(c->bake_in.p, positions3, 3 * (size_t)n_probes * sizeof(float), hipMemcpyHostToDevice));
        return probes_impl(who, c, c->bake_in.p, n_probes, rays_per_probe, prm, d_radiance, out_sh27 ? c->bake_sh.p : nullptr);
    }, [&] {
        return copy_back({{out_radiance, c->host_lin.p, 3 * np * sizeof(float)}, {out_sh27, c->bake_sh.p, 27 * (size_t)n_probes * sizeof(float)}});
    });
}

int pt_sh_project_device(PtContext* c, uint32_t n_probes, uint32_t rays_per_probe, const float* d_radiance, float* d_sh27) {
    const char* const who = "pt_sh_project_device";
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_film(who, ptbake::kProbe, rays_per_probe, n_probes)) || (rc = check_plane(who, "the radiance plane", d_radiance, 4)) ||
        (rc = check_plane(who, "sh27", d_sh27, 4)))
        return rc;
    HIP_TRY(hipSetDevice(c->device));
    ptk::launch_probe_sh(n_probes, rays_per_probe, d_radiance, d_sh27, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_sh_project_host(uint32_t n_probes, uint32_t rays_per_probe, const float* radiance, float* sh27) {
    const char* const who = "pt_sh_project_host";
    int rc;
    if ((rc = check_film(who, ptbake::kProbe, rays_per_probe, n_probes)) || (rc = check_plane(who, "the radiance plane", radiance, 4)) ||
        (rc = check_plane(who, "sh27", sh27, 4)))
        return rc;
    for (size_t p = 0; p < n_probes; ++p) ptbake::sh_project_probe(rays_per_probe, radiance + 3 * p * rays_per_probe, sh27 + 27 * p);
    return PT_OK;
}

int pt_sh_irradiance_host(const float* sh27, const float* normals3, uint32_t n, float* out_rgb) {
    if (!sh27 || (n && (!normals3 || !out_rgb))) return fail(PT_ERR_INVALID_ARG, "pt_sh_irradiance_host: null argument");
    for (size_t i = 0; i < n; ++i) ptbake::sh_irradiance(sh27, normals3 + 3 * i, out_rgb + 3 * i);
    return PT_OK;
}

int pt_bake_rays_host(uint32_t kind, uint32_t width, uint32_t height, const float* data, const uint32_t* xys, uint32_t n, float* out6) {
    const char* const who = "pt_bake_rays_host";
    int rc;
    if ((rc = check_film(who, kind, width, height))) return rc;
    if (!data || (n && (!xys || !out6))) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((rc = check_xys(who, width, height, xys, n))) return rc;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t x = xys[3 * i], y = xys[3 * i + 1], s = xys[3 * i + 2];
        float* o = out6 + 6 * i;
        if (kind == (uint32_t)ptbake::kTexel) {
            uint32_t w0, w1;
            ptflt::camera_words(x, y, s, &w0, &w1);
            float tp;
            ptbake::texel_ray<ptbake::Exact>(data + 6 * ((size_t)y * width + x), w0, w1, o, o + 3, &tp);
        } else {
            for (int k = 0; k < 3; ++k) o[k] = data[3 * (size_t)y + k];
            ptbake::probe_dir<ptbake::Exact>(x, width, o + 3);
        }
    }
    return PT_OK;
}

int pt_debug_bake_rays(PtContext* c, uint32_t kind, uint32_t width, uint32_t height, const float* data, const uint32_t* xys, uint32_t n,
                       uint32_t exact_math, float* out6) {
    const char* const who = "pt_debug_bake_rays";
    int rc;
    if ((rc = check_film(who, kind, width, height))) return rc;
    if (!c || !data || (n && (!xys || !out6))) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((rc = check_xys(who, width, height, xys, n))) return rc;
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nd = data_floats(kind, width, height);
    if ((rc = c->fn_in.ensure(nd + 2))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->fn_in.p, data, nd * sizeof(float), hipMemcpyHostToDevice));      // (hipMalloc's alignment: fine for 8-byte words)
    return debug_source_rays(c, bake_source(kind, width, height, c->fn_in.p), xys, n, exact_math, 6, out6);
}

}  // extern "C"
