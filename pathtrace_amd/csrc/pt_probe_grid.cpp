// pt_probe_grid.cpp -- the host side of the irradiance volume: the grid helpers, the bake of a grid (k_probe_positions in
// front of pt_bake_probes_device), the shading pass (k_probe_shade) alone and behind the feature pass, and the rule on the CPU
// (pt_probe_grid.h).  The shading passes take the moment maps of the probe visibility where they are given; the entries
// that give them stand in pt_probe_vis.cpp and share this file's checks and passes through pt_probe_entry.h.  The entries' rule,
// check_plane, the render's preconditions and the host entry's staging: pt_entry.h.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pt_probe_entry.h"
#include "pt_probe_vis.h"

namespace ptprobe {

static_assert(sizeof(PtProbeGrid) == sizeof(ptgrid::Grid) && offsetof(PtProbeGrid, spacing) == offsetof(ptgrid::Grid, spacing) &&
                  offsetof(PtProbeGrid, counts) == offsetof(ptgrid::Grid, counts),
              "ptgrid::Grid is PtProbeGrid");
static_assert((int)PT_PROBE_WEIGHT_TRILINEAR == (int)ptgrid::kTrilinear && (int)PT_PROBE_WEIGHT_FACING == (int)ptgrid::kFacing, "the weight modes");

ptgrid::Grid rule_grid(const PtProbeGrid* g) {
    ptgrid::Grid r;
    std::memcpy(&r, g, sizeof r);
    return r;
}

int check_grid(const char* who, const PtProbeGrid* g) {
    if (!g) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (pt_probe_grid_count(g) == 0u)
        return fail(PT_ERR_INVALID_ARG,
                    "%s: invalid probe grid %ux%ux%u: counts >= 1, at most 65535 probes, origin and spacing finite, spacing > 0 on an axis with "
                    "more than one probe",
                    who, g->counts[0], g->counts[1], g->counts[2]);
    return PT_OK;
}
int check_probe_count(const char* who, uint32_t n_probes) {
    if (n_probes == 0 || n_probes > ptgrid::kMaxProbes) return fail(PT_ERR_INVALID_ARG, "%s: n_probes must be in [1, 65535]", who);
    return PT_OK;
}
int check_rays_per_probe(const char* who, uint32_t rays_per_probe) {
    if (rays_per_probe == 0 || rays_per_probe > 65535u) return fail(PT_ERR_INVALID_ARG, "%s: rays_per_probe must be in [1, 65535]", who);
    return PT_OK;
}
// what a shading pass reads and writes, checked before anything looks at a context; feat_align: 16 on the device, 4 on the host
int check_shade(const char* who, const PtCamera* cam, const PtProbeGrid* g, const void* sh27, const void* features, const void* fallback,
                const PtProbeShade* sp, const void* out_linear, const void* out_rgba, uint32_t feat_align, bool own_features) {
    if (!cam || !sp) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_grid(who, g))) return rc;
    if (sp->weight >= (uint32_t)ptgrid::kWeights) return fail(PT_ERR_INVALID_ARG, "%s: unknown weight %u", who, sp->weight);
    if (!std::isfinite(sp->normal_bias)) return fail(PT_ERR_INVALID_ARG, "%s: normal_bias must be finite", who);
    if (cam->width == 0 || cam->height == 0) return fail(PT_ERR_INVALID_ARG, "%s: image %ux%u: a zero size", who, cam->width, cam->height);
    if ((rc = check_pixel_count(who, cam->width, cam->height)) || (rc = check_plane(who, "sh27", sh27, 4)) || (!own_features && (rc = check_plane(who, "the feature plane", features, feat_align))) ||
        (rc = check_plane(who, "the fallback plane", fallback, 4, true)) || (rc = check_plane(who, "the linear output", out_linear, 4)) ||
        (rc = check_plane(who, "the RGBA8 output", out_rgba, 4, true)))
        return rc;
    return PT_OK;
}

// the launch of a checked shading pass
int shade_launch(PtContext* c, const PtCamera* cam, const PtProbeGrid* g, const float* d_sh27, const float* d_features, const float* d_fallback,
                 const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba, const Maps& maps) {
    ptk::ProbeShadeArgs a{};
    a.feat = reinterpret_cast<const float4*>(d_features);
    a.sh27 = d_sh27; a.fallback = d_fallback; a.out_linear = d_out_linear; a.out_rgba = d_out_rgba;
    for (int k = 0; k < 3; ++k) {
        a.cam[k] = cam->origin[k]; a.cam[3 + k] = cam->lower_left[k]; a.cam[6 + k] = cam->horizontal[k]; a.cam[9 + k] = cam->vertical[k];
    }
    a.grid = rule_grid(g);
    a.width = cam->width; a.height = cam->height; a.weight = sp->weight; a.normal_bias = sp->normal_bias;
    if (maps.vis) ptk::launch_probe_shade_vis(a, maps.moments, maps.vis->resolution, c->stream);
    else ptk::launch_probe_shade(a, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// what pt_render_probe_lit_* checks of its own before the feature pass checks the rest
int check_probe_lit(const char* who, const PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtProbeGrid* g, const void* sh27,
                    const void* fallback, const PtProbeShade* sp, const void* out_linear, const void* out_rgba) {
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    return check_shade(who, cam, g, sh27, nullptr, fallback, sp, out_linear, out_rgba, 16, /*own_features=*/true);
}
int probe_lit_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g, const float* d_sh27,
                   const float* d_fallback, const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba, const Maps& maps) {
    int rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->pg_feat.ensure(2 * (size_t)cam->width * cam->height))) return rc;
    float* const feat = reinterpret_cast<float*>(c->pg_feat.p);
    if ((rc = pt_render_features_device(c, cam, prm, feature_samples, feat))) return rc;      // (refuses before its first launch)
    return shade_launch(c, cam, g, d_sh27, feat, d_fallback, sp, d_out_linear, d_out_rgba, maps);
}

// the rule on the CPU, with the maps or without
void shade_host(const PtCamera* cam, const PtProbeGrid* g, const float* sh27, const float* features, const float* fallback, const PtProbeShade* sp,
                float* out_linear, uint8_t* out_rgba, const Maps& maps) {
    const ptgrid::Grid r = rule_grid(g);
    const double camv[12] = {cam->origin[0],     cam->origin[1],     cam->origin[2],     cam->lower_left[0], cam->lower_left[1], cam->lower_left[2],
                             cam->horizontal[0], cam->horizontal[1], cam->horizontal[2], cam->vertical[0],   cam->vertical[1],   cam->vertical[2]};
    for (uint32_t y = 0; y < cam->height; ++y)
        for (uint32_t x = 0; x < cam->width; ++x) {
            const size_t p = (size_t)y * cam->width + x;
            float v[3];
            const bool lit = maps.vis ? ptvis::shade(r, sp->normal_bias, cam->width, cam->height, x, y, features + 8 * p, camv, sh27, maps.moments,
                                                     maps.vis->resolution, v)
                                      : ptgrid::shade(r, sp->normal_bias, sp->weight, cam->width, cam->height, x, y, features + 8 * p, camv, sh27, v);
            if (!lit)
                for (int k = 0; k < 3; ++k) v[k] = fallback ? fallback[3 * p + k] : 0.0f;
            for (int k = 0; k < 3; ++k) out_linear[3 * p + k] = v[k];
            if (out_rgba) {
                const uint32_t q8 = ptgrid::rgba8(v);
                std::memcpy(out_rgba + 4 * p, &q8, 4);
            }
        }
}

// pt_render_probe_lit_host, and with maps pt_render_probe_lit_visibility_host: the coefficients through bake_sh, the maps through
// pv_mom, the film through host_lin / host_rgba
int probe_lit_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g, const float* sh27,
                   const float* fallback, const PtProbeShade* sp, float* out_linear, uint8_t* out_rgba, const Maps& maps) {
    const size_t np = (size_t)cam->width * cam->height, n = pt_probe_grid_count(g), nsh = 27 * n;
    const size_t nm = maps.vis ? n * maps.vis->resolution * maps.vis->resolution : 0;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->bake_sh.ensure(nsh)) || (rc = c->pv_mom.ensure(nm))) return rc;
    return render_staged(c, 3 * np, out_rgba ? 4 * np : 0, [&](float* d_linear, uint8_t* d_rgba) {
        HIP_TRY(hipStreamSynchronize(c->stream));      // (an earlier call may still read the staging)
        HIP_TRY(hipMemcpy(c->bake_sh.p, sh27, nsh * sizeof(float), hipMemcpyHostToDevice));
        if (nm) HIP_TRY(hipMemcpy(c->pv_mom.p, maps.moments, nm * sizeof(float2), hipMemcpyHostToDevice));
        if (fallback) HIP_TRY(hipMemcpy(d_linear, fallback, 3 * np * sizeof(float), hipMemcpyHostToDevice));
        Maps dm = maps;
        if (nm) dm.moments = reinterpret_cast<const float*>(c->pv_mom.p);
        return probe_lit_impl(c, cam, prm, feature_samples, g, c->bake_sh.p, fallback ? d_linear : nullptr, sp, d_linear, d_rgba, dm);
    }, [&] { return copy_back({{out_linear, c->host_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np}}); });
}

}  // namespace ptprobe
using namespace ptprobe;

extern "C" {

void pt_default_probe_shade(PtProbeShade* out) {
    if (!out) return;
    out->normal_bias = 0.0f;
    out->weight = PT_PROBE_WEIGHT_TRILINEAR;
}

uint32_t pt_probe_grid_count(const PtProbeGrid* g) { return g ? ptgrid::count(rule_grid(g)) : 0u; }

int pt_probe_grid_positions_host(const PtProbeGrid* g, float* out_positions3) {
    const char* const who = "pt_probe_grid_positions_host";
    int rc;
    if ((rc = check_grid(who, g)) || (rc = check_plane(who, "out_positions3", out_positions3, 4))) return rc;
    const ptgrid::Grid r = rule_grid(g);
    const uint32_t n = ptgrid::count(r);
    for (uint32_t p = 0; p < n; ++p) ptgrid::position(r, p, out_positions3 + 3 * (size_t)p);
    return PT_OK;
}

int pt_probe_grid_bake_device(PtContext* c, const PtProbeGrid* g, uint32_t rays_per_probe, const PtRenderParams* prm, float* d_sh27) {
    const char* const who = "pt_probe_grid_bake_device";
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_grid(who, g)) || (rc = check_rays_per_probe(who, rays_per_probe)) || (rc = check_plane(who, "sh27", d_sh27, 4))) return rc;
    // what the probe bake would refuse behind the positions launch, by its own checks (band_count <= 1 from here on)
    if ((rc = check_whole_image(who, " bakes", "", prm, /*band_index_too=*/false)) || (rc = check_scene(c)) || (rc = check_spp(prm->spp)) ||
        (rc = check_integrator(prm->integrator)) || (rc = check_accel(prm->accel)) || (rc = check_band_index(prm->band_index, 1u)))
        return rc;
    const uint32_t n = pt_probe_grid_count(g);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->pg_pos.ensure(3 * (size_t)n)) || (rc = c->pg_rad.ensure(3 * (size_t)n * rays_per_probe))) return rc;
    // (a bake larger than max_paths_in_flight is refused by the bake itself, PT_ERR_UNSUPPORTED, behind this launch, which writes
    // the context's own plane and nothing else)
    ptk::launch_probe_positions(rule_grid(g), n, c->pg_pos.p, c->stream);
    HIP_TRY(hipGetLastError());
    return pt_bake_probes_device(c, c->pg_pos.p, n, rays_per_probe, prm, c->pg_rad.p, d_sh27);
}

int pt_probe_shade_device(PtContext* c, const PtCamera* cam, const PtProbeGrid* g, const float* d_sh27, const float* d_features,
                          const float* d_fallback, const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba) {
    const char* const who = "pt_probe_shade_device";
    if (int rc = check_shade(who, cam, g, d_sh27, d_features, d_fallback, sp, d_out_linear, d_out_rgba, 16)) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    return shade_launch(c, cam, g, d_sh27, d_features, d_fallback, sp, d_out_linear, d_out_rgba);
}

int pt_probe_shade_host(const PtCamera* cam, const PtProbeGrid* g, const float* sh27, const float* features, const float* fallback,
                        const PtProbeShade* sp, float* out_linear, uint8_t* out_rgba) {
    if (int rc = check_shade("pt_probe_shade_host", cam, g, sh27, features, fallback, sp, out_linear, out_rgba, 4)) return rc;
    shade_host(cam, g, sh27, features, fallback, sp, out_linear, out_rgba);
    return PT_OK;
}

int pt_render_probe_lit_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g,
                               const float* d_sh27, const float* d_fallback, const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba) {
    if (int rc = check_probe_lit("pt_render_probe_lit_device", c, cam, prm, g, d_sh27, d_fallback, sp, d_out_linear, d_out_rgba)) return rc;
    return probe_lit_impl(c, cam, prm, feature_samples, g, d_sh27, d_fallback, sp, d_out_linear, d_out_rgba);
}

int pt_render_probe_lit_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g,
                             const float* sh27, const float* fallback, const PtProbeShade* sp, float* out_linear, uint8_t* out_rgba) {
    if (int rc = check_probe_lit("pt_render_probe_lit_host", c, cam, prm, g, sh27, fallback, sp, out_linear, out_rgba)) return rc;
    return probe_lit_host(c, cam, prm, feature_samples, g, sh27, fallback, sp, out_linear, out_rgba);
}

int pt_debug_probe_positions(PtContext* c, const PtProbeGrid* g, float* out_positions3) {
    const char* const who = "pt_debug_probe_positions";
    int rc;
    if ((rc = check_grid(who, g)) || (rc = check_plane(who, "out_positions3", out_positions3, 4))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    const uint32_t n = pt_probe_grid_count(g);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->pg_pos.ensure(3 * (size_t)n))) return rc;
    ptk::launch_probe_positions(rule_grid(g), n, c->pg_pos.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_positions3, c->pg_pos.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
