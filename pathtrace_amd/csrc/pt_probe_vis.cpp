// pt_probe_vis.cpp -- the host side of the irradiance volume's probe visibility: the distances of the probe rays (the
// bake's feature-ray form in front of the first-hit pass, k_probe_distances), the moment maps (k_probe_moments), the entries that hand
// the maps to the shading passes of pt_probe_grid.cpp (pt_probe_entry.h), and the rule on the CPU (pt_probe_vis.h).  The entries'
// rule, check_plane, the render's preconditions and copy_back: pt_entry.h.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pt_probe_entry.h"
#include "pt_probe_update.h"      // ptupd::stage_ray; pt_probe_vis.h

using namespace ptprobe;

static_assert(sizeof(PtProbeVisibility) == sizeof(ptvis::Params) && offsetof(PtProbeVisibility, max_distance) == offsetof(ptvis::Params, max_distance) &&
                  offsetof(PtProbeVisibility, sharpness_log2) == offsetof(ptvis::Params, sharpness_log2),
              "ptvis::Params is PtProbeVisibility");

namespace ptprobe {

ptvis::Params rule_visibility(const PtProbeVisibility* vis) {
    ptvis::Params r{};
    if (vis) std::memcpy(&r, vis, sizeof r);
    return r;
}

int check_moments_plane(const char* who, const PtProbeVisibility* vis, const void* moments, bool device) {
    if (!vis) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (vis->resolution < ptvis::kMinResolution || vis->resolution > ptvis::kMaxResolution)
        return fail(PT_ERR_INVALID_ARG, "%s: resolution %u not in [%u, %u]", who, vis->resolution, ptvis::kMinResolution, ptvis::kMaxResolution);
    if (vis->sharpness_log2 > ptvis::kMaxSharpness)
        return fail(PT_ERR_INVALID_ARG, "%s: sharpness_log2 %u (at most %u)", who, vis->sharpness_log2, ptvis::kMaxSharpness);
    if (!(vis->max_distance > 0.0f) || !std::isfinite(vis->max_distance)) return fail(PT_ERR_INVALID_ARG, "%s: max_distance must be finite and > 0", who);
    return check_plane(who, "the moments plane", moments, device ? 8 : 4);
}

// The distances of n_rows x R probe rays into d_out, everything checked: per chunk of whole rows the source's feature-ray form
// (source(ctx, base, nb): the film of the rows base .. base + nb - 1), the first-hit pass of the feature entries, k_probe_distances.
// No path kernel.
int distances_of(PtContext* c, uint32_t n_rows, uint32_t R, const PtRenderParams* prm, float* d_out, RowSource source, const void* ctx) {
    int rc;
    uint32_t accel = prm->accel;
    if (accel == PT_ACCEL_AUTO) {
        const std::string keep = g_err;
        accel = (c->auto_bvh && c->tree.may_build() && ensure_bvh(c) == PT_OK) ? PT_ACCEL_BVH : PT_ACCEL_LINEAR;
        if (!accel) g_err = keep;
    }
    if (accel && (rc = ensure_bvh(c))) return rc;
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_rows, kFeatureRays / R));
    const size_t n_rays = (size_t)chunk * R;
    if ((rc = c->ft_rays.ensure(6 * n_rays)) || (rc = c->ft_ids.ensure(n_rays)) || (rc = c->ft_t.ensure(n_rays)) ||
        (accel && (rc = c->ft_scratch.ensure(3 * n_rays))))
        return rc;
    const ptk::SceneView sv = view_for(c, prm->exact_math);
    const hipStream_t st = c->stream;
    const float t_min = (float)prm->t_min, t_max = INFINITY;
    for (uint32_t base = 0; base < n_rows; base += chunk) {
        const uint32_t nb = std::min(chunk, n_rows - base), n = nb * R;
        if (!ptk::launch_source_feature_rays(prm->exact_math, source(ctx, base, nb), 0u, 1u, c->ft_rays.p, st))
            return fail(PT_ERR_INVALID_ARG, "the ray source has no feature-ray kernel");
        if (prm->exact_math) ptk::launch_debug_hit_exact(sv, accel, c->ft_rays.p, n, t_min, t_max, c->ft_scratch.p, c->ft_ids.p, c->ft_t.p, nullptr, st);
        else ptk::launch_debug_hit_fast(sv, accel, c->ft_rays.p, n, t_min, t_max, c->ft_scratch.p, c->ft_ids.p, c->ft_t.p, nullptr, st);
        ptk::launch_probe_distances(c->ft_ids.p, c->ft_t.p, n, d_out + (size_t)base * R, st);
        HIP_TRY(hipGetLastError());
    }
    return PT_OK;
}

}  // namespace ptprobe

namespace {

// the distances of the bake's rays from given positions
struct BakeRows { const float* d_positions3; uint32_t R; };
ptk::RaySourceF bake_rows(const void* ctx, uint32_t base, uint32_t nb) {
    const BakeRows* b = static_cast<const BakeRows*>(ctx);
    return bake_source(ptbake::kProbe, b->R, nb, b->d_positions3 + 3 * (size_t)base);
}
int distances_impl(PtContext* c, const float* d_positions3, uint32_t n_probes, uint32_t R, const PtRenderParams* prm, float* d_out) {
    const BakeRows rows{d_positions3, R};
    return distances_of(c, n_probes, R, prm, d_out, bake_rows, &rows);
}
int check_distances(const char* who, const PtContext* c, const void* positions3, uint32_t n_probes, uint32_t R, const PtRenderParams* prm, const void* out) {
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_probe_count(who, n_probes)) || (rc = check_rays_per_probe(who, R)) || (rc = check_plane(who, "positions3", positions3, 4)) ||
        (rc = check_plane(who, "the distances output", out, 4)) || (rc = check_accel(prm->accel)) || (rc = check_scene(c)))
        return rc;
    return PT_OK;
}
void moments_launch(PtContext* c, const float* d_distances, uint32_t n_probes, uint32_t R, const PtProbeVisibility* vis, float* d_moments) {
    ptk::ProbeMomentsArgs a{};
    a.distances = d_distances; a.moments = d_moments; a.n_probes = n_probes; a.rays_per_probe = R;
    a.vis = rule_visibility(vis);
    ptk::launch_probe_moments(a, c->stream);
}

}  // namespace

extern "C" {

void pt_default_probe_visibility(const PtProbeGrid* g, PtProbeVisibility* out) {
    if (!out) return;
    out->resolution = 8u; out->sharpness_log2 = 5u; out->max_distance = 1.0f; out->reserved = 0u;
    if (pt_probe_grid_count(g) == 0u) return;
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a)
        if (g->counts[a] > 1u) d2 += g->spacing[a] * g->spacing[a];
    const float m = (float)(1.5 * std::sqrt(d2));
    if (m > 0.0f && std::isfinite(m)) out->max_distance = m;
}

int pt_probe_distances_device(PtContext* c, const float* d_positions3, uint32_t n_probes, uint32_t rays_per_probe, const PtRenderParams* prm,
                              float* d_distances) {
    if (int rc = check_distances("pt_probe_distances_device", c, d_positions3, n_probes, rays_per_probe, prm, d_distances)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return distances_impl(c, d_positions3, n_probes, rays_per_probe, prm, d_distances);
}

int pt_probe_distances_host(PtContext* c, const float* positions3, uint32_t n_probes, uint32_t rays_per_probe, const PtRenderParams* prm,
                            float* out_distances) {
    if (int rc = check_distances("pt_probe_distances_host", c, positions3, n_probes, rays_per_probe, prm, out_distances)) return rc;
    const size_t n = (size_t)n_probes * rays_per_probe;
    int rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->bake_in.ensure(3 * (size_t)n_probes)) || (rc = c->pv_out.ensure(n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // (an earlier call may still read the staging)
    HIP_TRY(hipMemcpy(c->bake_in.p, positions3, 3 * (size_t)n_probes * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = distances_impl(c, c->bake_in.p, n_probes, rays_per_probe, prm, c->pv_out.p)) || (rc = pt_sync(c))) return rc;
    return copy_back({{out_distances, c->pv_out.p, n * sizeof(float)}});
}

int pt_probe_moments_device(PtContext* c, const float* d_distances, uint32_t n_probes, uint32_t rays_per_probe, const PtProbeVisibility* vis,
                            float* d_moments) {
    const char* const who = "pt_probe_moments_device";
    int rc;
    if ((rc = check_moments_plane(who, vis, d_moments, true)) || (rc = check_probe_count(who, n_probes)) ||
        (rc = check_rays_per_probe(who, rays_per_probe)) || (rc = check_plane(who, "the distances plane", d_distances, 4)))
        return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    moments_launch(c, d_distances, n_probes, rays_per_probe, vis, d_moments);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_probe_moments_host(const float* distances, uint32_t n_probes, uint32_t rays_per_probe, const PtProbeVisibility* vis, float* out_moments) {
    const char* const who = "pt_probe_moments_host";
    int rc;
    if ((rc = check_moments_plane(who, vis, out_moments, false)) || (rc = check_probe_count(who, n_probes)) ||
        (rc = check_rays_per_probe(who, rays_per_probe)) || (rc = check_plane(who, "the distances plane", distances, 4)))
        return rc;
    const ptvis::Params v = rule_visibility(vis);
    const uint32_t R = rays_per_probe;
    const size_t tt = (size_t)v.resolution * v.resolution;
    const float identity[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    std::vector<double> rays(4 * (size_t)R);
    for (size_t p = 0; p < n_probes; ++p) {
        for (uint32_t r = 0; r < R; ++r) ptupd::stage_ray(r, R, identity, true, true, distances[p * R + r], v.max_distance, &rays[4 * (size_t)r]);
        ptvis::probe_moments(v, R, rays.data(), out_moments + 2 * tt * p);
    }
    return PT_OK;
}

int pt_probe_grid_visibility_device(PtContext* c, const PtProbeGrid* g, uint32_t rays_per_probe, const PtRenderParams* prm,
                                    const PtProbeVisibility* vis, float* d_moments) {
    const char* const who = "pt_probe_grid_visibility_device";
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_grid(who, g)) || (rc = check_moments_plane(who, vis, d_moments, true)) || (rc = check_rays_per_probe(who, rays_per_probe)) ||
        (rc = check_accel(prm->accel)) || (rc = check_scene(c)))
        return rc;
    const uint32_t n = pt_probe_grid_count(g);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->pg_pos.ensure(3 * (size_t)n)) || (rc = c->pv_dist.ensure((size_t)n * rays_per_probe))) return rc;
    ptk::launch_probe_positions(rule_grid(g), n, c->pg_pos.p, c->stream);
    HIP_TRY(hipGetLastError());
    if ((rc = distances_impl(c, c->pg_pos.p, n, rays_per_probe, prm, c->pv_dist.p))) return rc;
    moments_launch(c, c->pv_dist.p, n, rays_per_probe, vis, d_moments);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_probe_shade_visibility_device(PtContext* c, const PtCamera* cam, const PtProbeGrid* g, const float* d_sh27, const float* d_moments,
                                     const PtProbeVisibility* vis, const float* d_features, const float* d_fallback, const PtProbeShade* sp,
                                     float* d_out_linear, uint8_t* d_out_rgba) {
    const char* const who = "pt_probe_shade_visibility_device";
    int rc;
    if ((rc = check_shade(who, cam, g, d_sh27, d_features, d_fallback, sp, d_out_linear, d_out_rgba, 16)) || (rc = check_moments_plane(who, vis, d_moments, true)))
        return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    return shade_launch(c, cam, g, d_sh27, d_features, d_fallback, sp, d_out_linear, d_out_rgba, Maps{d_moments, vis});
}

int pt_probe_shade_visibility_host(const PtCamera* cam, const PtProbeGrid* g, const float* sh27, const float* moments, const PtProbeVisibility* vis,
                                   const float* features, const float* fallback, const PtProbeShade* sp, float* out_linear, uint8_t* out_rgba) {
    const char* const who = "pt_probe_shade_visibility_host";
    int rc;
    if ((rc = check_shade(who, cam, g, sh27, features, fallback, sp, out_linear, out_rgba, 4)) || (rc = check_moments_plane(who, vis, moments, false))) return rc;
    shade_host(cam, g, sh27, features, fallback, sp, out_linear, out_rgba, Maps{moments, vis});
    return PT_OK;
}

int pt_render_probe_lit_visibility_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g,
                                          const float* d_sh27, const float* d_moments, const PtProbeVisibility* vis, const float* d_fallback,
                                          const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba) {
    const char* const who = "pt_render_probe_lit_visibility_device";
    int rc;
    if ((rc = check_probe_lit(who, c, cam, prm, g, d_sh27, d_fallback, sp, d_out_linear, d_out_rgba)) || (rc = check_moments_plane(who, vis, d_moments, true))) return rc;
    return probe_lit_impl(c, cam, prm, feature_samples, g, d_sh27, d_fallback, sp, d_out_linear, d_out_rgba, Maps{d_moments, vis});
}

int pt_render_probe_lit_visibility_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g,
                                        const float* sh27, const float* moments, const PtProbeVisibility* vis, const float* fallback,
                                        const PtProbeShade* sp, float* out_linear, uint8_t* out_rgba) {
    const char* const who = "pt_render_probe_lit_visibility_host";
    int rc;
    if ((rc = check_probe_lit(who, c, cam, prm, g, sh27, fallback, sp, out_linear, out_rgba)) || (rc = check_moments_plane(who, vis, moments, false))) return rc;
    return probe_lit_host(c, cam, prm, feature_samples, g, sh27, fallback, sp, out_linear, out_rgba, Maps{moments, vis});
}

}  // extern "C"
