// pt_probe_update.cpp -- the host side of the irradiance volume's updates over frames: the update as a ray source of
// the injected-path driver (render_injected_impl, pt_api.cpp) and of the distance pass (distances_of, pt_probe_vis.cpp), the launch
// that follows them (k_probe_update), the rule on the CPU (pt_probe_update.h), the rotation of a frame and the debug entry.  The
// entries' rule, check_plane and the render's preconditions: pt_entry.h.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pt_probe_entry.h"
#include "pt_probe_update.h"

using namespace ptprobe;

namespace {

static_assert(sizeof(PtProbeUpdate) == sizeof(ptupd::Params) && offsetof(PtProbeUpdate, rotation) == offsetof(ptupd::Params, rotation) &&
                  offsetof(PtProbeUpdate, hysteresis) == offsetof(ptupd::Params, hysteresis) &&
                  offsetof(PtProbeUpdate, change_alpha) == offsetof(ptupd::Params, change_alpha),
              "ptupd::Params is PtProbeUpdate");
// the public update struct as the rule and the kernels take it: the one conversion
ptupd::Params rule_update(const PtProbeUpdate* u) {
    ptupd::Params r;
    std::memcpy(&r, u, sizeof r);
    return r;
}

// the parameters of an update of n_probes probes; the first rule broken answers
int check_update(const char* who, const PtProbeUpdate* u, uint32_t n_probes) {
    if (!u) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (int rc = check_rays_per_probe(who, u->rays_per_probe)) return rc;
    if (u->stride == 0) return fail(PT_ERR_INVALID_ARG, "%s: stride must be >= 1", who);
    if (u->first >= n_probes) return fail(PT_ERR_INVALID_ARG, "%s: first %u is not below the %u probes", who, u->first, n_probes);
    if (!std::isfinite(u->hysteresis) || u->hysteresis < 0.0f || !(u->hysteresis < 1.0f))
        return fail(PT_ERR_INVALID_ARG, "%s: hysteresis must be in [0, 1)", who);
    if (!std::isfinite(u->change_threshold) || u->change_threshold < 0.0f)
        return fail(PT_ERR_INVALID_ARG, "%s: change_threshold must be finite and >= 0", who);
    if (!std::isfinite(u->change_alpha) || u->change_alpha < 0.0f || u->change_alpha > 1.0f)
        return fail(PT_ERR_INVALID_ARG, "%s: change_alpha must be in [0, 1]", who);
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(u->rotation[k])) return fail(PT_ERR_INVALID_ARG, "%s: the rotation must be finite", who);
    double err, det;
    ptupd::orthonormality(u->rotation, &err, &det);
    if (!(err <= 1e-5) || !(det > 0.0))
        return fail(PT_ERR_INVALID_ARG, "%s: the rotation must be orthonormal to 1e-5 (max |M M^T - I| = %g) with a positive determinant (%g)", who, err,
                    det);
    return PT_OK;
}
// what a blend reads and writes
int check_blend(const char* who, uint32_t n_probes, const PtProbeUpdate* u, const PtProbeVisibility* vis, const void* radiance, const void* distances,
                const void* sh27, const void* moments, const void* age, bool device) {
    int rc;
    if ((rc = check_probe_count(who, n_probes)) || (rc = check_update(who, u, n_probes))) return rc;
    if (vis) {
        if ((rc = check_moments_plane(who, vis, moments, device)) || (rc = check_plane(who, "the distances plane", distances, 4))) return rc;
    } else if (distances) {
        return fail(PT_ERR_INVALID_ARG, "%s: a distances plane without a visibility struct", who);
    }
    if ((rc = check_plane(who, "the radiance plane", radiance, 4)) || (rc = check_plane(who, "sh27", sh27, 4)) ||
        (rc = check_plane(who, "the age plane", age, 4)))
        return rc;
    return PT_OK;
}

// a camera for the film's geometry only (no camera ray is generated): directions x slots
PtCamera film_camera(uint32_t width, uint32_t height) {
    PtCamera cam{};
    cam.lower_left[0] = cam.lower_left[1] = cam.lower_left[2] = -1.0;
    cam.horizontal[0] = 2.0; cam.vertical[1] = 2.0;
    cam.width = width; cam.height = height;
    return cam;
}
// the update as a ray source: the film of the n slots from slot `base` on
ptk::RaySourceF update_source(const PtProbeGrid* g, const PtProbeUpdate* u, uint32_t base, uint32_t n) {
    const PtCamera cam = film_camera(u->rays_per_probe, n);
    ptk::RaySourceF s{};
    s.tag = ptk::kSrcProbeUpdate;
    s.cam = camera_f32(&cam);
    s.upd.grid = rule_grid(g);
    s.upd.rule = rule_update(u);
    s.upd.rule.first = u->first + base * u->stride;
    return s;
}
// update_source as distances_of takes it
struct SlotSource { const PtProbeGrid* g; const PtProbeUpdate* u; };
ptk::RaySourceF slot_source(const void* ctx, uint32_t base, uint32_t nb) {
    const SlotSource* s = static_cast<const SlotSource*>(ctx);
    return update_source(s->g, s->u, base, nb);
}
// xys = n x (direction, slot, sample) inside the film
int check_xys(const char* who, uint32_t width, uint32_t height, const uint32_t* xys, uint32_t n) {
    for (size_t i = 0; i < n; ++i)
        if (xys[3 * i] >= width || xys[3 * i + 1] >= height)
            return fail(PT_ERR_INVALID_ARG, "%s: position (%u, %u) of entry %zu lies outside the %ux%u film", who, xys[3 * i], xys[3 * i + 1], i, width,
                        height);
    return PT_OK;
}
int check_rays(const char* who, const PtProbeGrid* g, const PtProbeUpdate* u, const uint32_t* xys, uint32_t n, const float* out6) {
    int rc;
    if ((rc = check_grid(who, g)) || (rc = check_update(who, u, pt_probe_grid_count(g)))) return rc;
    if (n && (!xys || !out6)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    return check_xys(who, u->rays_per_probe, ptupd::slots(pt_probe_grid_count(g), u->first, u->stride), xys, n);
}

void blend_launch(PtContext* c, uint32_t n_probes, const PtProbeUpdate* u, const PtProbeVisibility* vis, const float* d_radiance,
                  const float* d_distances, float* d_sh27, float* d_moments, uint32_t* d_age) {
    ptk::ProbeUpdateArgs a{};
    a.radiance = d_radiance; a.distances = vis ? d_distances : nullptr; a.sh27 = d_sh27; a.moments = vis ? d_moments : nullptr; a.age = d_age;
    a.n_probes = n_probes;
    a.vis = rule_visibility(vis);
    a.u = rule_update(u);
    ptk::launch_probe_update(a, ptupd::slots(n_probes, u->first, u->stride), c->stream);
}

// one slot on the CPU, in the kernel's order: rad = the slot's float[R][3], dist = its float[R]; sh27, moments (float[T][T][2]) and
// age are the probe's own, in place
void update_probe(const ptupd::Params& u, const ptvis::Params* vis, const float* rad, const float* dist, float* sh27, float* moments, uint32_t* age) {
    const uint32_t R = u.rays_per_probe, old_age = *age;
    const bool id = ptupd::is_identity(u.rotation);
    std::vector<double> rays(4 * (size_t)R);
    for (uint32_t r = 0; r < R; ++r) ptupd::stage_ray(r, R, u.rotation, id, vis != nullptr, vis ? dist[r] : 0.0f, vis ? vis->max_distance : 0.0f, &rays[4 * (size_t)r]);
    float new_sh[27], new_moments[2 * ptvis::kMaxResolution * ptvis::kMaxResolution];
    ptupd::sh_project_staged(R, rays.data(), rad, new_sh);
    const uint32_t n_moments = vis ? 2u * vis->resolution * vis->resolution : 0u;
    if (vis) ptvis::probe_moments(*vis, R, rays.data(), new_moments);
    const double a = ptupd::alpha(u, old_age, sh27, new_sh);
    for (int k = 0; k < 27; ++k) sh27[k] = ptupd::blend(sh27[k], new_sh[k], a, old_age);
    for (uint32_t k = 0; k < n_moments; ++k) moments[k] = ptupd::blend(moments[k], new_moments[k], a, old_age);
    *age = ptupd::next_age(old_age);
}

// what pt_probe_grid_update_* checks, all of it before anything of the context is touched; device: the moments plane is 8-byte aligned
int check_grid_update(const char* who, const PtContext* c, const PtProbeGrid* g, const PtRenderParams* prm, const PtProbeVisibility* vis,
                      const PtProbeUpdate* u, const void* sh27, const void* moments, const void* age, bool device) {
    if (!c || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_grid(who, g))) return rc;
    if ((rc = check_update(who, u, pt_probe_grid_count(g))) || (vis && (rc = check_moments_plane(who, vis, moments, device))) ||
        (rc = check_plane(who, "sh27", sh27, 4)) || (rc = check_plane(who, "the age plane", age, 4)))
        return rc;
    // what the render of the slots would refuse, by its own checks
    if ((rc = check_whole_image(who, " updates", "", prm, /*band_index_too=*/false)) || (rc = check_scene(c)) || (rc = check_spp(prm->spp)) ||
        (rc = check_integrator(prm->integrator)) || (rc = check_accel(prm->accel)) || (rc = check_band_index(prm->band_index, 1u)))
        return rc;
    return PT_OK;
}
// the update on device planes, everything checked, the device set
int grid_update_impl(const char* who, PtContext* c, const PtProbeGrid* g, const PtRenderParams* prm, const PtProbeVisibility* vis, const PtProbeUpdate* u,
                     float* d_sh27, float* d_moments, uint32_t* d_age) {
    int rc;
    const uint32_t n = pt_probe_grid_count(g), R = u->rays_per_probe, n_upd = ptupd::slots(n, u->first, u->stride);
    if ((rc = c->pu_rad.ensure(3 * (size_t)n_upd * R)) || (vis && (rc = c->pu_dist.ensure((size_t)n_upd * R)))) return rc;
    // (a film larger than max_paths_in_flight is refused by the driver, PT_ERR_UNSUPPORTED, before its first launch)
    const PtCamera cam = film_camera(R, n_upd);
    if ((rc = render_injected_impl(who, c, &cam, prm, update_source(g, u, 0u, n_upd), c->pu_rad.p, nullptr, /*no_camera=*/true))) return rc;
    const SlotSource src{g, u};
    if (vis && (rc = distances_of(c, n_upd, R, prm, c->pu_dist.p, slot_source, &src))) return rc;
    blend_launch(c, n, u, vis, c->pu_rad.p, c->pu_dist.p, d_sh27, d_moments, d_age);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

}  // namespace

extern "C" {

void pt_probe_rotation(uint32_t frame, float* out9) {
    if (!out9) return;
    for (int k = 0; k < 9; ++k) out9[k] = (k % 4 == 0) ? 1.0f : 0.0f;
    if (frame == 0u) return;
    const uint32_t c[3] = {0x9E3779B9u, 0x85EBCA6Bu, 0xC2B2AE35u};
    double u[3];
    for (int i = 0; i < 3; ++i) u[i] = (double)((frame * c[i]) >> 8) * (1.0 / 16777216.0);
    const double two_pi = 2.0 * ptbake::kPi;
    const double a = std::sqrt(1.0 - u[0]), b = std::sqrt(u[0]);
    const double x = a * std::sin(two_pi * u[1]), y = a * std::cos(two_pi * u[1]), z = b * std::sin(two_pi * u[2]), w = b * std::cos(two_pi * u[2]);
    const double m[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w),       2.0 * (x * z + y * w),
                         2.0 * (x * y + z * w),       1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                         2.0 * (x * z - y * w),       2.0 * (y * z + x * w),       1.0 - 2.0 * (x * x + y * y)};
    for (int k = 0; k < 9; ++k) out9[k] = (float)m[k];
}

void pt_default_probe_update(uint32_t frame, uint32_t stride, PtProbeUpdate* out) {
    if (!out) return;
    const uint32_t s = stride ? stride : 1u;
    out->rays_per_probe = 64u;
    out->first = frame % s; out->stride = s;
    out->hysteresis = 0.9375f;
    out->change_threshold = 0.0f; out->change_alpha = 1.0f;
    pt_probe_rotation(frame, out->rotation);
    out->reserved = 0u;
}

int pt_probe_update_rays_host(const PtProbeGrid* g, const PtProbeUpdate* u, const uint32_t* xys, uint32_t n, float* out6) {
    const char* const who = "pt_probe_update_rays_host";
    if (int rc = check_rays(who, g, u, xys, n, out6)) return rc;
    const ptgrid::Grid r = rule_grid(g);
    const bool id = ptupd::is_identity(u->rotation);
    for (size_t i = 0; i < n; ++i) {
        float* o = out6 + 6 * i;
        ptgrid::position(r, u->first + xys[3 * i + 1] * u->stride, o);
        ptupd::dir<ptbake::Exact>(xys[3 * i], u->rays_per_probe, u->rotation, id, o + 3);
    }
    return PT_OK;
}

int pt_debug_probe_update_rays(PtContext* c, const PtProbeGrid* g, const PtProbeUpdate* u, const uint32_t* xys, uint32_t n, uint32_t exact_math,
                               float* out6) {
    const char* const who = "pt_debug_probe_update_rays";
    if (int rc = check_rays(who, g, u, xys, n, out6)) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    return debug_source_rays(c, update_source(g, u, 0u, ptupd::slots(pt_probe_grid_count(g), u->first, u->stride)), xys, n, exact_math, 6, out6);
}

int pt_probe_blend_device(PtContext* c, uint32_t n_probes, const PtProbeUpdate* u, const PtProbeVisibility* vis, const float* d_radiance,
                          const float* d_distances, float* d_sh27, float* d_moments, uint32_t* d_age) {
    const char* const who = "pt_probe_blend_device";
    if (int rc = check_blend(who, n_probes, u, vis, d_radiance, d_distances, d_sh27, d_moments, d_age, true)) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    blend_launch(c, n_probes, u, vis, d_radiance, d_distances, d_sh27, d_moments, d_age);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_probe_blend_host(uint32_t n_probes, const PtProbeUpdate* u, const PtProbeVisibility* vis, const float* radiance, const float* distances,
                        float* sh27, float* moments, uint32_t* age) {
    const char* const who = "pt_probe_blend_host";
    if (int rc = check_blend(who, n_probes, u, vis, radiance, distances, sh27, moments, age, false)) return rc;
    const ptupd::Params r = rule_update(u);
    const ptvis::Params vp = rule_visibility(vis);
    const uint32_t R = r.rays_per_probe, n_upd = ptupd::slots(n_probes, r.first, r.stride);
    const size_t tt = vis ? (size_t)vis->resolution * vis->resolution : 0;
    for (uint32_t k = 0; k < n_upd; ++k) {
        const size_t p = r.first + (size_t)k * r.stride;
        update_probe(r, vis ? &vp : nullptr, radiance + 3 * (size_t)k * R, vis ? distances + (size_t)k * R : nullptr, sh27 + 27 * p,
                     vis ? moments + 2 * tt * p : nullptr, age + p);
    }
    return PT_OK;
}

int pt_probe_grid_update_device(PtContext* c, const PtProbeGrid* g, const PtRenderParams* prm, const PtProbeVisibility* vis, const PtProbeUpdate* u,
                                float* d_sh27, float* d_moments, uint32_t* d_age) {
    const char* const who = "pt_probe_grid_update_device";
    if (int rc = check_grid_update(who, c, g, prm, vis, u, d_sh27, d_moments, d_age, true)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return grid_update_impl(who, c, g, prm, vis, u, d_sh27, d_moments, d_age);
}

int pt_probe_grid_update_host(PtContext* c, const PtProbeGrid* g, const PtRenderParams* prm, const PtProbeVisibility* vis, const PtProbeUpdate* u,
                              float* sh27, float* moments, uint32_t* age) {
    const char* const who = "pt_probe_grid_update_host";
    int rc;
    if ((rc = check_grid_update(who, c, g, prm, vis, u, sh27, moments, age, false))) return rc;
    const size_t n = pt_probe_grid_count(g), nsh = 27 * n, nm = vis ? n * vis->resolution * vis->resolution : 0;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->bake_sh.ensure(nsh)) || (rc = c->pv_mom.ensure(nm)) || (rc = c->pu_age.ensure(n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // (an earlier call may still read the staging)
    HIP_TRY(hipMemcpy(c->bake_sh.p, sh27, nsh * sizeof(float), hipMemcpyHostToDevice));
    if (nm) HIP_TRY(hipMemcpy(c->pv_mom.p, moments, nm * sizeof(float2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->pu_age.p, age, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((rc = grid_update_impl(who, c, g, prm, vis, u, c->bake_sh.p, reinterpret_cast<float*>(c->pv_mom.p), c->pu_age.p)) || (rc = pt_sync(c))) return rc;
    return copy_back({{sh27, c->bake_sh.p, nsh * sizeof(float)}, {nm ? moments : nullptr, c->pv_mom.p, nm * sizeof(float2)}, {age, c->pu_age.p, n * sizeof(uint32_t)}});
}

}  // extern "C"
