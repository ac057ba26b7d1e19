// pt_denoise.cpp -- the host side of the denoisers.  Device entries: the first-hit feature and id passes, the a-trous filter (its
// own or a given variance plane), the adaptive pass's variance plane, temporal accumulation (plain, following moving objects through
// pt_motion.h, with a per-pixel weight) and the gradients (pt_gradient.h) that make that weight.  Host entries: pt_render_*denoised*.
// The entries' rule, the checks shared with the other entries, the render's preconditions and copy_back: pt_entry.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_entry.h"
#include "pt_gradient.h"
#include "pt_motion.h"

namespace {

enum class History { none, plain, motion, alpha };   // the accumulation before the a-trous steps; motion reads d_ids, alpha d_alpha too
enum class Variance { spatial, given };              // the filter's initial variance: its own 3 x 3 estimate, or the plane d_var
enum class Strata { same_camera, prev_camera };      // the camera whose frame the gradient strata re-trace

int check_denoise(const char* who, const PtDenoise* dn) {   // (a check answers in the entry's name, who, with the first rule broken)
    if (dn->iterations > 16) return fail(PT_ERR_INVALID_ARG, "%s: %u iterations (at most 16)", who, dn->iterations);
    if (!(dn->sigma_l >= 0.0f) || !(dn->sigma_n >= 0.0f) || !(dn->sigma_d >= 0.0f) || !std::isfinite(dn->sigma_l) ||
        !std::isfinite(dn->sigma_n) || !std::isfinite(dn->sigma_d))
        return fail(PT_ERR_INVALID_ARG, "%s: sigma_l, sigma_n and sigma_d must be finite and >= 0", who);
    return PT_OK;
}

int check_weight(const char* who, const char* name, float alpha) {   // PtTemporal.alpha, or the gradient entries' alpha_min
    if (!(alpha >= 0.0f && alpha <= 1.0f)) return fail(PT_ERR_INVALID_ARG, "%s: %s %g not in [0, 1]", who, name, alpha);
    return PT_OK;
}

int check_gradient(const char* who, const PtGradient* g) {
    if (g->radius > ptgr::kMaxRadius) return fail(PT_ERR_INVALID_ARG, "%s: radius %u (at most %u)", who, g->radius, ptgr::kMaxRadius);
    if (!(g->scale >= 0.0f) || !std::isfinite(g->scale)) return fail(PT_ERR_INVALID_ARG, "%s: scale must be finite and >= 0", who);
    return PT_OK;
}

struct Film { const float* linear; const float* features; float* out_linear; uint8_t* out_rgba; };   // what a filter entry reads and writes
int check_film_aligned(const char* who, const Film& f) {
    if ((uintptr_t)f.features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if ((uintptr_t)f.linear % 4u || (uintptr_t)f.out_linear % 4u || (uintptr_t)f.out_rgba % 4u)
        return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    return PT_OK;
}

int check_film_size(const char* who, uint32_t width, uint32_t height, const Film& f) {
    if (f.out_linear == f.linear) return fail(PT_ERR_INVALID_ARG, "%s: the output must not be the input", who);
    return check_pixel_count(who, width, height);
}

int check_target(const char* who, const PtContext* c, const PtCamera* cam) {   // what render_impl would refuse, by its own checks
    int rc;
    if ((rc = check_scene(c)) || (rc = check_camera_size(cam))) return rc;
    return check_pixel_count(who, cam->width, cam->height);
}

bool same_camera(const PtCamera& a, const PtCamera& b) {   // the four vectors, field by field (the sizes are the caller's to compare)
    for (int k = 0; k < 3; ++k)
        if (a.origin[k] != b.origin[k] || a.lower_left[k] != b.lower_left[k] || a.horizontal[k] != b.horizontal[k] || a.vertical[k] != b.vertical[k])
            return false;
    return true;
}

void set_cameras(ptk::TemporalArgs& t, const PtCamera& cur, const PtCamera& prev) {
    for (int k = 0; k < 3; ++k) {
        t.cur[k] = cur.origin[k]; t.cur[3 + k] = cur.lower_left[k]; t.cur[6 + k] = cur.horizontal[k]; t.cur[9 + k] = cur.vertical[k];
        t.prev[k] = prev.origin[k]; t.prev[3 + k] = prev.lower_left[k]; t.prev[6 + k] = prev.horizontal[k]; t.prev[9 + k] = prev.vertical[k];
    }
    t.same_camera = same_camera(cur, prev);
}

// The arguments of the launch that fills plane 0 with (u, var); denoise_steps completes them per iteration.
ptk::DenoiseArgs denoise_args(const PtContext* c, uint32_t width, uint32_t height, const Film& f, const PtDenoise* dn) {
    ptk::DenoiseArgs a{};
    a.linear = f.linear; a.feat = reinterpret_cast<const float4*>(f.features);
    a.out_linear = f.out_linear; a.out_rgba = f.out_rgba;
    a.width = width; a.height = height;
    a.sigma_l = dn->sigma_l; a.sigma_n = dn->sigma_n; a.sigma_d = dn->sigma_d;
    a.dst = c->dn_plane[0].p; a.finalize = dn->iterations == 0;
    return a;
}

// The front of a pt_render_denoised* frame: staging for np pixels, then the render into host_lin, the features into dn_feat and, from
// History::motion on, the ids into dn_ids.  History::alpha (the gradient entries): gr_alpha too, and no previous frame from here on.
int features_impl(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm, uint32_t n_samples,
                  float* d_features, int32_t* d_ids);
int frame_front(History form, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, size_t np, PtRenderParams* p,
                const FrameSource& src = {}) {
    int rc;
    if ((rc = c->host_lin.ensure(3 * np)) || (rc = c->host_rgba.ensure(4 * np)) || (rc = c->dn_feat.ensure(2 * np)) || (rc = c->dn_lin.ensure(3 * np)) ||
        (form >= History::motion && (rc = c->dn_ids.ensure(np))) || (form == History::alpha && (rc = c->gr_alpha.ensure(np))))
        return rc;
    if (form == History::alpha) c->gr_valid = false;
    *p = *prm;                                // for the whole image
    p->band_count = 1; p->band_index = 0; p->band_rows = 0;
    // pt_render_lens_denoised, pt_render_projection_denoised: both passes through the source (History::none only)
    const char* const who = src.lens ? "pt_render_lens_denoised" : src.proj ? "pt_render_projection_denoised" : nullptr;
    if ((rc = who ? render_source_impl(who, c, cam, src, p, c->host_lin.p, nullptr) : render_impl(c, cam, p, FilmState{}, nullptr, c->host_lin.p, nullptr)) ||
        (rc = features_impl(who ? who : "pt_render_features_device", c, cam, src, p, std::min(feature_samples, p->spp),
                            reinterpret_cast<float*>(c->dn_feat.p), nullptr)))
        return rc;
    return form >= History::motion ? pt_render_feature_ids_device(c, cam, p, c->dn_ids.p) : PT_OK;
}

// First-hit features: per batch of samples, k_source_feature_rays writes the rays, launch_debug_hit (the scan or BVH of the
// parity entries) finds their hits, k_feature_resolve adds the records to the per-pixel sums in d_features.
// pt_render_feature_ids_device is the same pass over the one sample spp_offset without the resolve: the hit ids of that batch,
// copied out of the scratch (d_features null, d_ids set).  src (pt_render_features_lens_device, pt_render_features_projection_device):
// the source whose feature-ray form writes the rays; empty: the pinhole camera's.
int features_impl(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm, uint32_t n_samples,
                  float* d_features, int32_t* d_ids) {
    if (!c || !cam || !prm || (!d_features && !d_ids)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (n_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: n_samples must be > 0", who);
    int rc;
    ptk::RaySourceF sf;
    if ((rc = source_setup(who, cam, src, &sf))) return rc;
    if ((rc = check_whole_image(who, ": works on", "", prm))) return rc;
    if ((uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if ((uintptr_t)d_ids % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_ids must be 4-byte aligned", who);
    if ((rc = check_accel(prm->accel)) || (rc = check_target(who, c, cam))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t accel = prm->accel;
    if (accel == PT_ACCEL_AUTO) {
        const std::string keep = g_err;
        accel = (c->auto_bvh && c->tree.may_build() && ensure_bvh(c) == PT_OK) ? PT_ACCEL_BVH : PT_ACCEL_LINEAR;
        if (!accel) g_err = keep;
    }
    if (accel && (rc = ensure_bvh(c))) return rc;
    const uint32_t nb_max = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_samples, kFeatureRays / np));
    const size_t n_rays = (size_t)nb_max * np;
    if ((rc = c->ft_rays.ensure(6 * n_rays)) || (rc = c->ft_ids.ensure(n_rays)) || (rc = c->ft_t.ensure(n_rays)) || (rc = c->ft_rec.ensure(8 * n_rays)) ||
        (accel && (rc = c->ft_scratch.ensure(3 * n_rays))))
        return rc;
    const ptk::SceneView sv = view_for(c, prm->exact_math);
    const hipStream_t st = c->stream;
    const float t_min = (float)prm->t_min, t_max = INFINITY;
    for (uint32_t done = 0; done < n_samples;) {
        const uint32_t nb = std::min(nb_max, n_samples - done);
        const uint32_t s_base = prm->spp_offset + done;
        ptk::FeatureResolveArgs a{};
        a.mat = sv.mat; a.ids = c->ft_ids.p; a.rec = c->ft_rec.p; a.out = reinterpret_cast<float4*>(d_features);
        a.np = np; a.nb = nb; a.n_samples = n_samples; a.load = done > 0; a.finalize = done + nb == n_samples;
        if (!ptk::launch_source_feature_rays(prm->exact_math, sf, s_base, nb, c->ft_rays.p, st))
            return fail(PT_ERR_INVALID_ARG, "%s: ray source %u has no feature-ray kernel", who, sf.tag);
        if (prm->exact_math) ptk::launch_debug_hit_exact(sv, accel, c->ft_rays.p, nb * np, t_min, t_max, c->ft_scratch.p, c->ft_ids.p, c->ft_t.p, c->ft_rec.p, st);
        else ptk::launch_debug_hit_fast(sv, accel, c->ft_rays.p, nb * np, t_min, t_max, c->ft_scratch.p, c->ft_ids.p, c->ft_t.p, c->ft_rec.p, st);
        if (d_features) ptk::launch_feature_resolve(prm->exact_math, a, st);
        HIP_TRY(hipGetLastError());
        if (d_ids && done == 0) HIP_TRY(hipMemcpyAsync(d_ids, c->ft_ids.p, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToDevice, st));   // sample spp_offset
        done += nb;
    }
    return PT_OK;
}

// The a-trous iterations of pt_denoise_device and pt_denoise_temporal_device: (u, var) waits in plane 0; one k_denoise_step
// per iteration between the two planes, the last launch writes the film planes.
int denoise_steps(PtContext* c, ptk::DenoiseArgs a, uint32_t iterations) {
    for (uint32_t i = 0; i < iterations; ++i) {
        a.src = c->dn_plane[i & 1u].p; a.dst = c->dn_plane[(i + 1u) & 1u].p;
        a.step = 1u << i; a.finalize = i + 1u == iterations;
        ptk::launch_denoise(a, false, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return PT_OK;
}

// pt_render_denoised (History::none), pt_render_denoised_temporal (plain: tp) and pt_render_denoised_motion (motion: tp, the
// ids pass): render, features, filter; host buffers, blocking
int render_denoised_impl(const char* who, History form, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                         const PtDenoise* dn, const PtTemporal* tp, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                         float* out_features, int32_t* out_ids, const FrameSource& src = {}) {
    if (!c || !cam || !prm || !dn || (form != History::none && !tp) || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    ptk::RaySourceF checked;
    if ((rc = source_setup(who, cam, src, &checked))) return rc;
    if ((rc = check_whole_image(who, ": renders", "", prm))) return rc;
    if (feature_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: feature_samples must be > 0", who);
    if ((rc = check_target(who, c, cam))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    HIP_TRY(hipSetDevice(c->device));
    PtRenderParams p;
    if ((rc = frame_front(form, c, cam, prm, feature_samples, np, &p, src))) return rc;
    float* const feat = reinterpret_cast<float*>(c->dn_feat.p);
    uint8_t* const rgba = out_rgba ? c->host_rgba.p : nullptr;
    if ((rc = form == History::motion  ? pt_denoise_temporal_motion_device(c, cam, c->host_lin.p, feat, c->dn_ids.p, dn, tp, c->dn_lin.p, rgba)
              : form == History::plain ? pt_denoise_temporal_device(c, cam, c->host_lin.p, feat, dn, tp, c->dn_lin.p, rgba)
                                       : pt_denoise_device(c, cam->width, cam->height, c->host_lin.p, feat, dn, c->dn_lin.p, rgba)) ||
        (rc = pt_sync(c)))
        return rc;
    return copy_back({{out_linear, c->dn_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                      {out_noisy, c->host_lin.p, 3 * np * sizeof(float)}, {out_features, feat, 8 * np * sizeof(float)},
                      {out_ids, c->dn_ids.p, np * sizeof(int32_t)}});
}

// The maps current pose -> history pose of every object into c->mo_maps, on the context's stream.  Unchanged poses since the
// last call: the buffer already holds them.
int upload_motion_maps(PtContext* c) {
    const uint32_t n = c->view.n_objs;
    int rc;
    if ((rc = c->mo_maps.ensure((size_t)n + 1))) return rc;
    const bool hist = c->tm_valid && c->tm_pose.size() == c->pose.size();     // no history: every pixel is fresh anyway
    const uint64_t key[2] = {c->pose_gen, hist ? c->tm_pose_gen : ~0ull};
    if (key[0] == c->mo_key[0] && key[1] == c->mo_key[1]) return PT_OK;
    // (the copy below reads the staging vector when the stream reaches it: the copy that last read this vector must be through;
    // the stream's order keeps the kernels that read the device maps ahead of the copy that replaces them)
    const uint32_t slot = c->mo_slot ^= 1u;
    if (!c->mo_staged[slot]) HIP_TRY(c->mo_staged[slot].create(false));
    else HIP_TRY(hipEventSynchronize(c->mo_staged[slot]));
    std::vector<ptk::MotionMap>& h_maps = c->h_maps[slot];
    h_maps.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        ptk::MotionMap& m = h_maps[i];
        const double* cur = &c->pose[9 * (size_t)i];
        double out[12];
        m.flags = ptmo::motion_map(c->h_shape_tag[i] == PT_SHAPE_TRIANGLE, cur, hist ? &c->tm_pose[9 * (size_t)i] : cur, out);
        m.pad = 0;
        std::memcpy(m.a, out, 9 * sizeof(double)); std::memcpy(m.b, out + 9, 3 * sizeof(double));
    }
    if (n) HIP_TRY(hipMemcpyAsync(c->mo_maps.p, h_maps.data(), (size_t)n * sizeof(ptk::MotionMap), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->mo_staged[slot], c->stream));
    c->mo_key[0] = key[0]; c->mo_key[1] = key[1];
    return PT_OK;
}

// Temporal accumulation: k_denoise_temporal (history -> (u, var) in plane 0 and the next history), then the a-trous steps of
// pt_denoise_device.  The arguments are checked before the context is looked at.  History::motion and History::alpha read
// the ids and the motion maps, alpha its per-pixel plane as well.  All store a history frame, and with it the scene's pose
// becomes the history pose.
int temporal_impl(const char* who, History form, PtContext* c, const PtCamera* cam, const Film& f, const int32_t* d_ids, const float* d_alpha,
                  const PtDenoise* dn, const PtTemporal* tp) {
    const bool motion = form != History::plain;
    if (!cam || !dn || !tp || !f.linear || !f.features || !f.out_linear || (motion && !d_ids) || (form == History::alpha && !d_alpha))
        return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_camera_size(cam, who)) || (rc = check_denoise(who, dn)) || (rc = check_weight(who, "alpha", tp->alpha))) return rc;
    if (!(tp->depth_tol >= 0.0f) || !(tp->normal_tol >= 0.0f) || !std::isfinite(tp->depth_tol) || !std::isfinite(tp->normal_tol))
        return fail(PT_ERR_INVALID_ARG, "%s: depth_tol and normal_tol must be finite and >= 0", who);
    if ((rc = check_film_aligned(who, f)) || (rc = check_film_size(who, cam->width, cam->height, f))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    if ((uintptr_t)d_ids % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_ids must be 4-byte aligned", who);
    if ((uintptr_t)d_alpha % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_alpha must be 4-byte aligned", who);
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    if (motion && (rc = check_scene(c, who))) return rc;
    if (motion && c->view.n_objs > (1u << 24) - 2u)
        return fail(PT_ERR_UNSUPPORTED, "%s: %u objects (an id + 1 must be exact in the history's f32 lane: at most 2^24 - 2)", who, c->view.n_objs);
    HIP_TRY(hipSetDevice(c->device));
    if (motion && (rc = upload_motion_maps(c))) return rc;
    if ((rc = c->dn_plane[0].ensure(np)) || (rc = c->dn_plane[1].ensure(np)) || (rc = c->tm_hist[0].ensure(3 * np)) ||
        (rc = c->tm_hist[1].ensure(3 * np)))
        return rc;
    const bool have = c->tm_valid && c->tm_cam.width == cam->width && c->tm_cam.height == cam->height;
    ptk::TemporalAlphaArgs a{};                // the three kernels' arguments, one inside the other: each launch takes its own part
    ptk::TemporalArgs& t = a.m.t;
    t.dn = denoise_args(c, cam->width, cam->height, f, dn);
    t.hist_src = have ? c->tm_hist[c->tm_cur].p : nullptr;
    t.hist_dst = c->tm_hist[c->tm_cur ^ 1u].p;
    set_cameras(t, *cam, c->tm_cam);
    t.same_camera = have && t.same_camera;
    t.alpha = tp->alpha; t.depth_tol = tp->depth_tol; t.normal_tol = tp->normal_tol;
    if (motion) { a.m.ids = d_ids; a.m.maps = c->mo_maps.p; a.m.n_objs = c->view.n_objs; a.alpha = d_alpha; }
    if (form == History::alpha) ptk::launch_denoise_temporal_alpha(a, c->stream);
    else if (form == History::motion) ptk::launch_denoise_temporal_motion(a.m, c->stream);
    else ptk::launch_denoise_temporal(t, c->stream);
    HIP_TRY(hipGetLastError());
    c->tm_cur ^= 1u; c->tm_valid = true; c->tm_cam = *cam;
    if (!c->has_scene) c->tm_pose.clear();
    else if (c->tm_pose_gen != c->pose_gen || c->tm_pose.size() != c->pose.size()) c->tm_pose = c->pose;
    c->tm_pose_gen = c->pose_gen;
    return denoise_steps(c, t.dn, dn->iterations);
}

// The filter of pt_denoise_device and pt_denoise_var_device (Variance::given: k_denoise_init_var and the caller's variance
// plane in place of k_denoise_init): (u, var) into plane 0, then one k_denoise_step per iteration between the two planes; the
// last launch writes the film planes.
int denoise_impl(const char* who, Variance form, PtContext* c, uint32_t width, uint32_t height, const Film& f, const float* d_var,
                 const PtDenoise* dn) {
    if (!c || !dn || !f.linear || !f.features || !f.out_linear || (form == Variance::given && !d_var))
        return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARG, "%s: image %ux%u", who, width, height);
    int rc;
    if ((rc = check_denoise(who, dn)) || (rc = check_film_aligned(who, f))) return rc;
    if ((uintptr_t)d_var % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_var must be 4-byte aligned", who);
    if ((rc = check_film_size(who, width, height, f))) return rc;
    const size_t np = (size_t)width * height;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->dn_plane[0].ensure(np)) || (rc = c->dn_plane[1].ensure(np))) return rc;
    const ptk::DenoiseArgs a = denoise_args(c, width, height, f, dn);
    if (form == Variance::given) ptk::launch_denoise_init_var(a, d_var, c->stream);
    else ptk::launch_denoise(a, true, c->stream);
    HIP_TRY(hipGetLastError());
    return denoise_steps(c, a, dn->iterations);
}

// The strata's pixel list (k_gradient_list), its render with the previous frame's parameters in the current scene (a list
// render that may take the regenerating kernel, as pt_render_adaptive's passes do), the records and the plane.  The
// arguments are checked before the context is looked at, and everything the list render checks is checked before the first
// launch: a refused call leaves the context as it was.
//
// Strata::prev_camera (pt_temporal_gradient_camera_device): the strata lie in the image of prev_cam, whose
// re-trace this is, and k_gradient_alpha_camera looks every pixel of cam up in them through d_features.
int gradient_impl(const char* who, Strata form, PtContext* c, const PtCamera* cam, const PtCamera* prev_cam, const PtRenderParams* prev,
                  uint32_t seed, const float* d_prev, const float* d_features, const PtGradient* g, float alpha_min, float* d_alpha) {
    const bool moved = form == Strata::prev_camera;
    if (!cam || !prev || !d_prev || !g || !d_alpha || (moved && (!prev_cam || !d_features)))
        return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((uintptr_t)d_prev % 4u || (uintptr_t)d_alpha % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_prev_linear and d_alpha must be 4-byte aligned", who);
    if (moved && (uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if (moved && (prev_cam->width != cam->width || prev_cam->height != cam->height))
        return fail(PT_ERR_INVALID_ARG, "%s: the previous camera is %ux%u, the camera %ux%u", who, prev_cam->width, prev_cam->height,
                    cam->width, cam->height);
    int rc;
    if ((rc = check_whole_image(who, ": works on", "", prev)) || (rc = check_gradient(who, g)) || (rc = check_weight(who, "alpha_min", alpha_min)) ||
        (rc = check_camera_size(cam, who)) || (rc = check_spp(prev->spp, who)) || (rc = check_integrator(prev->integrator, who)) ||
        (rc = check_accel(prev->accel, who)) || (rc = check_pixel_count(who, cam->width, cam->height)))
        return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    if ((rc = check_scene(c, who))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t ns = (size_t)ptgr::strata(cam->width) * ptgr::strata(cam->height);
    if ((rc = c->gr_list.ensure(ns)) || (rc = c->gr_film.ensure(3 * ns)) || (rc = c->gr_rec.ensure(2 * ns))) return rc;
    ptk::GradientArgs a{};
    a.retraced = c->gr_film.p; a.prev = d_prev; a.list = c->gr_list.p; a.rec = c->gr_rec.p; a.alpha = d_alpha;
    a.width = cam->width; a.height = cam->height; a.seed = seed; a.radius = g->radius;
    a.scale = g->scale; a.alpha_min = alpha_min;
    ptk::launch_gradient_list(a, c->stream);
    HIP_TRY(hipGetLastError());
    PtRenderParams p = *prev;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    ListRender lr;
    lr.d_pixels = c->gr_list.p; lr.n = (uint32_t)ns; lr.regen = true;
    if ((rc = render_impl(c, moved ? prev_cam : cam, &p, FilmState{}, &lr, c->gr_film.p, nullptr))) return rc;
    ptk::launch_gradient_strata(a, c->stream);
    if (moved) {
        ptk::TemporalArgs t{};
        t.dn.feat = reinterpret_cast<const float4*>(d_features);
        t.dn.width = cam->width; t.dn.height = cam->height;
        set_cameras(t, *cam, *prev_cam);
        ptk::launch_gradient_alpha_camera(a, t, c->stream);
    } else {
        ptk::launch_gradient_alpha(a, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// pt_render_denoised_motion with the alpha plane between the ids pass and the accumulation, and the frame's noisy film kept
// for the next call.  Strata::prev_camera (pt_render_denoised_gradient_camera): the previous frame stays usable when the
// camera moved, and the plane is pt_temporal_gradient_camera_device's.
int render_gradient_impl(const char* who, Strata form, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                         const PtDenoise* dn, const PtTemporal* tp, const PtGradient* g, float* out_linear, uint8_t* out_rgba,
                         float* out_noisy, float* out_features, int32_t* out_ids, float* out_alpha) {
    if (!c || !cam || !prm || !dn || !tp || !g || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_whole_image(who, ": renders", "", prm))) return rc;
    if (feature_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: feature_samples must be > 0", who);
    if ((rc = check_gradient(who, g)) || (rc = check_weight(who, "alpha", tp->alpha)) || (rc = check_target(who, c, cam))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    HIP_TRY(hipSetDevice(c->device));
    // the previous frame is usable: one of the two entries completed it, at this size, through this camera (prev_camera:
    // through any), and the history it went into is there
    const bool usable = c->gr_valid && c->tm_valid && c->gr_prev.cap >= 3 * np && c->gr_cam.width == cam->width &&
                        c->gr_cam.height == cam->height && (form == Strata::prev_camera || same_camera(c->gr_cam, *cam));
    const PtCamera prev_cam = c->gr_cam;
    PtRenderParams p;
    if ((rc = frame_front(History::alpha, c, cam, prm, feature_samples, np, &p))) return rc;
    float* const feat = reinterpret_cast<float*>(c->dn_feat.p);
    uint8_t* const rgba = out_rgba ? c->host_rgba.p : nullptr;
    if (!usable) HIP_TRY(hipMemsetAsync(c->gr_alpha.p, 0xFF, np * sizeof(float), c->stream));      // every entry a NaN: no measurement
    else if ((rc = form == Strata::prev_camera
                       ? pt_temporal_gradient_camera_device(c, cam, &prev_cam, &c->gr_params, c->gr_frame, c->gr_prev.p, feat, g, tp->alpha, c->gr_alpha.p)
                       : pt_temporal_gradient_device(c, cam, &c->gr_params, c->gr_frame, c->gr_prev.p, g, tp->alpha, c->gr_alpha.p)))
        return rc;
    if ((rc = pt_denoise_temporal_alpha_device(c, cam, c->host_lin.p, feat, c->dn_ids.p, c->gr_alpha.p, dn, tp, c->dn_lin.p, rgba)) ||
        (rc = c->gr_prev.ensure(3 * np)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->gr_prev.p, c->host_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = pt_sync(c))) return rc;
    c->gr_valid = true; c->gr_params = p; c->gr_cam = *cam; ++c->gr_frame;
    return copy_back({{out_linear, c->dn_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                      {out_noisy, c->host_lin.p, 3 * np * sizeof(float)}, {out_features, feat, 8 * np * sizeof(float)},
                      {out_ids, c->dn_ids.p, np * sizeof(int32_t)}, {out_alpha, c->gr_alpha.p, np * sizeof(float)}});
}

}  // namespace

// For pt_render_denoised_upsampled (pt_upsample.cpp): what pt_render_denoised does on the device for cam -- its checks in the
// name who, the frame front, the filter from host_lin into dn_lin under the features in dn_feat -- without the wait and the
// copies.  *p: the parameters of the whole image, for the passes the caller adds.
int denoised_frame_device(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                          const PtDenoise* dn, PtRenderParams* p) {
    if (!c || !cam || !prm || !dn) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_whole_image(who, ": renders", "", prm))) return rc;
    if (feature_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: feature_samples must be > 0", who);
    if ((rc = check_denoise(who, dn)) || (rc = check_target(who, c, cam))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = frame_front(History::none, c, cam, prm, feature_samples, (size_t)cam->width * cam->height, p))) return rc;
    return pt_denoise_device(c, cam->width, cam->height, c->host_lin.p, reinterpret_cast<float*>(c->dn_feat.p), dn, c->dn_lin.p, nullptr);
}

// The lens and projection forms of pt_render_features_device and pt_render_denoised (their entries: pt_lens.cpp, pt_projection.cpp)
int features_source_device(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm,
                           uint32_t n_samples, float* d_features) {
    return features_impl(who, c, cam, src, prm, n_samples, d_features, nullptr);
}
int render_source_denoised_host(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm,
                                uint32_t feature_samples, const PtDenoise* dn, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                float* out_features) {
    return render_denoised_impl(who, History::none, c, cam, prm, feature_samples, dn, nullptr, out_linear, out_rgba, out_noisy, out_features,
                                nullptr, src);
}

extern "C" {

int pt_render_features_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t n_samples, float* d_features) {
    return features_impl("pt_render_features_device", c, cam, {}, prm, n_samples, d_features, nullptr);
}

int pt_render_feature_ids_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, int32_t* d_ids) {
    return features_impl("pt_render_feature_ids_device", c, cam, {}, prm, 1, nullptr, d_ids);
}

int pt_denoise_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const float* d_features,
                      const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba) {
    return denoise_impl("pt_denoise_device", Variance::spatial, c, width, height, {d_linear, d_features, d_out_linear, d_out_rgba}, nullptr, dn);
}

int pt_denoise_var_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const float* d_features,
                          const float* d_var, const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba) {
    return denoise_impl("pt_denoise_var_device", Variance::given, c, width, height, {d_linear, d_features, d_out_linear, d_out_rgba}, d_var, dn);
}

// k_adaptive_variance over the state the last completed pt_render_adaptive left in the context
int pt_adaptive_variance_device(PtContext* c, uint32_t width, uint32_t height, const float* d_features, float* d_var) {
    if (!c || !d_features || !d_var) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_variance_device: null argument");
    if ((uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_variance_device: d_features must be 16-byte aligned");
    if ((uintptr_t)d_var % 4u) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_variance_device: d_var must be 4-byte aligned");
    if (!c->ad_valid) return fail(PT_ERR_INVALID_ARG, "pt_adaptive_variance_device: the context holds no completed pt_render_adaptive");
    if (width != c->ad_width || height != c->ad_height)
        return fail(PT_ERR_INVALID_ARG, "pt_adaptive_variance_device: image %ux%u, the last pt_render_adaptive was %ux%u", width, height,
                    c->ad_width, c->ad_height);
    HIP_TRY(hipSetDevice(c->device));
    ptk::launch_adaptive_variance(c->ad_sums.p, c->ad_count.p, reinterpret_cast<const float4*>(d_features), width * height, d_var, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// pt_render_adaptive's passes (the film stays in host_lin), the feature pass, the variance plane, the filter; host buffers, blocking
int pt_render_adaptive_denoised(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtAdaptive* ad, uint32_t feature_samples,
                                const PtDenoise* dn, float* out_linear, uint8_t* out_rgba, float* out_noisy, uint32_t* out_spp,
                                float* out_rel_err, float* out_var) {
    if (!c || !cam || !prm || !ad || !dn || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive_denoised: null argument");
    if (feature_samples == 0) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive_denoised: feature_samples must be > 0");
    int rc;
    if ((rc = render_adaptive_impl(c, cam, prm, ad))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    if ((rc = c->dn_feat.ensure(2 * np)) || (rc = c->dn_lin.ensure(3 * np)) || (rc = c->dn_var.ensure(np))) return rc;
    PtRenderParams p = *prm;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    float* const feat = reinterpret_cast<float*>(c->dn_feat.p);
    uint8_t* const rgba = out_rgba ? c->host_rgba.p : nullptr;
    if ((rc = pt_render_features_device(c, cam, &p, std::min(feature_samples, ad->spp_min), feat)) ||
        (rc = pt_adaptive_variance_device(c, cam->width, cam->height, feat, c->dn_var.p)) ||
        (rc = pt_denoise_var_device(c, cam->width, cam->height, c->host_lin.p, feat, c->dn_var.p, dn, c->dn_lin.p, rgba)) ||
        (rc = pt_sync(c)))
        return rc;
    return copy_back({{out_linear, c->dn_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                      {out_noisy, c->host_lin.p, 3 * np * sizeof(float)}, {out_spp, c->ad_count.p, np * sizeof(uint32_t)},
                      {out_rel_err, c->ad_err.p, np * sizeof(float)}, {out_var, c->dn_var.p, np * sizeof(float)}});
}

int pt_render_denoised(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtDenoise* dn,
                       float* out_linear, uint8_t* out_rgba, float* out_noisy, float* out_features) {
    return render_denoised_impl("pt_render_denoised", History::none, c, cam, prm, feature_samples, dn, nullptr, out_linear, out_rgba,
                                out_noisy, out_features, nullptr);
}

int pt_temporal_reset(PtContext* c) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_temporal_reset: null context");
    c->tm_valid = false;
    c->gr_valid = false; c->gr_frame = 0;
    return PT_OK;
}

int pt_denoise_temporal_device(PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features,
                               const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear, uint8_t* d_out_rgba) {
    return temporal_impl("pt_denoise_temporal_device", History::plain, c, cam, {d_linear, d_features, d_out_linear, d_out_rgba}, nullptr, nullptr, dn, tp);
}

int pt_denoise_temporal_motion_device(PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features, const int32_t* d_ids,
                                      const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear, uint8_t* d_out_rgba) {
    return temporal_impl("pt_denoise_temporal_motion_device", History::motion, c, cam, {d_linear, d_features, d_out_linear, d_out_rgba}, d_ids, nullptr,
                         dn, tp);
}

int pt_render_denoised_motion(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtDenoise* dn,
                              const PtTemporal* tp, float* out_linear, uint8_t* out_rgba, float* out_noisy, float* out_features,
                              int32_t* out_ids) {
    return render_denoised_impl("pt_render_denoised_motion", History::motion, c, cam, prm, feature_samples, dn, tp, out_linear, out_rgba,
                                out_noisy, out_features, out_ids);
}

int pt_denoise_temporal_alpha_device(PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features, const int32_t* d_ids,
                                     const float* d_alpha, const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear,
                                     uint8_t* d_out_rgba) {
    return temporal_impl("pt_denoise_temporal_alpha_device", History::alpha, c, cam, {d_linear, d_features, d_out_linear, d_out_rgba}, d_ids, d_alpha,
                         dn, tp);
}

void pt_default_gradient(PtGradient* out) {
    if (!out) return;
    out->radius = 1;
    out->scale = 1.0f;
}

int pt_temporal_gradient_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prev, uint32_t seed, const float* d_prev,
                                const PtGradient* g, float alpha_min, float* d_alpha) {
    return gradient_impl("pt_temporal_gradient_device", Strata::same_camera, c, cam, nullptr, prev, seed, d_prev, nullptr, g, alpha_min, d_alpha);
}

int pt_temporal_gradient_camera_device(PtContext* c, const PtCamera* cam, const PtCamera* prev_cam, const PtRenderParams* prev, uint32_t seed,
                                       const float* d_prev, const float* d_features, const PtGradient* g, float alpha_min, float* d_alpha) {
    return gradient_impl("pt_temporal_gradient_camera_device", Strata::prev_camera, c, cam, prev_cam, prev, seed, d_prev, d_features, g, alpha_min,
                         d_alpha);
}

// Debug: the strata of the last pt_temporal_gradient_device on this context copied back (blocking): per stratum its gradient
// pixel, its re-traced film and its record.
int pt_debug_gradient_strata(PtContext* c, uint32_t width, uint32_t height, uint32_t* out_xy, float* out_film, double* out_rec) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_debug_gradient_strata: null context");
    const size_t ns = (size_t)ptgr::strata(width) * ptgr::strata(height);
    if (ns == 0 || c->gr_list.cap < ns || c->gr_film.cap < 3 * ns || c->gr_rec.cap < 2 * ns)
        return fail(PT_ERR_INVALID_ARG, "pt_debug_gradient_strata: the context holds no strata of a %ux%u image", width, height);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return copy_back({{out_xy, c->gr_list.p, ns * sizeof(uint2)}, {out_film, c->gr_film.p, 3 * ns * sizeof(float)},
                      {out_rec, c->gr_rec.p, 2 * ns * sizeof(double)}});
}

int pt_render_denoised_gradient(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtDenoise* dn,
                                const PtTemporal* tp, const PtGradient* g, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                float* out_features, int32_t* out_ids, float* out_alpha) {
    return render_gradient_impl("pt_render_denoised_gradient", Strata::same_camera, c, cam, prm, feature_samples, dn, tp, g, out_linear, out_rgba,
                                out_noisy, out_features, out_ids, out_alpha);
}

int pt_render_denoised_gradient_camera(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                                       const PtDenoise* dn, const PtTemporal* tp, const PtGradient* g, float* out_linear, uint8_t* out_rgba,
                                       float* out_noisy, float* out_features, int32_t* out_ids, float* out_alpha) {
    return render_gradient_impl("pt_render_denoised_gradient_camera", Strata::prev_camera, c, cam, prm, feature_samples, dn, tp, g, out_linear,
                                out_rgba, out_noisy, out_features, out_ids, out_alpha);
}

int pt_render_denoised_temporal(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                                const PtDenoise* dn, const PtTemporal* tp, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                float* out_features) {
    return render_denoised_impl("pt_render_denoised_temporal", History::plain, c, cam, prm, feature_samples, dn, tp, out_linear, out_rgba,
                                out_noisy, out_features, nullptr);
}

}  // extern "C"
