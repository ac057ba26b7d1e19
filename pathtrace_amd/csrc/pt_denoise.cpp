// pt_denoise.cpp -- the first-hit feature pass and the denoisers: a-trous (with its own or the adaptive pass's variance),
// temporal accumulation with camera reprojection, and the motion form that follows moving objects (pt_motion.h); device
// entries and the host entries that render first.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_context.h"
#include "pt_gradient.h"
#include "pt_motion.h"

namespace {

constexpr uint64_t kFeatureRays = 1ull << 21;    // pt_render_features_device: rays per batch (108 B of scratch each with the BVH)

// First-hit features: per batch of samples, k_feature_rays writes the camera rays, launch_debug_hit (the scan or BVH of the
// parity entries) finds their hits, k_feature_resolve adds the records to the per-pixel sums in d_features.
// pt_render_feature_ids_device is the same pass over the one sample spp_offset without the resolve: the hit ids of that batch,
// copied out of the scratch (d_features null, d_ids set).
int features_impl(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t n_samples, float* d_features,
                  int32_t* d_ids) {
    if (!c || !cam || !prm || (!d_features && !d_ids)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (n_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: n_samples must be > 0", who);
    if ((prm->band_count ? prm->band_count : 1) != 1 || prm->band_index != 0)
        return fail(PT_ERR_INVALID_ARG, "%s: works on the whole image (band_count = 1)", who);
    if ((uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if ((uintptr_t)d_ids % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_ids must be 4-byte aligned", who);
    if (prm->accel > PT_ACCEL_AUTO) return fail(PT_ERR_INVALID_ARG, "unknown accel %u", prm->accel);
    if (!c->has_scene) return fail(PT_ERR_INVALID_ARG, "render: no scene uploaded");
    if (cam->width < 2 || cam->height < 2) return fail(PT_ERR_INVALID_ARG, "camera %ux%u: width and height must be >= 2", cam->width, cam->height);
    const uint64_t np64 = (uint64_t)cam->width * cam->height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)np64);
    const uint32_t np = (uint32_t)np64;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t accel = prm->accel;
    if (accel == PT_ACCEL_AUTO) {
        const std::string keep = g_err;
        accel = (c->auto_bvh && !c->bvh_refused && !c->bvh_failed && ensure_bvh(c) == PT_OK) ? PT_ACCEL_BVH : PT_ACCEL_LINEAR;
        if (!accel) g_err = keep;
    }
    int rc;
    if (accel && (rc = ensure_bvh(c))) return rc;
    const uint32_t nb_max = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_samples, kFeatureRays / np));
    const size_t n_rays = (size_t)nb_max * np;
    if ((rc = c->ft_rays.ensure(6 * n_rays)) || (rc = c->ft_ids.ensure(n_rays)) || (rc = c->ft_t.ensure(n_rays)) || (rc = c->ft_rec.ensure(8 * n_rays)) ||
        (accel && (rc = c->ft_scratch.ensure(3 * n_rays))))
        return rc;
    const ptk::SceneView sv = view_for(c, prm->exact_math);
    ptk::CameraF cf{};
    for (int k = 0; k < 3; ++k) {
        cf.origin[k] = (float)cam->origin[k]; cf.lower_left[k] = (float)cam->lower_left[k];
        cf.horizontal[k] = (float)cam->horizontal[k]; cf.vertical[k] = (float)cam->vertical[k];
    }
    cf.width = cam->width; cf.height = cam->height;
    const hipStream_t st = c->stream;
    const float t_min = (float)prm->t_min, t_max = INFINITY;
    for (uint32_t done = 0; done < n_samples;) {
        const uint32_t nb = std::min(nb_max, n_samples - done);
        const uint32_t s_base = prm->spp_offset + done;
        ptk::FeatureResolveArgs a{};
        a.mat = sv.mat; a.ids = c->ft_ids.p; a.rec = c->ft_rec.p; a.out = reinterpret_cast<float4*>(d_features);
        a.np = np; a.nb = nb; a.n_samples = n_samples; a.load = done > 0; a.finalize = done + nb == n_samples;
        if (prm->exact_math) {
            ptk::launch_feature_rays_exact(cf, s_base, nb, c->ft_rays.p, st);
            ptk::launch_debug_hit_exact(sv, accel, c->ft_rays.p, nb * np, t_min, t_max, c->ft_scratch.p, c->ft_ids.p, c->ft_t.p, c->ft_rec.p, st);
            if (d_features) ptk::launch_feature_resolve_exact(a, st);
        } else {
            ptk::launch_feature_rays_fast(cf, s_base, nb, c->ft_rays.p, st);
            ptk::launch_debug_hit_fast(sv, accel, c->ft_rays.p, nb * np, t_min, t_max, c->ft_scratch.p, c->ft_ids.p, c->ft_t.p, c->ft_rec.p, st);
            if (d_features) ptk::launch_feature_resolve_fast(a, st);
        }
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

// pt_render_denoised, pt_render_denoised_temporal (tp != null) and pt_render_denoised_motion (motion: the ids pass and the
// motion entry): render, features, filter; host buffers, blocking
int render_denoised_impl(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                         const PtDenoise* dn, const PtTemporal* tp, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                         float* out_features, bool motion = false, int32_t* out_ids = nullptr) {
    if ((prm->band_count ? prm->band_count : 1) != 1 || prm->band_index != 0)
        return fail(PT_ERR_INVALID_ARG, "%s: renders the whole image (band_count = 1)", who);
    if (feature_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: feature_samples must be > 0", who);
    if (!c->has_scene) return fail(PT_ERR_INVALID_ARG, "render: no scene uploaded");
    if (cam->width < 2 || cam->height < 2) return fail(PT_ERR_INVALID_ARG, "camera %ux%u: width and height must be >= 2", cam->width, cam->height);
    const uint64_t np64 = (uint64_t)cam->width * cam->height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)np64);
    const size_t np = (size_t)np64;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->host_lin.ensure(3 * np)) || (rc = c->host_rgba.ensure(4 * np)) || (rc = c->dn_feat.ensure(2 * np)) ||
        (rc = c->dn_lin.ensure(3 * np)) || (motion && (rc = c->dn_ids.ensure(np))))
        return rc;
    PtRenderParams p = *prm;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    float* const feat = reinterpret_cast<float*>(c->dn_feat.p);
    uint8_t* const rgba = out_rgba ? c->host_rgba.p : nullptr;
    if ((rc = render_impl(c, cam, &p, FilmState{}, nullptr, c->host_lin.p, nullptr)) ||
        (rc = pt_render_features_device(c, cam, &p, std::min(feature_samples, p.spp), feat)) ||
        (motion && (rc = pt_render_feature_ids_device(c, cam, &p, c->dn_ids.p))) ||
        (rc = motion ? pt_denoise_temporal_motion_device(c, cam, c->host_lin.p, feat, c->dn_ids.p, dn, tp, c->dn_lin.p, rgba)
              : tp   ? pt_denoise_temporal_device(c, cam, c->host_lin.p, feat, dn, tp, c->dn_lin.p, rgba)
                     : pt_denoise_device(c, cam->width, cam->height, c->host_lin.p, feat, dn, c->dn_lin.p, rgba)) ||
        (rc = pt_sync(c)))
        return rc;
    HIP_TRY(hipMemcpy(out_linear, c->dn_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, c->host_rgba.p, 4 * np, hipMemcpyDeviceToHost));
    if (out_noisy) HIP_TRY(hipMemcpy(out_noisy, c->host_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_features) HIP_TRY(hipMemcpy(out_features, feat, 8 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_ids) HIP_TRY(hipMemcpy(out_ids, c->dn_ids.p, np * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PT_OK;
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
// pt_denoise_device.  The arguments are checked before the context is looked at.  d_ids: the motion entry, whose kernel is
// k_denoise_temporal_motion; with_alpha (a motion entry too): the alpha entry with its per-pixel plane, k_denoise_temporal_alpha.
// All store a history frame, and with it the scene's pose becomes the history pose.
int temporal_impl(const char* who, PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features, const int32_t* d_ids,
                  bool motion, const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear, uint8_t* d_out_rgba,
                  const float* d_alpha = nullptr, bool with_alpha = false) {
    if (!cam || !dn || !tp || !d_linear || !d_features || !d_out_linear || (motion && !d_ids) || (with_alpha && !d_alpha))
        return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (cam->width < 2 || cam->height < 2)
        return fail(PT_ERR_INVALID_ARG, "%s: camera %ux%u: width and height must be >= 2", who, cam->width, cam->height);
    if (dn->iterations > 16) return fail(PT_ERR_INVALID_ARG, "%s: %u iterations (at most 16)", who, dn->iterations);
    if (!(dn->sigma_l >= 0.0f) || !(dn->sigma_n >= 0.0f) || !(dn->sigma_d >= 0.0f) || !std::isfinite(dn->sigma_l) ||
        !std::isfinite(dn->sigma_n) || !std::isfinite(dn->sigma_d))
        return fail(PT_ERR_INVALID_ARG, "%s: sigma_l, sigma_n and sigma_d must be finite and >= 0", who);
    if (!(tp->alpha >= 0.0f && tp->alpha <= 1.0f)) return fail(PT_ERR_INVALID_ARG, "%s: alpha %g not in [0, 1]", who, tp->alpha);
    if (!(tp->depth_tol >= 0.0f) || !(tp->normal_tol >= 0.0f) || !std::isfinite(tp->depth_tol) || !std::isfinite(tp->normal_tol))
        return fail(PT_ERR_INVALID_ARG, "%s: depth_tol and normal_tol must be finite and >= 0", who);
    if ((uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if ((uintptr_t)d_linear % 4u || (uintptr_t)d_out_linear % 4u || (uintptr_t)d_out_rgba % 4u)
        return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    if (d_out_linear == d_linear) return fail(PT_ERR_INVALID_ARG, "%s: the output must not be the input", who);
    const uint64_t np64 = (uint64_t)cam->width * cam->height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)np64);
    if ((uintptr_t)d_ids % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_ids must be 4-byte aligned", who);
    if ((uintptr_t)d_alpha % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_alpha must be 4-byte aligned", who);
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    if (motion && !c->has_scene) return fail(PT_ERR_INVALID_ARG, "%s: no scene uploaded", who);
    if (motion && c->view.n_objs > (1u << 24) - 2u)
        return fail(PT_ERR_UNSUPPORTED, "%s: %u objects (an id + 1 must be exact in the history's f32 lane: at most 2^24 - 2)", who, c->view.n_objs);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if (motion && (rc = upload_motion_maps(c))) return rc;
    if ((rc = c->dn_plane[0].ensure(np64)) || (rc = c->dn_plane[1].ensure(np64)) || (rc = c->tm_hist[0].ensure(3 * np64)) ||
        (rc = c->tm_hist[1].ensure(3 * np64)))
        return rc;
    const bool have = c->tm_valid && c->tm_cam.width == cam->width && c->tm_cam.height == cam->height;
    bool same = have;
    for (int k = 0; k < 3; ++k)
        same = same && c->tm_cam.origin[k] == cam->origin[k] && c->tm_cam.lower_left[k] == cam->lower_left[k] &&
               c->tm_cam.horizontal[k] == cam->horizontal[k] && c->tm_cam.vertical[k] == cam->vertical[k];
    ptk::TemporalArgs t{};
    ptk::DenoiseArgs& a = t.dn;
    a.linear = d_linear; a.feat = reinterpret_cast<const float4*>(d_features);
    a.out_linear = d_out_linear; a.out_rgba = d_out_rgba;
    a.width = cam->width; a.height = cam->height;
    a.sigma_l = dn->sigma_l; a.sigma_n = dn->sigma_n; a.sigma_d = dn->sigma_d;
    a.dst = c->dn_plane[0].p; a.finalize = dn->iterations == 0;
    t.hist_src = have ? c->tm_hist[c->tm_cur].p : nullptr;
    t.hist_dst = c->tm_hist[c->tm_cur ^ 1u].p;
    for (int k = 0; k < 3; ++k) {
        t.cur[k] = cam->origin[k]; t.cur[3 + k] = cam->lower_left[k]; t.cur[6 + k] = cam->horizontal[k]; t.cur[9 + k] = cam->vertical[k];
        t.prev[k] = c->tm_cam.origin[k]; t.prev[3 + k] = c->tm_cam.lower_left[k];
        t.prev[6 + k] = c->tm_cam.horizontal[k]; t.prev[9 + k] = c->tm_cam.vertical[k];
    }
    t.same_camera = same;
    t.alpha = tp->alpha; t.depth_tol = tp->depth_tol; t.normal_tol = tp->normal_tol;
    if (motion) {
        ptk::TemporalMotionArgs m{};
        m.t = t; m.ids = d_ids; m.maps = c->mo_maps.p; m.n_objs = c->view.n_objs;
        if (with_alpha) {
            ptk::TemporalAlphaArgs g{};
            g.m = m; g.alpha = d_alpha;
            ptk::launch_denoise_temporal_alpha(g, c->stream);
        } else {
            ptk::launch_denoise_temporal_motion(m, c->stream);
        }
    } else {
        ptk::launch_denoise_temporal(t, c->stream);
    }
    HIP_TRY(hipGetLastError());
    c->tm_cur ^= 1u; c->tm_valid = true; c->tm_cam = *cam;
    if (!c->has_scene) c->tm_pose.clear();
    else if (c->tm_pose_gen != c->pose_gen || c->tm_pose.size() != c->pose.size()) c->tm_pose = c->pose;
    c->tm_pose_gen = c->pose_gen;
    return denoise_steps(c, a, dn->iterations);
}

// The filter of pt_denoise_device and pt_denoise_var_device (with_var: k_denoise_init_var and the caller's variance plane in
// place of k_denoise_init): (u, var) into plane 0, then one k_denoise_step per iteration between the two planes; the last
// launch writes the film planes.
int denoise_impl(const char* who, PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const float* d_features,
                 const float* d_var, bool with_var, const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba) {
    if (!c || !dn || !d_linear || !d_features || !d_out_linear || (with_var && !d_var)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARG, "%s: image %ux%u", who, width, height);
    if (dn->iterations > 16) return fail(PT_ERR_INVALID_ARG, "%s: %u iterations (at most 16)", who, dn->iterations);
    if (!(dn->sigma_l >= 0.0f) || !(dn->sigma_n >= 0.0f) || !(dn->sigma_d >= 0.0f) || !std::isfinite(dn->sigma_l) ||
        !std::isfinite(dn->sigma_n) || !std::isfinite(dn->sigma_d))
        return fail(PT_ERR_INVALID_ARG, "%s: sigma_l, sigma_n and sigma_d must be finite and >= 0", who);
    if ((uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if ((uintptr_t)d_linear % 4u || (uintptr_t)d_out_linear % 4u || (uintptr_t)d_out_rgba % 4u)
        return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    if ((uintptr_t)d_var % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_var must be 4-byte aligned", who);
    if (d_out_linear == d_linear) return fail(PT_ERR_INVALID_ARG, "%s: the output must not be the input", who);
    const uint64_t np64 = (uint64_t)width * height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)np64);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->dn_plane[0].ensure(np64)) || (rc = c->dn_plane[1].ensure(np64))) return rc;
    ptk::DenoiseArgs a{};
    a.linear = d_linear; a.feat = reinterpret_cast<const float4*>(d_features);
    a.out_linear = d_out_linear; a.out_rgba = d_out_rgba;
    a.width = width; a.height = height;
    a.sigma_l = dn->sigma_l; a.sigma_n = dn->sigma_n; a.sigma_d = dn->sigma_d;
    a.dst = c->dn_plane[0].p; a.finalize = dn->iterations == 0;
    if (with_var) ptk::launch_denoise_init_var(a, d_var, c->stream);
    else ptk::launch_denoise(a, true, c->stream);
    HIP_TRY(hipGetLastError());
    return denoise_steps(c, a, dn->iterations);
}

}  // namespace

extern "C" {

int pt_render_features_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t n_samples, float* d_features) {
    if (!d_features) return fail(PT_ERR_INVALID_ARG, "pt_render_features_device: null argument");
    return features_impl("pt_render_features_device", c, cam, prm, n_samples, d_features, nullptr);
}

int pt_render_feature_ids_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, int32_t* d_ids) {
    if (!d_ids) return fail(PT_ERR_INVALID_ARG, "pt_render_feature_ids_device: null argument");
    return features_impl("pt_render_feature_ids_device", c, cam, prm, 1, nullptr, d_ids);
}

int pt_denoise_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const float* d_features,
                      const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba) {
    return denoise_impl("pt_denoise_device", c, width, height, d_linear, d_features, nullptr, false, dn, d_out_linear, d_out_rgba);
}

int pt_denoise_var_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const float* d_features,
                          const float* d_var, const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba) {
    return denoise_impl("pt_denoise_var_device", c, width, height, d_linear, d_features, d_var, true, dn, d_out_linear, d_out_rgba);
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
    HIP_TRY(hipMemcpy(out_linear, c->dn_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, c->host_rgba.p, 4 * np, hipMemcpyDeviceToHost));
    if (out_noisy) HIP_TRY(hipMemcpy(out_noisy, c->host_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_spp) HIP_TRY(hipMemcpy(out_spp, c->ad_count.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_rel_err) HIP_TRY(hipMemcpy(out_rel_err, c->ad_err.p, np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_var) HIP_TRY(hipMemcpy(out_var, c->dn_var.p, np * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_render_denoised(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtDenoise* dn,
                       float* out_linear, uint8_t* out_rgba, float* out_noisy, float* out_features) {
    if (!c || !cam || !prm || !dn || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_denoised: null argument");
    return render_denoised_impl("pt_render_denoised", c, cam, prm, feature_samples, dn, nullptr, out_linear, out_rgba, out_noisy,
                                out_features);
}

int pt_temporal_reset(PtContext* c) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_temporal_reset: null context");
    c->tm_valid = false;
    c->gr_valid = false; c->gr_frame = 0;
    return PT_OK;
}

int pt_denoise_temporal_device(PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features,
                               const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear, uint8_t* d_out_rgba) {
    return temporal_impl("pt_denoise_temporal_device", c, cam, d_linear, d_features, nullptr, false, dn, tp, d_out_linear, d_out_rgba);
}

int pt_denoise_temporal_motion_device(PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features, const int32_t* d_ids,
                                      const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear, uint8_t* d_out_rgba) {
    return temporal_impl("pt_denoise_temporal_motion_device", c, cam, d_linear, d_features, d_ids, true, dn, tp, d_out_linear, d_out_rgba);
}

int pt_render_denoised_motion(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtDenoise* dn,
                              const PtTemporal* tp, float* out_linear, uint8_t* out_rgba, float* out_noisy, float* out_features,
                              int32_t* out_ids) {
    if (!c || !cam || !prm || !dn || !tp || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_denoised_motion: null argument");
    return render_denoised_impl("pt_render_denoised_motion", c, cam, prm, feature_samples, dn, tp, out_linear, out_rgba, out_noisy,
                                out_features, true, out_ids);
}


int pt_denoise_temporal_alpha_device(PtContext* c, const PtCamera* cam, const float* d_linear, const float* d_features, const int32_t* d_ids,
                                     const float* d_alpha, const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear,
                                     uint8_t* d_out_rgba) {
    return temporal_impl("pt_denoise_temporal_alpha_device", c, cam, d_linear, d_features, d_ids, true, dn, tp, d_out_linear, d_out_rgba,
                         d_alpha, true);
}

void pt_default_gradient(PtGradient* out) {
    if (!out) return;
    out->radius = 1;
    out->scale = 1.0f;
}

// The strata's pixel list (k_gradient_list), its render with the previous frame's parameters in the current scene (a list
// render that may take the regenerating kernel, as pt_render_adaptive's passes do), the records and the plane.  The
// arguments are checked before the context is looked at, and everything the list render checks is checked before the first
// launch: a refused call leaves the context as it was.
//
// with_camera (pt_temporal_gradient_camera_device): the strata lie in the image of prev_cam, whose re-trace
// this is, and k_gradient_alpha_camera looks every pixel of cam up in them through d_features.
static int gradient_impl(const char* who, PtContext* c, const PtCamera* cam, const PtCamera* prev_cam, bool with_camera,
                         const PtRenderParams* prev, uint32_t seed, const float* d_prev, const float* d_features, const PtGradient* g,
                         float alpha_min, float* d_alpha) {
    if (!cam || !prev || !d_prev || !g || !d_alpha || (with_camera && (!prev_cam || !d_features)))
        return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((uintptr_t)d_prev % 4u || (uintptr_t)d_alpha % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_prev_linear and d_alpha must be 4-byte aligned", who);
    if (with_camera && (uintptr_t)d_features % 16u) return fail(PT_ERR_INVALID_ARG, "%s: d_features must be 16-byte aligned", who);
    if (with_camera && (prev_cam->width != cam->width || prev_cam->height != cam->height))
        return fail(PT_ERR_INVALID_ARG, "%s: the previous camera is %ux%u, the camera %ux%u", who, prev_cam->width, prev_cam->height,
                    cam->width, cam->height);
    if ((prev->band_count ? prev->band_count : 1) != 1 || prev->band_index != 0)
        return fail(PT_ERR_INVALID_ARG, "%s: works on the whole image (band_count = 1)", who);
    if (g->radius > ptgr::kMaxRadius) return fail(PT_ERR_INVALID_ARG, "%s: radius %u (at most %u)", who, g->radius, ptgr::kMaxRadius);
    if (!(g->scale >= 0.0f) || !std::isfinite(g->scale)) return fail(PT_ERR_INVALID_ARG, "%s: scale must be finite and >= 0", who);
    if (!(alpha_min >= 0.0f && alpha_min <= 1.0f)) return fail(PT_ERR_INVALID_ARG, "%s: alpha_min %g not in [0, 1]", who, alpha_min);
    if (cam->width < 2 || cam->height < 2)
        return fail(PT_ERR_INVALID_ARG, "%s: camera %ux%u: width and height must be >= 2", who, cam->width, cam->height);
    if (prev->spp == 0) return fail(PT_ERR_INVALID_ARG, "%s: spp must be > 0", who);
    if (prev->integrator > PT_INTEGRATOR_BRDF_ONLY) return fail(PT_ERR_INVALID_ARG, "%s: unknown integrator %u", who, prev->integrator);
    if (prev->accel > PT_ACCEL_AUTO) return fail(PT_ERR_INVALID_ARG, "%s: unknown accel %u", who, prev->accel);
    const uint64_t np64 = (uint64_t)cam->width * cam->height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)np64);
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    if (!c->has_scene) return fail(PT_ERR_INVALID_ARG, "%s: no scene uploaded", who);
    HIP_TRY(hipSetDevice(c->device));
    const size_t ns = (size_t)ptgr::strata(cam->width) * ptgr::strata(cam->height);
    int rc;
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
    if ((rc = render_impl(c, with_camera ? prev_cam : cam, &p, FilmState{}, &lr, c->gr_film.p, nullptr))) return rc;
    ptk::launch_gradient_strata(a, c->stream);
    if (with_camera) {
        ptk::TemporalArgs t{};
        t.dn.feat = reinterpret_cast<const float4*>(d_features);
        t.dn.width = cam->width; t.dn.height = cam->height;
        bool same = true;
        for (int k = 0; k < 3; ++k) {
            t.cur[k] = cam->origin[k]; t.cur[3 + k] = cam->lower_left[k]; t.cur[6 + k] = cam->horizontal[k]; t.cur[9 + k] = cam->vertical[k];
            t.prev[k] = prev_cam->origin[k]; t.prev[3 + k] = prev_cam->lower_left[k];
            t.prev[6 + k] = prev_cam->horizontal[k]; t.prev[9 + k] = prev_cam->vertical[k];
            same = same && prev_cam->origin[k] == cam->origin[k] && prev_cam->lower_left[k] == cam->lower_left[k] &&
                   prev_cam->horizontal[k] == cam->horizontal[k] && prev_cam->vertical[k] == cam->vertical[k];
        }
        t.same_camera = same;
        ptk::launch_gradient_alpha_camera(a, t, c->stream);
    } else {
        ptk::launch_gradient_alpha(a, c->stream);
    }
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_temporal_gradient_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prev, uint32_t seed, const float* d_prev,
                                const PtGradient* g, float alpha_min, float* d_alpha) {
    return gradient_impl("pt_temporal_gradient_device", c, cam, nullptr, false, prev, seed, d_prev, nullptr, g, alpha_min, d_alpha);
}

int pt_temporal_gradient_camera_device(PtContext* c, const PtCamera* cam, const PtCamera* prev_cam, const PtRenderParams* prev, uint32_t seed,
                                       const float* d_prev, const float* d_features, const PtGradient* g, float alpha_min, float* d_alpha) {
    return gradient_impl("pt_temporal_gradient_camera_device", c, cam, prev_cam, true, prev, seed, d_prev, d_features, g, alpha_min, d_alpha);
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
    if (out_xy) HIP_TRY(hipMemcpy(out_xy, c->gr_list.p, ns * sizeof(uint2), hipMemcpyDeviceToHost));
    if (out_film) HIP_TRY(hipMemcpy(out_film, c->gr_film.p, 3 * ns * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rec) HIP_TRY(hipMemcpy(out_rec, c->gr_rec.p, 2 * ns * sizeof(double), hipMemcpyDeviceToHost));
    return PT_OK;
}

// pt_render_denoised_motion with the alpha plane between the ids pass and the accumulation, and the frame's noisy film kept
// for the next call.  any_camera (pt_render_denoised_gradient_camera): the previous frame stays usable when the camera moved,
// and the plane is pt_temporal_gradient_camera_device's.
static int render_gradient_impl(const char* who, bool any_camera, PtContext* c, const PtCamera* cam, const PtRenderParams* prm,
                                uint32_t feature_samples, const PtDenoise* dn, const PtTemporal* tp, const PtGradient* g, float* out_linear,
                                uint8_t* out_rgba, float* out_noisy, float* out_features, int32_t* out_ids, float* out_alpha) {
    if (!c || !cam || !prm || !dn || !tp || !g || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((prm->band_count ? prm->band_count : 1) != 1 || prm->band_index != 0)
        return fail(PT_ERR_INVALID_ARG, "%s: renders the whole image (band_count = 1)", who);
    if (feature_samples == 0) return fail(PT_ERR_INVALID_ARG, "%s: feature_samples must be > 0", who);
    if (g->radius > ptgr::kMaxRadius) return fail(PT_ERR_INVALID_ARG, "%s: radius %u (at most %u)", who, g->radius, ptgr::kMaxRadius);
    if (!(g->scale >= 0.0f) || !std::isfinite(g->scale)) return fail(PT_ERR_INVALID_ARG, "%s: scale must be finite and >= 0", who);
    if (!(tp->alpha >= 0.0f && tp->alpha <= 1.0f)) return fail(PT_ERR_INVALID_ARG, "%s: alpha %g not in [0, 1]", who, tp->alpha);
    if (!c->has_scene) return fail(PT_ERR_INVALID_ARG, "render: no scene uploaded");
    if (cam->width < 2 || cam->height < 2) return fail(PT_ERR_INVALID_ARG, "camera %ux%u: width and height must be >= 2", cam->width, cam->height);
    const uint64_t np64 = (uint64_t)cam->width * cam->height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "%s: %llu pixels", who, (unsigned long long)np64);
    const size_t np = (size_t)np64;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->host_lin.ensure(3 * np)) || (rc = c->host_rgba.ensure(4 * np)) || (rc = c->dn_feat.ensure(2 * np)) ||
        (rc = c->dn_lin.ensure(3 * np)) || (rc = c->dn_ids.ensure(np)) || (rc = c->gr_alpha.ensure(np)))
        return rc;
    // the previous frame is usable: one of the two entries completed it, at this size, through this camera (any_camera: through
    // any), and the history it went into is there
    bool usable = c->gr_valid && c->tm_valid && c->gr_prev.cap >= 3 * np && c->gr_cam.width == cam->width && c->gr_cam.height == cam->height;
    for (int k = 0; k < 3 && !any_camera; ++k)
        usable = usable && c->gr_cam.origin[k] == cam->origin[k] && c->gr_cam.lower_left[k] == cam->lower_left[k] &&
                 c->gr_cam.horizontal[k] == cam->horizontal[k] && c->gr_cam.vertical[k] == cam->vertical[k];
    const PtCamera prev_cam = c->gr_cam;
    c->gr_valid = false;                      // (a frame that fails from here on leaves none)
    PtRenderParams p = *prm;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    float* const feat = reinterpret_cast<float*>(c->dn_feat.p);
    uint8_t* const rgba = out_rgba ? c->host_rgba.p : nullptr;
    if ((rc = render_impl(c, cam, &p, FilmState{}, nullptr, c->host_lin.p, nullptr)) ||
        (rc = pt_render_features_device(c, cam, &p, std::min(feature_samples, p.spp), feat)) ||
        (rc = pt_render_feature_ids_device(c, cam, &p, c->dn_ids.p)))
        return rc;
    if (usable) {
        if ((rc = any_camera ? pt_temporal_gradient_camera_device(c, cam, &prev_cam, &c->gr_params, c->gr_frame, c->gr_prev.p, feat, g,
                                                                  tp->alpha, c->gr_alpha.p)
                             : pt_temporal_gradient_device(c, cam, &c->gr_params, c->gr_frame, c->gr_prev.p, g, tp->alpha, c->gr_alpha.p)))
            return rc;
    } else {
        HIP_TRY(hipMemsetAsync(c->gr_alpha.p, 0xFF, np * sizeof(float), c->stream));      // every entry a NaN: no measurement
    }
    if ((rc = pt_denoise_temporal_alpha_device(c, cam, c->host_lin.p, feat, c->dn_ids.p, c->gr_alpha.p, dn, tp, c->dn_lin.p, rgba)) ||
        (rc = c->gr_prev.ensure(3 * np)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->gr_prev.p, c->host_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = pt_sync(c))) return rc;
    c->gr_valid = true; c->gr_params = p; c->gr_cam = *cam; ++c->gr_frame;
    HIP_TRY(hipMemcpy(out_linear, c->dn_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, c->host_rgba.p, 4 * np, hipMemcpyDeviceToHost));
    if (out_noisy) HIP_TRY(hipMemcpy(out_noisy, c->host_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_features) HIP_TRY(hipMemcpy(out_features, feat, 8 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_ids) HIP_TRY(hipMemcpy(out_ids, c->dn_ids.p, np * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_alpha) HIP_TRY(hipMemcpy(out_alpha, c->gr_alpha.p, np * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_render_denoised_gradient(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtDenoise* dn,
                                const PtTemporal* tp, const PtGradient* g, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                float* out_features, int32_t* out_ids, float* out_alpha) {
    return render_gradient_impl("pt_render_denoised_gradient", false, c, cam, prm, feature_samples, dn, tp, g, out_linear, out_rgba, out_noisy,
                                out_features, out_ids, out_alpha);
}

int pt_render_denoised_gradient_camera(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                                       const PtDenoise* dn, const PtTemporal* tp, const PtGradient* g, float* out_linear, uint8_t* out_rgba,
                                       float* out_noisy, float* out_features, int32_t* out_ids, float* out_alpha) {
    return render_gradient_impl("pt_render_denoised_gradient_camera", true, c, cam, prm, feature_samples, dn, tp, g, out_linear, out_rgba,
                                out_noisy, out_features, out_ids, out_alpha);
}

int pt_render_denoised_temporal(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                                const PtDenoise* dn, const PtTemporal* tp, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                float* out_features) {
    if (!c || !cam || !prm || !dn || !tp || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_denoised_temporal: null argument");
    return render_denoised_impl("pt_render_denoised_temporal", c, cam, prm, feature_samples, dn, tp, out_linear, out_rgba, out_noisy,
                                out_features);
}

}  // extern "C"
