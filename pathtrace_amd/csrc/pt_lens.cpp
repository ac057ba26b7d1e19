// pt_lens.cpp -- the host side of the thin-lens camera that is not the render driver's (pt_api.cpp: render_source_impl): the checks
// and the device's words (pt_lens.h), the defaults, the debug entries, and the entries of the lens forms pt_denoise.cpp holds.
#include "pt_entry.h"
#include "pt_lens.h"

ptk::CameraF camera_f32(const PtCamera* cam) {
    ptk::CameraF cf{};
    for (int k = 0; k < 3; ++k) {
        cf.origin[k] = (float)cam->origin[k]; cf.lower_left[k] = (float)cam->lower_left[k];
        cf.horizontal[k] = (float)cam->horizontal[k]; cf.vertical[k] = (float)cam->vertical[k];
    }
    cf.width = cam->width; cf.height = cam->height;
    return cf;
}

// The lens and the camera's frame checked (a check answers in the entry's name, who), Lu, Lv and inv_phi in f32.  No context.
int lens_setup(const char* who, const PtCamera* cam, const PtLens* lens, ptk::LensF* out) {
    ptlens::Setup s;
    switch (ptlens::setup(cam->origin, cam->lower_left, cam->horizontal, cam->vertical, lens->aperture, lens->focus_distance, &s)) {
    case ptlens::kOk: break;
    case ptlens::kBadAperture: return fail(PT_ERR_INVALID_ARG, "%s: aperture %g must be finite and >= 0", who, lens->aperture);
    case ptlens::kBadFocus: return fail(PT_ERR_INVALID_ARG, "%s: focus_distance %g must be finite and > 0", who, lens->focus_distance);
    default:
        return fail(PT_ERR_INVALID_ARG, "%s: degenerate camera (the view axis, horizontal and vertical must have a finite length > 0)", who);
    }
    for (int k = 0; k < 3; ++k) { out->lu[k] = s.lu[k]; out->lv[k] = s.lv[k]; }
    out->inv_phi = s.inv_phi;
    return PT_OK;
}

extern "C" {

void pt_default_lens(PtLens* out) {
    if (!out) return;
    out->aperture = 0.0;
    out->focus_distance = 1.0;
}

int pt_render_features_lens_device(PtContext* c, const PtCamera* cam, const PtLens* lens, const PtRenderParams* prm, uint32_t n_samples,
                                   float* d_features) {
    if (!lens) return fail(PT_ERR_INVALID_ARG, "pt_render_features_lens_device: null argument");
    return features_source_device("pt_render_features_lens_device", c, cam, {lens, nullptr}, prm, n_samples, d_features);
}

int pt_render_lens_denoised(PtContext* c, const PtCamera* cam, const PtLens* lens, const PtRenderParams* prm, uint32_t feature_samples,
                            const PtDenoise* dn, float* out_linear, uint8_t* out_rgba, float* out_noisy, float* out_features) {
    if (!lens) return fail(PT_ERR_INVALID_ARG, "pt_render_lens_denoised: null argument");
    return render_source_denoised_host("pt_render_lens_denoised", c, cam, {lens, nullptr}, prm, feature_samples, dn, out_linear, out_rgba,
                                       out_noisy, out_features);
}

int pt_debug_lens_setup(const PtCamera* cam, const PtLens* lens, float* out7) {
    if (!cam || !lens || !out7) return fail(PT_ERR_INVALID_ARG, "pt_debug_lens_setup: null argument");
    ptk::LensF l;
    if (int rc = lens_setup("pt_debug_lens_setup", cam, lens, &l)) return rc;
    for (int k = 0; k < 3; ++k) { out7[k] = l.lu[k]; out7[3 + k] = l.lv[k]; }
    out7[6] = l.inv_phi;
    return PT_OK;
}

int pt_debug_lens_rays(PtContext* c, const PtCamera* cam, const PtLens* lens, const uint32_t* xys, uint32_t n, uint32_t exact_math,
                       float* out8) {
    if (!c || !cam || !lens || (n && (!xys || !out8))) return fail(PT_ERR_INVALID_ARG, "pt_debug_lens_rays: null argument");
    ptk::LensF l;
    int rc;
    if ((rc = lens_setup("pt_debug_lens_rays", cam, lens, &l)) || (rc = check_camera_size(cam))) return rc;
    ptk::RaySourceF s{};
    s.tag = ptk::kSrcLens;
    s.cam = camera_f32(cam);
    s.lens = l;
    return debug_source_rays(c, s, xys, n, exact_math, 8, out8);
}

}  // extern "C"
