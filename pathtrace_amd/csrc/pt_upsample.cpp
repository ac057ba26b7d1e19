// pt_upsample.cpp -- the host side of feature-guided upsampling (rule: pt_upsample.h): the device entry (one launch
// of k_upsample), the same rule on host planes on the CPU, and the one-call frame that renders low and reconstructs at full size.
// The entries' rule, the pixel limit and the one-call frame's staging: pt_entry.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_entry.h"
#include "pt_upsample.h"

namespace {

int check_upsample(const char* who, const PtUpsample* up) {
    if (!(up->sigma_n >= 0.0f) || !(up->sigma_d >= 0.0f) || !std::isfinite(up->sigma_n) || !std::isfinite(up->sigma_d))
        return fail(PT_ERR_INVALID_ARG, "%s: sigma_n and sigma_d must be finite and >= 0", who);
    return PT_OK;
}

int check_size(const char* who, uint32_t lo_width, uint32_t lo_height, uint32_t width, uint32_t height) {
    if (lo_width < 2 || lo_height < 2 || width < 2 || height < 2)
        return fail(PT_ERR_INVALID_ARG, "%s: image %ux%u from %ux%u: every dimension must be >= 2", who, width, height, lo_width, lo_height);
    if (lo_width > width || lo_height > height)
        return fail(PT_ERR_INVALID_ARG, "%s: the low size %ux%u is above the full size %ux%u", who, lo_width, lo_height, width, height);
    return check_pixel_count(who, width, height);      // (the two lines above: this entry's own four-dimension form)
}

// What pt_upsample_device and pt_upsample_host read and write, and what both check before anything is looked at
struct Planes { const float* lo_linear; const float* lo_features; const float* features; float* out_linear; uint8_t* out_rgba; };
int check_planes(const char* who, uint32_t lo_width, uint32_t lo_height, uint32_t width, uint32_t height, const Planes& f, const PtUpsample* up) {
    if (!f.lo_linear || !f.lo_features || !f.features || !up || !f.out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((uintptr_t)f.lo_features % 16u || (uintptr_t)f.features % 16u)
        return fail(PT_ERR_INVALID_ARG, "%s: the feature records must be 16-byte aligned", who);
    if ((uintptr_t)f.lo_linear % 4u || (uintptr_t)f.out_linear % 4u || (uintptr_t)f.out_rgba % 4u)
        return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    int rc;
    if ((rc = check_size(who, lo_width, lo_height, width, height))) return rc;
    // (byte ranges, not addresses: an output that starts inside an input is overwritten under the taps other threads still read)
    const size_t np = (size_t)width * height, np_lo = (size_t)lo_width * lo_height;
    const Range in[3] = {{f.lo_linear, 12 * np_lo}, {f.lo_features, 32 * np_lo}, {f.features, 32 * np}};
    const Range out_lin{f.out_linear, 12 * np}, out_rgba{f.out_rgba, 4 * np};        // (a null out_rgba: no range)
    for (const Range& q : in)
        if (ranges_overlap(out_lin, q) || ranges_overlap(out_rgba, q)) return fail(PT_ERR_INVALID_ARG, "%s: the output must not be an input", who);
    if (ranges_overlap(out_lin, out_rgba)) return fail(PT_ERR_INVALID_ARG, "%s: the two outputs must not share a byte", who);
    return check_upsample(who, up);
}

}  // namespace

extern "C" {

void pt_default_upsample(PtUpsample* out) {
    if (!out) return;
    out->sigma_n = 128.0f;
    out->sigma_d = 0.025f;
}

// One launch of k_upsample on the context's stream; nothing of the context but its device and stream is read
int pt_upsample_device(PtContext* c, uint32_t lo_width, uint32_t lo_height, const float* d_lo_linear, const float* d_lo_features,
                       uint32_t width, uint32_t height, const float* d_features, const PtUpsample* up, float* d_out_linear,
                       uint8_t* d_out_rgba) {
    const char* who = "pt_upsample_device";
    int rc;
    if ((rc = check_planes(who, lo_width, lo_height, width, height, {d_lo_linear, d_lo_features, d_features, d_out_linear, d_out_rgba}, up)))
        return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    ptk::UpsampleArgs a{};
    a.lo_linear = d_lo_linear; a.lo_feat = reinterpret_cast<const float4*>(d_lo_features); a.feat = reinterpret_cast<const float4*>(d_features);
    a.out_linear = d_out_linear; a.out_rgba = d_out_rgba;
    a.width = width; a.height = height; a.lo_width = lo_width; a.lo_height = lo_height;
    a.sigma_n = up->sigma_n; a.sigma_d = up->sigma_d;
    ptk::launch_upsample(a, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// The rule header on the CPU, pixel by pixel: what k_upsample computes, as the host compiler builds it
int pt_upsample_host(uint32_t lo_width, uint32_t lo_height, const float* lo_linear, const float* lo_features, uint32_t width,
                     uint32_t height, const float* features, const PtUpsample* up, float* out_linear, uint8_t* out_rgba) {
    int rc;
    if ((rc = check_planes("pt_upsample_host", lo_width, lo_height, width, height, {lo_linear, lo_features, features, out_linear, out_rgba}, up)))
        return rc;
    const ptup::Shape s{width, height, lo_width, lo_height};
    const ptup::Rec* const lo_feat = reinterpret_cast<const ptup::Rec*>(lo_features);
    const ptup::Rec* const feat = reinterpret_cast<const ptup::Rec*>(features);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            ptup::pixel(s, lo_linear, lo_feat, feat[p], x, y, up->sigma_n, up->sigma_d, out_linear + 3 * p);
            if (out_rgba) {
                const uint32_t q8 = ptup::rgba8(out_linear + 3 * p);
                std::memcpy(out_rgba + 4 * p, &q8, 4);
            }
        }
    return PT_OK;
}

// Render low, reconstruct at full size: pt_render_denoised's device part through the low camera (the denoised low film in
// dn_lin, its features in dn_feat), the full-size features into up_feat, k_upsample into up_lin; host buffers, blocking
int pt_render_denoised_upsampled(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t lo_width, uint32_t lo_height,
                                 uint32_t feature_samples, const PtDenoise* dn, const PtUpsample* up, float* out_linear, uint8_t* out_rgba,
                                 float* out_lo_linear, float* out_features) {
    const char* who = "pt_render_denoised_upsampled";
    if (!c || !cam || !prm || !dn || !up || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_size(who, lo_width, lo_height, cam->width, cam->height)) || (rc = check_upsample(who, up))) return rc;
    PtCamera lo_cam = *cam;                   // the cached frustum fields do not depend on the pixel count
    lo_cam.width = lo_width; lo_cam.height = lo_height;
    const size_t np = (size_t)cam->width * cam->height, np_lo = (size_t)lo_width * lo_height;
    PtRenderParams p;
    if ((rc = denoised_frame_device(who, c, &lo_cam, prm, feature_samples, dn, &p))) return rc;      // (the remaining checks are its own)
    // (the RGBA8 staging whether asked for or not, and none of host_lin: it holds the low film's noisy input)
    return render_staged(c, 0, 4 * np, [&](float*, uint8_t* d_rgba) {
        int bad;
        if ((bad = c->up_feat.ensure(2 * np)) || (bad = c->up_lin.ensure(3 * np))) return bad;
        float* const feat = reinterpret_cast<float*>(c->up_feat.p);
        if ((bad = pt_render_features_device(c, cam, &p, std::min(feature_samples, p.spp), feat))) return bad;
        return pt_upsample_device(c, lo_width, lo_height, c->dn_lin.p, reinterpret_cast<float*>(c->dn_feat.p), cam->width, cam->height, feat, up,
                                  c->up_lin.p, out_rgba ? d_rgba : nullptr);
    }, [&] {
        return copy_back({{out_linear, c->up_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                          {out_lo_linear, c->dn_lin.p, 3 * np_lo * sizeof(float)}, {out_features, c->up_feat.p, 8 * np * sizeof(float)}});
    });
}

}  // extern "C"
