// pt_filter.cpp -- the host side of the film's reconstruction filters (rule: pt_filter.h): the render whose resolve
// is k_resolve_filter, that kernel on given samples, and the same rule on host planes on the CPU.  The entries' rule and the
// checks they share with the other film entries: pt_entry.h; here, the filter's own.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_entry.h"
#include "pt_filter.h"

namespace {

int check_filter(const char* who, const PtFilter* f, ptflt::Rule* r) {
    if (f->kind >= ptflt::kKinds) return fail(PT_ERR_INVALID_ARG, "%s: unknown filter kind %u", who, f->kind);
    if (!std::isfinite(f->radius) || !(f->radius >= 0.5f) || !(f->radius <= 2.5f))
        return fail(PT_ERR_INVALID_ARG, "%s: radius must be finite and in [0.5, 2.5]", who);
    if (f->kind == PT_FILTER_GAUSSIAN && (!std::isfinite(f->a) || !(f->a > 0.0f) || !(f->a <= 16.0f)))
        return fail(PT_ERR_INVALID_ARG, "%s: the Gaussian's alpha (a) must be finite and in (0, 16]", who);
    if (f->kind == PT_FILTER_MITCHELL && (!std::isfinite(f->a) || !(f->a >= 0.0f) || !(f->a <= 1.0f) || !std::isfinite(f->b) || !(f->b >= 0.0f) ||
                                          !(f->b <= 1.0f)))
        return fail(PT_ERR_INVALID_ARG, "%s: Mitchell's B (a) and C (b) must be finite and in [0, 1]", who);
    if (!ptflt::rule(f->kind, f->radius, f->a, f->b, r)) return fail(PT_ERR_INVALID_ARG, "%s: filter parameters out of range", who);
    return PT_OK;
}

// the planes an entry writes: aligned, and no two of them (nor any of them and the samples read) share a byte
int check_planes(const char* who, size_t np, const void* samples, size_t samples_bytes, const float* linear, const uint8_t* rgba,
                 const float* plain, const double* wsum) {
    if ((uintptr_t)samples % 4u || (uintptr_t)linear % 4u || (uintptr_t)rgba % 4u || (uintptr_t)plain % 4u || (uintptr_t)wsum % 8u)
        return fail(PT_ERR_INVALID_ARG, "%s: the sample and film buffers must be 4-byte aligned, the weight sums 8-byte", who);
    return check_no_alias(who, {{linear, 12 * np}, {rgba, 4 * np}, {plain, 12 * np}, {wsum, 8 * np}}, {samples, samples_bytes});
}

ptk::FilterResolveArgs resolve_args(const PtContext* c, const ptflt::Rule& r, uint32_t width, uint32_t height, uint32_t n, float* d_linear,
                                    uint8_t* d_rgba, float* d_plain, double* d_wsum) {
    ptk::FilterResolveArgs a{};
    a.kind = r.kind; a.m = r.m; a.R = r.R; a.alpha = r.alpha; a.gR = r.gR;
    a.a3 = r.a3; a.a2 = r.a2; a.a0 = r.a0; a.b3 = r.b3; a.b2 = r.b2; a.b1 = r.b1; a.b0 = r.b0;
    a.state = c->flt_state.p;
    a.width = width; a.height = height; a.n_total = n;
    a.out_linear = d_linear; a.out_rgba = d_rgba; a.out_plain = d_plain; a.out_wsum = d_wsum;
    return a;
}

// what pt_render_filtered_device and pt_render_filtered_host refuse before they touch the context
int check_render_filtered(const char* who, const PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtFilter* f,
                          ptflt::Rule* r) {
    int rc;
    if ((rc = check_filter(who, f, r)) || (rc = check_image_size(who, cam->width, cam->height)) ||
        (rc = check_whole_image(who, ": renders", ": the filter reads a pixel's neighbours", prm)) || (rc = check_spp(prm->spp)))
        return rc;
    return check_scene(c);
}

int render_filtered_device(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtFilter* f, float* d_linear,
                           uint8_t* d_rgba, float* d_plain) {
    if (!c || !cam || !prm || !f || !d_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptflt::Rule r;
    int rc;
    if ((rc = check_render_filtered(who, c, cam, prm, f, &r))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    if ((rc = check_planes(who, np, nullptr, 0, d_linear, d_rgba, d_plain, nullptr))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->flt_state.ensure(7 * np))) return rc;
    FilterPass pass;
    pass.r = resolve_args(c, r, cam->width, cam->height, prm->spp, d_linear, d_rgba, d_plain, nullptr);
    PtRenderParams p = *prm;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    return render_impl(c, cam, &p, FilmState{}, nullptr, d_linear, d_rgba, nullptr, nullptr, nullptr, &pass);
}

}  // namespace

extern "C" {

void pt_default_filter(PtFilter* out) {
    if (!out) return;
    out->kind = PT_FILTER_GAUSSIAN;
    out->radius = 1.5f;
    out->a = 2.0f;
    out->b = 0.0f;
}

int pt_debug_filter_weight(const PtFilter* flt, double t, double* f) {
    const char* who = "pt_debug_filter_weight";
    if (!flt || !f) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptflt::Rule r;
    if (int rc = check_filter(who, flt, &r)) return rc;
    *f = ptflt::weight1(r, t < 0.0 ? -t : t);
    return PT_OK;
}

int pt_debug_filter_offsets(uint32_t x, uint32_t y, uint32_t sample, double* ox, double* oy) {
    if (!ox || !oy) return fail(PT_ERR_INVALID_ARG, "pt_debug_filter_offsets: null argument");
    ptflt::offsets(x, y, sample, ox, oy);
    return PT_OK;
}

int pt_debug_filter_exp_neg(double e, double* out) {
    if (!out || !(e >= 0.0) || !(e <= 100.0)) return fail(PT_ERR_INVALID_ARG, "pt_debug_filter_exp_neg: e must lie in [0, 100]");
    *out = ptflt::exp_neg(e);
    return PT_OK;
}

// The rule header on the CPU
int pt_filter_host(const PtFilter* flt, uint32_t width, uint32_t height, uint32_t n, uint32_t first_sample, const float* samples,
                   float* out_linear, uint8_t* out_rgba, float* out_plain, double* out_wsum) {
    const char* who = "pt_filter_host";
    if (!flt || !samples || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptflt::Rule r;
    int rc;
    if ((rc = check_filter(who, flt, &r)) || (rc = check_image_size(who, width, height))) return rc;
    if (n == 0) return fail(PT_ERR_INVALID_ARG, "%s: n must be > 0", who);
    const size_t np = (size_t)width * height;
    if ((rc = check_planes(who, np, samples, 12 * np * n, out_linear, out_rgba, out_plain, out_wsum))) return rc;
    ptflt::host_film(r, width, height, n, first_sample, samples, out_linear, out_rgba, out_plain, out_wsum);
    return PT_OK;
}

// The kernel on given samples: ceil(n / batch) launches of k_resolve_filter, each starting from the sums the one before left;
// all on the context's stream
int pt_filter_samples_device(PtContext* c, const PtFilter* flt, uint32_t width, uint32_t height, uint32_t n, uint32_t first_sample,
                             uint32_t batch, const float* d_samples, float* d_linear, uint8_t* d_rgba, float* d_plain, double* d_wsum) {
    const char* who = "pt_filter_samples_device";
    if (!flt || !d_samples || !d_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptflt::Rule r;
    int rc;
    if ((rc = check_filter(who, flt, &r)) || (rc = check_image_size(who, width, height))) return rc;
    if (n == 0) return fail(PT_ERR_INVALID_ARG, "%s: n must be > 0", who);
    const size_t np = (size_t)width * height;
    if ((rc = check_planes(who, np, d_samples, 12 * np * n, d_linear, d_rgba, d_plain, d_wsum))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->flt_state.ensure(7 * np))) return rc;
    const uint32_t step = batch ? std::min(batch, n) : n;
    ptk::FilterResolveArgs a = resolve_args(c, r, width, height, n, d_linear, d_rgba, d_plain, d_wsum);
    for (uint32_t done = 0; done < n; done += step) {
        a.nb = std::min(step, n - done);
        a.lsamp = reinterpret_cast<const ptk::Rgb*>(d_samples) + (size_t)done * np;
        a.first_sample = first_sample + done;
        a.load = done > 0;
        a.finalize = done + a.nb == n;
        ptk::launch_resolve_filter(a, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return PT_OK;
}

int pt_render_filtered_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtFilter* flt, float* d_linear,
                              uint8_t* d_rgba, float* d_plain) {
    return render_filtered_device("pt_render_filtered_device", c, cam, prm, flt, d_linear, d_rgba, d_plain);
}

int pt_render_filtered_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtFilter* flt, float* out_linear,
                            uint8_t* out_rgba, float* out_plain, double* out_wsum) {
    const char* who = "pt_render_filtered_host";
    if (!c || !cam || !prm || !flt || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptflt::Rule r;
    int rc;
    if ((rc = check_render_filtered(who, c, cam, prm, flt, &r))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    HIP_TRY(hipSetDevice(c->device));
    return render_staged(c, 3 * np, out_rgba ? 4 * np : 0, [&](float* d_linear, uint8_t* d_rgba) {
        if (int bad = c->flt_plain.ensure(out_plain ? 3 * np : 0)) return bad;
        return render_filtered_device(who, c, cam, prm, flt, d_linear, d_rgba, out_plain ? c->flt_plain.p : nullptr);
    }, [&] {
        return copy_back({{out_linear, c->host_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                          {out_plain, c->flt_plain.p, 3 * np * sizeof(float)},
                          {out_wsum, c->flt_state.p + 3 * np, np * sizeof(double)}});   // plane 3 of the state: Wt
    });
}

}  // extern "C"
