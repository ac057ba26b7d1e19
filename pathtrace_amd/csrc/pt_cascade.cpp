// pt_cascade.cpp -- the host side of the brightness cascade (rule: pt_cascade.h): the render whose resolve is
// k_resolve_cascade followed by k_cascade_reweight, the two kernels on given samples, and the same rule on host planes on the
// CPU.  The entries' rule and the checks they share with the other film entries: pt_entry.h; here, the cascade's own.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_entry.h"
#include "pt_cascade.h"

namespace {

int check_cascade(const char* who, const PtCascade* cs, ptcas::Levels* lv) {
    if (cs->layers < ptcas::kMinLayers || cs->layers > ptcas::kMaxLayers)
        return fail(PT_ERR_INVALID_ARG, "%s: layers %u not in [%u, %u]", who, cs->layers, ptcas::kMinLayers, ptcas::kMaxLayers);
    if (!std::isfinite(cs->start) || !(cs->start > 0.0f)) return fail(PT_ERR_INVALID_ARG, "%s: start must be finite and > 0", who);
    if (!std::isfinite(cs->base) || !(cs->base >= 2.0f)) return fail(PT_ERR_INVALID_ARG, "%s: base must be finite and >= 2", who);
    if (!std::isfinite(cs->kappa) || !(cs->kappa >= 0.0f)) return fail(PT_ERR_INVALID_ARG, "%s: kappa must be finite and >= 0", who);
    if (!ptcas::levels(cs->layers, cs->start, cs->base, cs->kappa, lv))
        return fail(PT_ERR_INVALID_ARG, "%s: the level table start * base^k overflows within %u layers", who, cs->layers);
    return PT_OK;
}

// the planes an entry writes: aligned, and no two of them (nor any of them and the samples read) share a byte
int check_planes(const char* who, size_t np, const void* samples, size_t samples_bytes, const float* linear, const uint8_t* rgba,
                 const float* plain) {
    if ((uintptr_t)samples % 4u || (uintptr_t)linear % 4u || (uintptr_t)rgba % 4u || (uintptr_t)plain % 4u)
        return fail(PT_ERR_INVALID_ARG, "%s: the sample and film buffers must be 4-byte aligned", who);
    return check_no_alias(who, {{linear, 12 * np}, {rgba, 4 * np}, {plain, 12 * np}}, {samples, samples_bytes});
}

int ensure_state(PtContext* c, uint32_t K, size_t np) {
    int rc;
    if ((rc = c->cas_state.ensure((3 * (size_t)K + 3) * np)) || (rc = c->cas_cnt.ensure((size_t)K * np))) return rc;
    return PT_OK;
}

ptk::CascadeResolveArgs resolve_args(const PtContext* c, const ptcas::Levels& lv) {
    ptk::CascadeResolveArgs r{};
    for (uint32_t k = 0; k < ptcas::kMaxLayers; ++k) r.B[k] = lv.B[k];
    r.kappa = lv.kappa; r.K = lv.K;
    r.state = c->cas_state.p; r.cnt = c->cas_cnt.p;
    return r;
}

int reweight(PtContext* c, const ptcas::Levels& lv, uint32_t width, uint32_t height, uint32_t n, float* d_linear, uint8_t* d_rgba,
             float* d_plain, float* d_weights) {
    ptk::CascadeReweightArgs w{};
    for (uint32_t k = 0; k < ptcas::kMaxLayers; ++k) w.B[k] = lv.B[k];
    w.kappa = lv.kappa; w.K = lv.K;
    w.state = c->cas_state.p; w.cnt = c->cas_cnt.p;
    w.width = width; w.height = height; w.n_total = n;
    w.out_linear = d_linear; w.out_rgba = d_rgba; w.out_plain = d_plain; w.out_weights = d_weights;
    ptk::launch_cascade_reweight(w, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// what pt_render_cascade_device and pt_render_cascade_host refuse before they touch the context
int check_render_cascade(const char* who, const PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtCascade* cs,
                         ptcas::Levels* lv) {
    int rc;
    if ((rc = check_cascade(who, cs, lv)) || (rc = check_image_size(who, cam->width, cam->height)) ||
        (rc = check_whole_image(who, ": renders", ": the re-weighting reads a pixel's neighbours", prm)) || (rc = check_spp(prm->spp)))
        return rc;
    return check_scene(c);
}

int render_cascade_device(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtCascade* cs, float* d_linear,
                          uint8_t* d_rgba, float* d_plain, float* d_weights) {
    if (!c || !cam || !prm || !cs || !d_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptcas::Levels lv;
    int rc;
    if ((rc = check_render_cascade(who, c, cam, prm, cs, &lv))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    if ((rc = check_planes(who, np, nullptr, 0, d_linear, d_rgba, d_plain))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_state(c, lv.K, np))) return rc;
    CascadePass pass;
    pass.r = resolve_args(c, lv);
    PtRenderParams p = *prm;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    if ((rc = render_impl(c, cam, &p, FilmState{}, nullptr, d_linear, d_rgba, nullptr, nullptr, &pass))) return rc;
    return reweight(c, lv, cam->width, cam->height, prm->spp, d_linear, d_rgba, d_plain, d_weights);
}

// device planes [3 k + c][np] -> the host's layer-major K * np * 3
void layers_from_planes(const std::vector<double>& planes, uint32_t K, size_t np, double* out) {
    for (uint32_t k = 0; k < K; ++k)
        for (size_t p = 0; p < np; ++p)
            for (uint32_t ch = 0; ch < 3; ++ch) out[((size_t)k * np + p) * 3 + ch] = planes[(3 * (size_t)k + ch) * np + p];
}

}  // namespace

extern "C" {

void pt_default_cascade(PtCascade* out) {
    if (!out) return;
    out->layers = 6;
    out->start = 1.0f;
    out->base = 8.0f;
    out->kappa = 1.0f;        // docs/EXPERIMENTS.md "Brightness cascade": the least plain MSE of {1, 2, 4, 8} that keeps the mean
}

int pt_debug_cascade_split(const PtCascade* cs, double L, uint32_t* j, double* w_lo, double* w_hi) {
    const char* who = "pt_debug_cascade_split";
    if (!cs || !j || !w_lo || !w_hi) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptcas::Levels lv;
    if (int rc = check_cascade(who, cs, &lv)) return rc;
    ptcas::split(lv, L, j, w_lo, w_hi);
    return PT_OK;
}

// The rule header on the CPU: the sums of every pixel in sample order, the counts, then the film pixel by pixel
int pt_cascade_host(const PtCascade* cs, uint32_t width, uint32_t height, uint32_t n, const float* samples, float* out_linear,
                    uint8_t* out_rgba, float* out_plain, double* out_layers, float* out_weights) {
    const char* who = "pt_cascade_host";
    if (!cs || !samples || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptcas::Levels lv;
    int rc;
    if ((rc = check_cascade(who, cs, &lv)) || (rc = check_image_size(who, width, height))) return rc;
    if (n == 0) return fail(PT_ERR_INVALID_ARG, "%s: n must be > 0", who);
    const size_t np = (size_t)width * height;
    if ((rc = check_planes(who, np, samples, 12 * np * n, out_linear, out_rgba, out_plain))) return rc;
    ptcas::host_film(lv, width, height, n, samples, out_linear, out_rgba, out_plain, out_layers, out_weights);
    return PT_OK;
}

// The two kernels on given samples: ceil(n / batch) launches of k_resolve_cascade, each starting from the sums the one before
// left, then k_cascade_reweight; all on the context's stream
int pt_cascade_samples_device(PtContext* c, const PtCascade* cs, uint32_t width, uint32_t height, uint32_t n, uint32_t batch,
                              const float* d_samples, float* d_linear, uint8_t* d_rgba, float* d_plain) {
    const char* who = "pt_cascade_samples_device";
    if (!cs || !d_samples || !d_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptcas::Levels lv;
    int rc;
    if ((rc = check_cascade(who, cs, &lv)) || (rc = check_image_size(who, width, height))) return rc;
    if (n == 0) return fail(PT_ERR_INVALID_ARG, "%s: n must be > 0", who);
    const size_t np = (size_t)width * height;
    if ((rc = check_planes(who, np, d_samples, 12 * np * n, d_linear, d_rgba, d_plain))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_state(c, lv.K, np))) return rc;
    const uint32_t step = batch ? std::min(batch, n) : n;
    ptk::CascadeResolveArgs r = resolve_args(c, lv);
    r.np = (uint32_t)np;
    for (uint32_t done = 0; done < n; done += step) {
        r.nb = std::min(step, n - done);
        r.lsamp = reinterpret_cast<const ptk::Rgb*>(d_samples) + (size_t)done * np;
        r.load = done > 0;
        r.finalize = done + r.nb == n;
        ptk::launch_resolve_cascade(r, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return reweight(c, lv, width, height, n, d_linear, d_rgba, d_plain, nullptr);
}

int pt_render_cascade_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtCascade* cs, float* d_linear,
                             uint8_t* d_rgba, float* d_plain) {
    return render_cascade_device("pt_render_cascade_device", c, cam, prm, cs, d_linear, d_rgba, d_plain, nullptr);
}

int pt_render_cascade_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtCascade* cs, float* out_linear,
                           uint8_t* out_rgba, float* out_plain, double* out_layers, float* out_weights) {
    const char* who = "pt_render_cascade_host";
    if (!c || !cam || !prm || !cs || !out_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptcas::Levels lv;
    int rc;
    if ((rc = check_render_cascade(who, c, cam, prm, cs, &lv))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    const uint32_t K = lv.K;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<double> planes;
    rc = render_staged(c, 3 * np, out_rgba ? 4 * np : 0, [&](float* d_linear, uint8_t* d_rgba) {
        int bad;
        if ((bad = c->cas_plain.ensure(out_plain ? 3 * np : 0)) || (bad = c->cas_weights.ensure(out_weights ? (size_t)K * np : 0))) return bad;
        return render_cascade_device(who, c, cam, prm, cs, d_linear, d_rgba, out_plain ? c->cas_plain.p : nullptr, out_weights ? c->cas_weights.p : nullptr);
    }, [&] {
        if (out_layers) planes.resize(3 * (size_t)K * np);
        return copy_back({{out_linear, c->host_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                          {out_plain, c->cas_plain.p, 3 * np * sizeof(float)}, {out_weights, c->cas_weights.p, (size_t)K * np * sizeof(float)},
                          {out_layers ? planes.data() : nullptr, c->cas_state.p, planes.size() * sizeof(double)}});
    });
    if (!rc && out_layers) layers_from_planes(planes, K, np, out_layers);
    return rc;
}

}  // extern "C"
