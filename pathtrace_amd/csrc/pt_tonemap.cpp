// pt_tonemap.cpp -- the host side of the display transform (rule: pt_tonemap.h): the film's luminance histogram,
// the exposure the context adapts over frames, the curve and the transfer.  The entries' rule and the checks they share with the
// other film entries: pt_entry.h.
#include <cmath>
#include <cstring>

#include "pt_entry.h"
#include "pt_tonemap.h"

int TonemapState::ensure(hipStream_t st) {
    if (state.p) return PT_OK;
    int rc;
    if ((rc = hist.ensure(ptone::kWords))) return rc;
    HIP_TRY(hipMemsetAsync(hist.p, 0, ptone::kWords * sizeof(uint32_t), st));
    if ((rc = state.ensure(1))) return rc;
    HIP_TRY(hipMemsetAsync(state.p, 0, sizeof(ptk::ExposureState), st));   // all zero: no exposure yet
    return PT_OK;
}

namespace {

int check_film(const char* who, uint32_t width, uint32_t height, const float* d_linear) {
    if (!d_linear) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((uintptr_t)d_linear % 4u) return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    return check_image_size(who, width, height);
}

bool in_unit(float v) { return v >= 0.0f && v <= 1.0f; }      // false for NaN

int check_tonemap(const char* who, const PtTonemap* tm) {
    if (tm->mode > PT_EXPOSURE_MANUAL) return fail(PT_ERR_INVALID_ARG, "%s: unknown mode %u", who, tm->mode);
    if (tm->curve > PT_CURVE_ACES) return fail(PT_ERR_INVALID_ARG, "%s: unknown curve %u", who, tm->curve);
    if (tm->transfer > PT_TRANSFER_SRGB) return fail(PT_ERR_INVALID_ARG, "%s: unknown transfer %u", who, tm->transfer);
    if (!std::isfinite(tm->ev)) return fail(PT_ERR_INVALID_ARG, "%s: ev must be finite", who);
    if (!in_unit(tm->pct_lo) || !in_unit(tm->pct_hi) || tm->pct_lo > tm->pct_hi)
        return fail(PT_ERR_INVALID_ARG, "%s: pct_lo %g and pct_hi %g must satisfy 0 <= pct_lo <= pct_hi <= 1", who, tm->pct_lo, tm->pct_hi);
    if (!(tm->key > 0.0f) || !std::isfinite(tm->key) || !(tm->white > 0.0f) || !std::isfinite(tm->white))
        return fail(PT_ERR_INVALID_ARG, "%s: key and white must be finite and > 0", who);
    if (!in_unit(tm->adapt)) return fail(PT_ERR_INVALID_ARG, "%s: adapt %g not in [0, 1]", who, tm->adapt);
    if (!(tm->log2_min <= tm->log2_max)) return fail(PT_ERR_INVALID_ARG, "%s: log2_min %g above log2_max %g", who, tm->log2_min, tm->log2_max);
    return PT_OK;
}

}  // namespace

// what pt_tonemap_device refuses before it looks at the context (pt_display_device asks the same in front of its bloom stage)
int tonemap_check_args(const char* who, uint32_t width, uint32_t height, const float* d_linear, const PtTonemap* tm, const float* d_out_linear,
                       const uint8_t* d_out_rgba) {
    if (!tm || !d_out_rgba) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_film(who, width, height, d_linear))) return rc;
    if ((uintptr_t)d_out_linear % 4u || (uintptr_t)d_out_rgba % 4u) return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    return check_tonemap(who, tm);
}

extern "C" {

void pt_default_tonemap(PtTonemap* out) {
    if (!out) return;
    out->mode = PT_EXPOSURE_AUTO; out->curve = PT_CURVE_ACES; out->transfer = PT_TRANSFER_SQRT;
    out->ev = 0.0f; out->key = 0.18f;
    out->pct_lo = 0.5f; out->pct_hi = 0.95f;
    out->log2_min = -8.0f; out->log2_max = 8.0f;
    out->adapt = 0.1f; out->white = 4.0f;
}

int pt_film_histogram_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, uint32_t* d_hist) {
    const char* who = "pt_film_histogram_device";
    if (!d_hist) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_film(who, width, height, d_linear))) return rc;
    if ((uintptr_t)d_hist % 4u) return fail(PT_ERR_INVALID_ARG, "%s: d_hist258 must be 4-byte aligned", who);
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(d_hist, 0, ptone::kWords * sizeof(uint32_t), c->stream));
    ptk::launch_film_histogram(d_linear, width * height, d_hist, c->n_cus, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int pt_tonemap_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const PtTonemap* tm, float* d_out_linear,
                      uint8_t* d_out_rgba) {
    const char* who = "pt_tonemap_device";
    int rc;
    if ((rc = tonemap_check_args(who, width, height, d_linear, tm, d_out_linear, d_out_rgba))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    HIP_TRY(hipSetDevice(c->device));
    ptk::TonemapArgs t{};
    t.linear = d_linear; t.out_linear = d_out_linear; t.out_rgba = d_out_rgba;
    t.np = width * height; t.curve = tm->curve; t.transfer = tm->transfer; t.white = tm->white;
    if (tm->mode == PT_EXPOSURE_MANUAL) {
        t.e_manual = (float)std::exp2((double)tm->ev);
    } else {
        if ((rc = c->tone.ensure(c->stream))) return rc;
        HIP_TRY(hipMemsetAsync(c->tone.hist.p, 0, ptone::kWords * sizeof(uint32_t), c->stream));
        ptk::launch_film_histogram(d_linear, t.np, c->tone.hist.p, c->n_cus, c->stream);
        ptk::ExposureArgs e{};
        e.hist = c->tone.hist.p; e.state = c->tone.state.p; e.width = width; e.height = height;
        e.pct_lo = tm->pct_lo; e.pct_hi = tm->pct_hi; e.key = tm->key; e.log2_min = tm->log2_min; e.log2_max = tm->log2_max; e.adapt = tm->adapt;
        ptk::launch_exposure_meter(e, c->stream);
        t.e_dev = &c->tone.state.p->E;
    }
    ptk::launch_tonemap(t, c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// pt_tonemap_device on host planes (blocking): the film is staged on the device and mapped in place
int pt_tonemap_host(PtContext* c, uint32_t width, uint32_t height, const float* linear, const PtTonemap* tm, float* out_linear, uint8_t* out_rgba) {
    const char* who = "pt_tonemap_host";
    if (!tm || !out_rgba) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    if ((rc = check_film(who, width, height, linear)) || (rc = check_tonemap(who, tm))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    const size_t np = (size_t)width * height;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->tone.lin.ensure(3 * np)) || (rc = c->tone.rgba.ensure(4 * np))) return rc;
    HIP_TRY(hipMemcpyAsync(c->tone.lin.p, linear, 3 * np * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = pt_tonemap_device(c, width, height, c->tone.lin.p, tm, c->tone.lin.p, c->tone.rgba.p))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // (not pt_sync: no render ran, there are no statistics to collect)
    return copy_back({{out_linear, c->tone.lin.p, 3 * np * sizeof(float)}, {out_rgba, c->tone.rgba.p, 4 * np}});
}

// On the stream, like the frames around it: a context that has not metered yet has nothing to forget.
int pt_exposure_reset(PtContext* c) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_exposure_reset: null context");
    if (!c->tone.state.p) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->tone.state.p, 0, sizeof(ptk::ExposureState), c->stream));
    return PT_OK;
}

int pt_debug_exposure_state(PtContext* c, double* log2E, float* E, uint32_t* valid, uint32_t* hist) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_debug_exposure_state: null context");
    ptk::ExposureState s{};
    if (hist) std::memset(hist, 0, ptone::kWords * sizeof(uint32_t));
    if (c->tone.state.p) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(&s, c->tone.state.p, sizeof(s), hipMemcpyDeviceToHost));
        if (hist) HIP_TRY(hipMemcpy(hist, c->tone.hist.p, ptone::kWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (log2E) *log2E = s.log2E;
    if (E) *E = s.valid ? s.E : 1.0f;
    if (valid) *valid = s.valid;
    return PT_OK;
}

int pt_exposure_get(PtContext* c, double* log2E, uint32_t* hist) {
    if (!c || !log2E) return fail(PT_ERR_INVALID_ARG, "pt_exposure_get: null argument");
    return pt_debug_exposure_state(c, log2E, nullptr, nullptr, hist);
}

uint32_t pt_debug_tonemap_bin(float L) { return ptone::word(L); }

double pt_debug_tonemap_meter(const uint32_t* hist, const PtTonemap* tm, int fresh, double log2E_prev) {
    if (!hist || !tm) return std::nan("");
    return ptone::meter(hist, tm->pct_lo, tm->pct_hi, tm->key, tm->log2_min, tm->log2_max, tm->adapt, fresh != 0, log2E_prev);
}

int pt_debug_tonemap_pixel(const PtTonemap* tm, float E, const float* rgb, float* out_y, uint8_t* out_rgba) {
    if (!tm || !rgb || !out_y || !out_rgba) return fail(PT_ERR_INVALID_ARG, "pt_debug_tonemap_pixel: null argument");
    int rc;
    if ((rc = check_tonemap("pt_debug_tonemap_pixel", tm))) return rc;
    ptone::curve(tm->curve, E, tm->white, rgb, out_y);
    const uint32_t q8 = ptone::rgba8(tm->transfer, out_y);
    std::memcpy(out_rgba, &q8, 4);
    return PT_OK;
}

}  // extern "C"
