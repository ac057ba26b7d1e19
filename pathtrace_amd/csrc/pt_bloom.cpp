// pt_bloom.cpp -- the host side of the bloom stage (rule: pt_bloom.h): the entries, their one argument check, the
// launches of a frame's pyramid, the rule on the CPU (pt_bloom_host), and pt_display_device = bloom, then pt_tonemap_device.  The
// entries' rule and the checks they share with the other film entries: pt_entry.h.
#include <cassert>
#include <cmath>
#include <vector>

#include "pt_bloom.h"
#include "pt_entry.h"

namespace {

// planes: the addresses of the float planes of the call (null ones were refused by the caller or are optional)
int check_bloom(const char* who, uint32_t width, uint32_t height, const PtBloom* bl, const float* in, const float* out) {
    if (!bl || !in || !out) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if ((uintptr_t)in % 4u || (uintptr_t)out % 4u) return fail(PT_ERR_INVALID_ARG, "%s: the film buffers must be 4-byte aligned", who);
    if (int rc = check_image_min(who, width, height)) return rc;
    // (not check_pixel_count: this entry's code and words for the same limit differ from the other film entries', and are its ABI)
    if ((uint64_t)width * height > (1ull << 30)) return fail(PT_ERR_INVALID_ARG, "%s: %llu pixels: at most 2^30", who, (unsigned long long)width * height);
    if (bl->levels < 1u || bl->levels > pbloom::kMaxLevels) return fail(PT_ERR_INVALID_ARG, "%s: levels %u not in 1 .. 8", who, bl->levels);
    if (!std::isfinite(bl->threshold) || !(bl->threshold >= 0.0f)) return fail(PT_ERR_INVALID_ARG, "%s: threshold must be finite and >= 0", who);
    if (!std::isfinite(bl->knee) || !(bl->knee >= 0.0f)) return fail(PT_ERR_INVALID_ARG, "%s: knee must be finite and >= 0", who);
    if (!(bl->clamp > 0.0f)) return fail(PT_ERR_INVALID_ARG, "%s: clamp must be > 0 (+inf allowed)", who);
    if (!(bl->scatter >= 0.0f && bl->scatter <= 1.0f)) return fail(PT_ERR_INVALID_ARG, "%s: scatter %g not in [0, 1]", who, bl->scatter);
    if (!std::isfinite(bl->intensity) || !(bl->intensity >= 0.0f)) return fail(PT_ERR_INVALID_ARG, "%s: intensity must be finite and >= 0", who);
    return PT_OK;
}

pbloom::Rule rule_of(const PtBloom* bl) { return pbloom::rule(bl->threshold, bl->knee, bl->clamp, bl->scatter, bl->intensity); }

ptk::BloomRule kernel_rule(const pbloom::Rule& r) { return ptk::BloomRule{r.T, r.k, r.clamp, r.s, r.oms, r.intensity}; }

uint32_t tiles(uint32_t w, uint32_t tw) { return (w + tw - 1u) / tw; }

// The launches of one frame.  Checked arguments; the pyramid buffer is there.
int enqueue_bloom(PtContext* c, uint32_t W, uint32_t H, const float* d_in, const PtBloom* bl, float* d_out) {
    const pbloom::Plan p = pbloom::plan(W, H, bl->levels);
    const ptk::BloomRule r = kernel_rule(rule_of(bl));
    float* pyr = c->bloom_pyr.p;
    const uint32_t ft = c->bloom_no_tail ? p.n : p.first_tail;
    // down: the reduce kernels write D_0 .. D_(ft - 1) -- and D_0 when the tail starts there: only they read the film
    const uint32_t n_reduce = ft == 0u ? 1u : ft;
    for (uint32_t i = 0; i < n_reduce; ++i) {
        ptk::BloomReduceArgs a{};
        a.first = i == 0u;
        a.src = i == 0u ? d_in : pyr + p.off[i - 1];
        a.src_stride = i == 0u ? 0 : p.stride[i - 1];
        a.sw = i == 0u ? W : p.w[i - 1]; a.sh = i == 0u ? H : p.h[i - 1];
        a.dst = pyr + p.off[i]; a.dst_stride = p.stride[i];
        a.dw = p.w[i]; a.dh = p.h[i];
        a.tiles_x = tiles(a.dw, 16u);
        a.r = r;
        ptk::launch_bloom_reduce(a, a.tiles_x * tiles(a.dh, 16u), c->stream);
    }
    if (ft < p.n) {
        ptk::BloomTailArgs t{};
        if (ft > 0u) { t.src = pyr + p.off[ft - 1]; t.src_stride = p.stride[ft - 1]; t.sw = p.w[ft - 1]; t.sh = p.h[ft - 1]; }
        t.dst = pyr + p.off[ft]; t.dst_stride = p.stride[ft];
        t.n = p.n - ft;
        size_t texels = 0;
        for (uint32_t l = 0; l < t.n; ++l) { t.w[l] = p.w[ft + l]; t.h[l] = p.h[ft + l]; texels += (size_t)t.w[l] * t.h[l]; }
        if (texels >= pbloom::kTailTexels) return fail(PT_ERR_UNSUPPORTED, "pt_bloom_device: tail of %zu texels", texels);
        t.r = r;
        ptk::launch_bloom_tail(t, c->stream);
    }
    // up: U_i over D_i for the levels above the tail (above the last level without one), then the combine at full size
    const uint32_t top = ft < p.n ? ft : p.n - 1u;            // U_top is in place
    for (uint32_t i = top; i-- > 0u;) {
        ptk::BloomExpandArgs a{};
        a.coarse = pyr + p.off[i + 1]; a.coarse_stride = p.stride[i + 1]; a.cw = p.w[i + 1]; a.ch = p.h[i + 1];
        a.fine = pyr + p.off[i]; a.fine_stride = p.stride[i];
        a.w = p.w[i]; a.h = p.h[i];
        a.tiles_x = tiles(a.w, 32u);
        a.r = r;
        ptk::launch_bloom_expand(a, a.tiles_x * tiles(a.h, 8u), c->stream);
    }
    ptk::BloomExpandArgs a{};
    a.coarse = pyr + p.off[0]; a.coarse_stride = p.stride[0]; a.cw = p.w[0]; a.ch = p.h[0];
    a.film = d_in; a.out = d_out; a.last = 1u;
    a.w = W; a.h = H;
    a.tiles_x = tiles(W, 32u);
    a.r = r;
    ptk::launch_bloom_expand(a, a.tiles_x * tiles(H, 8u), c->stream);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// A grid is tiles x 256 threads and must stay below 2^32 threads: only an image two or three pixels wide or high and of some 2^29
// pixels reaches that.  Refused before anything is allocated.
int check_grid(const char* who, uint32_t W, uint32_t H) {
    const uint64_t reduce0 = (uint64_t)tiles(pbloom::half_up(W), 16u) * tiles(pbloom::half_up(H), 16u);
    const uint64_t last = (uint64_t)tiles(W, 32u) * tiles(H, 8u);
    if (reduce0 >= (1ull << 24) || last >= (1ull << 24)) return fail(PT_ERR_UNSUPPORTED, "%s: image %ux%u needs more than 2^24 tiles", who, W, H);
    return PT_OK;
}

int bloom_device(const char* who, PtContext* c, uint32_t W, uint32_t H, const float* d_in, const PtBloom* bl, float* d_out) {
    int rc;
    if ((rc = check_grid(who, W, H))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->bloom_pyr.ensure(pbloom::plan(W, H, pbloom::kMaxLevels).total))) return rc;   // by size alone: no level count regrows it
    return enqueue_bloom(c, W, H, d_in, bl, d_out);
}

// level planes of the host: three vectors per level
struct HostLevel {
    uint32_t w = 0, h = 0;
    std::vector<float> ch[3];
};

}  // namespace

extern "C" {

void pt_default_bloom(PtBloom* out) {
    if (!out) return;
    out->levels = 6; out->threshold = 1.0f; out->knee = 0.5f; out->clamp = INFINITY; out->scatter = 0.7f; out->intensity = 0.05f;
}

int pt_bloom_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const PtBloom* bl, float* d_out_linear) {
    const char* who = "pt_bloom_device";
    int rc;
    if ((rc = check_bloom(who, width, height, bl, d_linear, d_out_linear))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    return bloom_device(who, c, width, height, d_linear, bl, d_out_linear);
}

int pt_display_device(PtContext* c, uint32_t width, uint32_t height, const float* d_linear, const PtBloom* bl, const PtTonemap* tm,
                      float* d_out_linear, uint8_t* d_out_rgba) {
    const char* who = "pt_display_device";
    if (!bl) return pt_tonemap_device(c, width, height, d_linear, tm, d_out_linear, d_out_rgba);
    // both stages' checks before the context is touched: a refused call leaves no half-done frame
    int rc;
    if ((rc = check_bloom(who, width, height, bl, d_linear, d_linear))) return rc;
    if ((rc = tonemap_check_args(who, width, height, d_linear, tm, d_out_linear, d_out_rgba))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    if ((rc = check_grid(who, width, height))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->bloom_lin.ensure(3 * (size_t)width * height))) return rc;
    if ((rc = bloom_device(who, c, width, height, d_linear, bl, c->bloom_lin.p))) return rc;
    return pt_tonemap_device(c, width, height, c->bloom_lin.p, tm, d_out_linear, d_out_rgba);
}

// pt_display_device on host planes (blocking), staged as pt_tonemap_host stages its film
int pt_display_host(PtContext* c, uint32_t width, uint32_t height, const float* linear, const PtBloom* bl, const PtTonemap* tm, float* out_linear,
                    uint8_t* out_rgba) {
    const char* who = "pt_display_host";
    int rc;
    if (bl && (rc = check_bloom(who, width, height, bl, linear, linear))) return rc;
    if ((rc = tonemap_check_args(who, width, height, linear, tm, out_linear, out_rgba))) return rc;
    if (!c) return fail(PT_ERR_INVALID_ARG, "%s: null context", who);
    const size_t np = (size_t)width * height;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->tone.lin.ensure(3 * np)) || (rc = c->tone.rgba.ensure(4 * np))) return rc;
    HIP_TRY(hipMemcpyAsync(c->tone.lin.p, linear, 3 * np * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if ((rc = pt_display_device(c, width, height, c->tone.lin.p, bl, tm, c->tone.lin.p, c->tone.rgba.p))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));      // (as pt_tonemap_host: not pt_sync)
    return copy_back({{out_linear, c->tone.lin.p, 3 * np * sizeof(float)}, {out_rgba, c->tone.rgba.p, 4 * np}});
}

int pt_bloom_host(uint32_t width, uint32_t height, const float* linear, const PtBloom* bl, float* out) {
    int rc;
    if ((rc = check_bloom("pt_bloom_host", width, height, bl, linear, out))) return rc;
    const pbloom::Plan p = pbloom::plan(width, height, bl->levels);
    const pbloom::Rule r = rule_of(bl);
    const size_t np = (size_t)width * height;
    std::vector<HostLevel> lv(p.n);
    // the bright pass of every pixel, planar: the source of level 0
    HostLevel film;
    film.w = width; film.h = height;
    for (auto& pl : film.ch) pl.resize(np);
    for (size_t i = 0; i < np; ++i) {
        float b[3];
        pbloom::bright(r, linear[3 * i], linear[3 * i + 1], linear[3 * i + 2], b);
        for (int c = 0; c < 3; ++c) film.ch[c][i] = b[c];
    }
    for (uint32_t l = 0; l < p.n; ++l) {
        const HostLevel& src = l == 0u ? film : lv[l - 1];
        HostLevel& dst = lv[l];
        dst.w = p.w[l]; dst.h = p.h[l];
        assert(dst.w == pbloom::half_up(src.w) && dst.h == pbloom::half_up(src.h));   // rule 4: j >> 1 never passes the coarse plane
        for (int c = 0; c < 3; ++c) {
            dst.ch[c].resize((size_t)dst.w * dst.h);
            const float* plane = src.ch[c].data();
            const uint32_t sw = src.w;
            const auto at = [plane, sw](uint32_t x, uint32_t y) { return plane[(size_t)y * sw + x]; };
            for (uint32_t y = 0; y < dst.h; ++y)
                for (uint32_t x = 0; x < dst.w; ++x) dst.ch[c][(size_t)y * dst.w + x] = pbloom::reduce_at(at, src.w, src.h, x, y);
        }
    }
    for (uint32_t l = p.n - 1u; l-- > 0u;) {
        HostLevel& fine = lv[l];
        const HostLevel& coarse = lv[l + 1];
        for (int c = 0; c < 3; ++c) {
            const float* plane = coarse.ch[c].data();
            const uint32_t cw = coarse.w;
            const auto at = [plane, cw](uint32_t x, uint32_t y) { return plane[(size_t)y * cw + x]; };
            for (uint32_t y = 0; y < fine.h; ++y)
                for (uint32_t x = 0; x < fine.w; ++x) {
                    float& d = fine.ch[c][(size_t)y * fine.w + x];
                    d = pbloom::collect(r, d, pbloom::expand_at(at, coarse.w, coarse.h, x, y));
                }
        }
    }
    for (int c = 0; c < 3; ++c) {
        const float* plane = lv[0].ch[c].data();
        const uint32_t cw = lv[0].w;
        const auto at = [plane, cw](uint32_t x, uint32_t y) { return plane[(size_t)y * cw + x]; };
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                const size_t i = 3 * ((size_t)y * width + x) + c;
                out[i] = pbloom::combine(r, linear[i], pbloom::expand_at(at, lv[0].w, lv[0].h, x, y));
            }
    }
    return PT_OK;
}

int pt_debug_bloom_plan(uint32_t width, uint32_t height, uint32_t levels, uint32_t* out_wh, uint32_t* n_levels, uint32_t* first_tail_level) {
    if (!out_wh || !n_levels || !first_tail_level) return fail(PT_ERR_INVALID_ARG, "pt_debug_bloom_plan: null argument");
    if (width < 2 || height < 2 || (uint64_t)width * height > (1ull << 30) || levels < 1u || levels > pbloom::kMaxLevels)
        return fail(PT_ERR_INVALID_ARG, "pt_debug_bloom_plan: image %ux%u, levels %u", width, height, levels);
    const pbloom::Plan p = pbloom::plan(width, height, levels);
    for (uint32_t i = 0; i < p.n; ++i) { out_wh[2 * i] = p.w[i]; out_wh[2 * i + 1] = p.h[i]; }
    *n_levels = p.n;
    *first_tail_level = p.first_tail;
    return PT_OK;
}

int pt_debug_bloom_bright(const PtBloom* bl, const float* rgb, float* out_b) {
    int rc;
    if ((rc = check_bloom("pt_debug_bloom_bright", 2, 2, bl, rgb, out_b))) return rc;
    pbloom::bright(rule_of(bl), rgb[0], rgb[1], rgb[2], out_b);
    return PT_OK;
}

int pt_debug_bloom_tail(PtContext* c, int enable) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_debug_bloom_tail: null context");
    c->bloom_no_tail = enable == 0;
    return PT_OK;
}

}  // extern "C"
