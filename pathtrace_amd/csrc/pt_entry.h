// pt_entry.h -- what the entries of the C ABI share (internal to csrc/; pt_entry.cpp, the render's own checks: pt_api.cpp).
//
// The rule of an entry: it checks its arguments before it looks at the context and before any HIP call, in its own name (`who`,
// the first word of the message), and the first rule broken answers; a refused call leaves the context as it was.  A check that
// more than one host file makes stands here, once, and so do its words; a check of one feature's parameters (check_filter,
// check_cascade, check_tonemap, check_grid, the rule fields of check_bloom) stays in that feature's file.  What an entry would be
// refused for by the render behind it, it refuses with the render's function, not with a copy of its words.  The refusals that
// need no device are pinned in tests/test_entry_refusals_cpu.py and tests/test_denoise_refusals_cpu.py, the ones behind the
// context in tests/test_gpu_entry_refusals.py.
//
// A host-buffer entry is its device entry on the context's staging: render_staged below, and copy_back for the planes.
#pragma once
#include <initializer_list>

#include "pt_context.h"

// ---- planes
// p is there (unless it may be null) and a multiple of align
int check_plane(const char* who, const char* name, const void* p, uint32_t align, bool may_be_null = false);
struct Range { const void* p; size_t bytes; };            // a null p: no range
bool ranges_overlap(const Range& a, const Range& b);      // they share a byte (ranges that touch do not)
// no output shares a byte with the input read or with another output; output by output: first the input, then the outputs behind it
int check_no_alias(const char* who, std::initializer_list<Range> outputs, const Range& input);

// ---- sizes
int check_image_min(const char* who, uint32_t width, uint32_t height);        // both >= 2
int check_pixel_count(const char* who, uint32_t width, uint32_t height);      // at most 2^30 (PT_ERR_UNSUPPORTED)
int check_image_size(const char* who, uint32_t width, uint32_t height);       // the two above, in that order

// ---- the whole image: "<who><verb> the whole image (band_count = 1)<tail>"; the bakes ask band_count alone (band_index_too = false)
int check_whole_image(const char* who, const char* verb, const char* tail, const PtRenderParams* prm, bool band_index_too = true);

// ---- the render's preconditions, the functions render_impl's own check is made of (pt_api.cpp).  who: the word in front of the
// message ("<who>: "), null for none
int check_scene(const PtContext* c, const char* who = "render");              // (a null context holds no scene)
int check_camera_size(const PtCamera* cam, const char* who = nullptr);
int check_spp(uint32_t spp, const char* who = nullptr);
int check_integrator(uint32_t integrator, const char* who = nullptr);
int check_accel(uint32_t accel, const char* who = nullptr);
int check_band_index(uint32_t band_index, uint32_t band_count);

// ---- the first-hit passes over the context's ft_* scratch (pt_render_features_device, pt_probe_distances_device): rays per batch
// (108 B of scratch each with the BVH)
constexpr uint64_t kFeatureRays = 1ull << 21;

// ---- from the device to the caller's host planes
struct CopyBack { void* host; const void* dev; size_t bytes; };   // blocking, the stream is through; a null host pointer: not asked for
int copy_back(std::initializer_list<CopyBack> copies);

// The tail of a host-buffer render: the context's film staging (host_lin for lin_floats floats, host_rgba for rgba_bytes bytes; 0:
// not used), run(d_linear, d_rgba) -- the device part, which ensures the entry's further staging first --, pt_sync, then copies(),
// the entry's copy_back (made when the staging is there: ensure() may move a buffer).  The caller has set the device.
template <class Run, class Copies>
int render_staged(PtContext* c, size_t lin_floats, size_t rgba_bytes, Run&& run, Copies&& copies) {
    int rc;
    if ((rc = c->host_lin.ensure(lin_floats)) || (rc = c->host_rgba.ensure(rgba_bytes))) return rc;
    rc = run(c->host_lin.p, rgba_bytes ? c->host_rgba.p : nullptr);
    if (!rc) rc = pt_sync(c);
    return rc ? rc : copies();
}
