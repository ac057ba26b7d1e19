// pt_context.cpp -- a context's lifetime: create / destroy (the members of PtContext own their GPU resources, pt_context.h),
// stream and tuning, synchronisation and the statistics collected with it, the context-side debug entries, and the contexts
// the one-shot pt_render keeps between calls.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>

#include "pt_entry.h"
#include "pt_scene_records.h"

namespace {

// The lanes' streams are created with a priority other than the default: the runtime keeps a pool of hardware queues per
// priority level and deals a level's streams over its pool, so the lanes then never share a hardware queue with a
// default-priority stream -- the caller's, on which this library puts the resolves and its waits for the lanes.  (A wait
// sitting in a shared hardware queue holds back whatever another stream put behind it there, e.g. the next lane launch.)
#ifndef PT_LANE_PRIORITY
#define PT_LANE_PRIORITY 1        // 1: the lowest priority the device offers (resolves go first), -1: the highest, 0: default
#endif
int lane_priority() {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return 0;
    return PT_LANE_PRIORITY > 0 ? least : PT_LANE_PRIORITY < 0 ? greatest : 0;
}

// the contexts pt_render() keeps between calls (one per device it has been asked to use)
std::mutex g_render_mu;
std::vector<PtContext*> g_render_ctx;

}  // namespace

hipStream_t pt_internal_stream(PtContext* c) { return c->stream; }

// pt_shutdown at exit, registered once by whichever one-shot entry (pt_render, pt_render_multi) creates cached state first
void pt_internal_register_atexit(void) {
    static std::once_flag once;
    std::call_once(once, [] { std::atexit(pt_shutdown); });
}

extern "C" {

int pt_context_create(int device, PtContext** out) {
    if (!out) return fail(PT_ERR_INVALID_ARG, "pt_context_create: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(PT_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(PT_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<PtContext> c(new PtContext());   // a failure below frees what was created before it: the members own it
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->n_cus = (uint32_t)cus;
    }
    if (c->own_stream.create() != hipSuccess) return fail(PT_ERR_HIP, "hipStreamCreateWithFlags failed");
    c->stream = c->own_stream;
    if (c->side_stream.create() != hipSuccess) return fail(PT_ERR_HIP, "hipStreamCreateWithFlags failed");
    for (int k = 0; k < 2; ++k)
        if (c->ev_l0[k].create(false) != hipSuccess || c->ev_resolved[k].create(false) != hipSuccess)
            return fail(PT_ERR_HIP, "hipEventCreate failed");
    for (int k = 0; k < kLanes; ++k)
        if (c->lane_stream[k].create(lane_priority()) != hipSuccess || c->lane_done[k].create(false) != hipSuccess ||
            c->lane_begun[k].create(false) != hipSuccess)
            return fail(PT_ERR_HIP, "lane stream / event creation failed");
    for (int k = 0; k < kSets; ++k)
        if (c->set_free[k].create(false) != hipSuccess) return fail(PT_ERR_HIP, "hipEventCreate failed");
    if (c->ev_switch.create(false) != hipSuccess || c->ev_pre.create(false) != hipSuccess) return fail(PT_ERR_HIP, "hipEventCreate failed");
    if (c->h_posted.alloc_mapped(1) != hipSuccess) return fail(PT_ERR_HIP, "context allocation failed (mapped host word)");
    *c->h_posted.p = 0u;
    if (c->h_dstats.alloc(16) != hipSuccess || c->h_ovf.alloc(4) != hipSuccess || c->ev_begin.create(true) != hipSuccess ||
        c->ev_end.create(true) != hipSuccess)
        return fail(PT_ERR_HIP, "context allocation failed");
    *out = c.release();
    return PT_OK;
}

int pt_context_destroy(PtContext* c) {
    if (!c) return PT_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    for (int k = 0; k < kLanes; ++k) if (c->lane_stream[k]) (void)hipStreamSynchronize(c->lane_stream[k]);
    delete c;       // idle now: every member frees what it owns
    return PT_OK;
}

int pt_context_set_stream(PtContext* c, void* hip_stream) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "null context");
    hipStream_t next = hip_stream == PT_STREAM_LEGACY_DEFAULT ? nullptr                       // HIP's legacy default stream (handle 0)
                                                               : hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (next != c->stream && c->ev_switch) {
        // The context's buffers (sample buffers, counters, film sums, statistics) are handed from render to render in the order of
        // ONE stream: what is already enqueued on the old stream comes before anything the new one gets.
        (void)hipSetDevice(c->device);
        if (hipEventRecord(c->ev_switch, c->stream) == hipSuccess) (void)hipStreamWaitEvent(next, c->ev_switch, 0);
        (void)hipGetLastError();
    }
    c->stream = next;
    return PT_OK;
}

int pt_context_set_tuning(PtContext* c, const PtTuning* t) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "null context");
    c->tuning = t ? *t : PtTuning{};
    return PT_OK;
}

int pt_sync(PtContext* c) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const bool collect = c->sched.stats_pending != 0;
    bool cleared = false;
    int rc = PT_OK;
    if (collect) {
        // the device-side statistics of the renders since the last collection: read now (the stream is idle) and cleared
        // for the next ones, so that no render carries a copy or a fill of them in its stream
        HIP_TRY(hipMemcpy(c->h_dstats.p, c->ovf_count.p, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        cleared = hipMemsetAsync(c->ovf_count.p, 0, kStatsWords * sizeof(uint32_t), c->stream) == hipSuccess;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_begin, c->ev_end) == hipSuccess) c->stats.total_ms = ms;
        (void)hipGetLastError();          // (events recorded into a graph have no time)
        double kms = 0.0;
        for (uint32_t b = 0; b < c->sched.profiled; ++b)
            if (hipEventElapsedTime(&ms, c->ev_pool[2 * b], c->ev_pool[2 * b + 1]) == hipSuccess) kms += ms;
        c->stats.bounce_kernel_ms = kms;
        c->stats.shadow_rays = c->h_dstats.p[0];
        c->stats.vertices = c->h_dstats.p[1];
        c->stats.primary_vertices = c->h_dstats.p[3];
        double pms = 0.0;
        if (c->sched.profiled)
            for (uint32_t li : c->primary_events)
                if (hipEventElapsedTime(&ms, c->ev_pool[2 * li], c->ev_pool[2 * li + 1]) == hipSuccess) pms += ms;
        c->stats.primary_kernel_ms = pms;
        c->stats.max_depth_reached = (uint32_t)c->h_dstats.p[2];
        // PtStats.samples is what the DEVICE counted: a path adds one where its radiance is written to the sample buffer
        // (stats[4]).  The host's own arithmetic -- tile pixels x spp of every render enqueued -- is the expectation; a render
        // that lost or repeated work (a scheduling race, a counter cleared under a running launch) shows up here, not in a film
        // somebody has to look at.  Renders captured into graphs ran zero or more times: multiples of their size are accepted.
        const uint64_t dev = c->h_dstats.p[4], exp = c->expected_samples;
        c->stats.samples = dev;
        c->stats.samples_expected = exp;
        bool ok = dev == exp;
        if (!ok && c->capture_gcd) ok = dev >= exp && (dev - exp) % c->capture_gcd == 0;
        c->expected_samples = 0;
        if (c->h_dstats.p[7] != 0)     // a kernel found one of its own invariants violated: the film is not to be trusted
            rc = fail(PT_ERR_HIP, "internal: the exchange stacks of k_paths_regen_split overflowed (please report; PtTuning.level0_form = 1 avoids the kernel)");
        else if (!ok)
            rc = fail(PT_ERR_HIP, "internal: the device finished %llu samples where the renders since the last collection asked for %llu "
                                  "(please report; the films of these renders are not to be trusted)", (unsigned long long)dev, (unsigned long long)exp);
    }
    ptsched::on_sync(c->sched, collect, cleared);      // everything enqueued so far is complete: the buffer sets and lanes start over
    return rc;
}

// Test hook: the n-th stream operation (0-based) of the NEXT render on this context fails as if its HIP call had; < 0: none.
int pt_debug_fail_after(PtContext* c, int64_t n) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "null context");
    c->debug_fail_at = n;
    return PT_OK;
}

// Debug: the instance codes (ptk::instance_code) of the path-kernel launches enqueued since the last call, in launch order (the
// first kLaunchLogCap of them); clears the log.  *n = codes written (at most cap).
int pt_debug_launch_log(PtContext* c, uint32_t* out, uint32_t cap, uint32_t* n) {
    if (!c || !n || (!out && cap)) return fail(PT_ERR_INVALID_ARG, "null argument");
    const uint32_t k = (uint32_t)std::min<size_t>(cap, c->launch_log.size());
    std::copy(c->launch_log.begin(), c->launch_log.begin() + k, out);
    *n = k;
    c->launch_log.clear();
    return PT_OK;
}

// Debug: what one linear scan of the uploaded scene tests -- spheres, single triangles, triangle PAIRS (two consecutive
// triangles with the same v0 and plane normal share determinant, t and hit point: tripair_test).
int pt_debug_scan_layout(PtContext* c, uint32_t* n_spheres, uint32_t* n_triangles, uint32_t* n_pairs) {
    if (int rc = check_scene(c, nullptr)) return rc;
    if (n_spheres) *n_spheres = c->scan_counts[0];
    if (n_triangles) *n_triangles = c->scan_counts[1];
    if (n_pairs) *n_pairs = c->scan_counts[2];
    return PT_OK;
}

// Debug: is the scan array nothing but one run of at most kSpheresOnlyMax spheres (SceneView::spheres_only)?  With a context: the
// flag the uploaded scene carries to the kernels (objs, n unused).  Without one: what an upload of objs[0 .. n) would record, on the
// host alone (ptscene::build).
static int debug_scene_flag(const char* who, PtContext* c, const PtObject* objs, uint32_t n, uint32_t* out,
                            uint32_t ptk::SceneView::*of_view, bool ptscene::Records::*of_records) {
    if (!out) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (c) {
        if (int rc = check_scene(c, nullptr)) return rc;
        *out = c->view.*of_view;
        return PT_OK;
    }
    if (!objs && n) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptscene::Records rec;
    if (int rc = ptscene::build(objs, n, &rec)) return rc;
    *out = rec.*of_records ? 1u : 0u;
    return PT_OK;
}
int pt_debug_spheres_only(PtContext* c, const PtObject* objs, uint32_t n, uint32_t* out) {
    return debug_scene_flag("pt_debug_spheres_only", c, objs, n, out, &ptk::SceneView::spheres_only, &ptscene::Records::spheres_only);
}
// Debug, in the same two forms: can a path go on from Lambertian surfaces only -- every object Lambertian, or Emissive with a
// non-zero emission (SceneView::lambert_surfaces)?  No object: yes.
int pt_debug_lambert_surfaces(PtContext* c, const PtObject* objs, uint32_t n, uint32_t* out) {
    return debug_scene_flag("pt_debug_lambert_surfaces", c, objs, n, out, &ptk::SceneView::lambert_surfaces, &ptscene::Records::lambert_surfaces);
}

// Debug: the 16 raw device-side statistics words as last collected (pt_sync / pt_get_stats).  [0] shadow rays [1] vertices
// [2] deepest vertex [3] level-0 vertices [7] internal error flag; [8..12] only in a PT_DRAIN_TIMING measurement build.
int pt_debug_raw_stats(PtContext* c, uint64_t* out16) {
    if (!c || !out16) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (!c->h_dstats.p) return fail(PT_ERR_INVALID_ARG, "no statistics yet");
    for (int k = 0; k < 16; ++k) out16[k] = c->h_dstats.p[k];
    return PT_OK;
}

#ifdef PT_DRAIN_TIMING
// measurement build only: the per-wave records k_paths_regen left in the hand-over queue (4 words per wave)
int pt_debug_wave_dump(PtContext* c, uint32_t* out, uint32_t n_waves) {      // n_waves | lane << 31
    const uint32_t plane = n_waves >> 30; n_waves &= 0x3FFFFFFFu;      // plane = buffer set of the launch (BounceArgs.debug_tag)
    if (!c || !out || !c->ovf[0][plane].p || n_waves > c->ovf[0][plane].cap) return fail(PT_ERR_INVALID_ARG, "bad argument");
    HIP_TRY(hipMemcpy(out, c->ovf[0][plane].p, (size_t)n_waves * 16, hipMemcpyDeviceToHost));
    return PT_OK;
}
#endif

int pt_get_stats(PtContext* c, PtStats* out) {
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "null argument");
    int rc = pt_sync(c);
    if (rc) return rc;
    *out = c->stats;
    return PT_OK;
}

void pt_shutdown(void) {
    pt_internal_multi_shutdown();
    std::lock_guard<std::mutex> lk(g_render_mu);
    for (PtContext* c : g_render_ctx) pt_context_destroy(c);
    g_render_ctx.clear();
}

int pt_render(const PtCamera* cam, const PtObject* objs, uint32_t n, const PtRenderParams* prm, float* out_linear,
              uint8_t* out_rgba) {
    if (!cam || !prm || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render: null argument");
    if (prm->n_devices > 1) {
        std::vector<int> dev(prm->n_devices);
        for (uint32_t i = 0; i < prm->n_devices; ++i) dev[i] = (int)i;
        return pt_render_multi(dev.data(), prm->n_devices, cam, objs, n, prm, out_linear, out_rgba);
    }
    std::lock_guard<std::mutex> lk(g_render_mu);
    int rc;
    if (g_render_ctx.empty()) {
        PtContext* ctx = nullptr;
        if ((rc = pt_context_create(0, &ctx))) return rc;
        g_render_ctx.push_back(ctx);
        pt_internal_register_atexit();
    }
    PtContext* ctx = g_render_ctx[0];
    if ((rc = pt_scene_upload(ctx, objs, n))) return rc;
    return pt_render_host(ctx, cam, prm, out_linear, out_rgba);
}

}  // extern "C"
