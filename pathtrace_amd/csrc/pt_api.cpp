// pt_api.cpp -- the wavefront render driver (render_impl) and the entries of the C ABI (include/pathtrace_amd.h) that are thin
// callers of it.  The context and what the host files share: pt_context.h.
//
// render() == everything src/main.rs:43-60 does: enumerate the tile's pixels, give
// every pixel the RNG key (x, y) (main.rs:51), run SAMPLE_NUM paths per pixel
// (world.rs:296) and fill the two film buffers (world.rs:55-57).  Here the pixel
// x sample loop is a queue of paths in HBM advanced one vertex per kernel launch.
//
// There is no CPU fallback: without a HIP device every rendering entry point
// fails with PT_ERR_NO_DEVICE.
#include <algorithm>
#include <cstring>

#include "pt_entry.h"
#include "pt_shape.h"

// ---- the render's preconditions (pt_entry.h): each message stands here and nowhere else.  who: "<who>: " in front, null: nothing
#define PT_WHO(who) (who) ? (who) : "", (who) ? ": " : ""
int check_scene(const PtContext* c, const char* who) {
    if (!c || !c->has_scene) return fail(PT_ERR_INVALID_ARG, "%s%sno scene uploaded", PT_WHO(who));
    return PT_OK;
}
int check_camera_size(const PtCamera* cam, const char* who) {   // get_ray_with_offset divides by width-1 / height-1 (camera.rs:140-141)
    if (cam->width < 2 || cam->height < 2)
        return fail(PT_ERR_INVALID_ARG, "%s%scamera %ux%u: width and height must be >= 2", PT_WHO(who), cam->width, cam->height);
    return PT_OK;
}
int check_spp(uint32_t spp, const char* who) {
    if (spp == 0) return fail(PT_ERR_INVALID_ARG, "%s%sspp must be > 0", PT_WHO(who));
    return PT_OK;
}
int check_integrator(uint32_t integrator, const char* who) {
    if (integrator > PT_INTEGRATOR_BRDF_ONLY) return fail(PT_ERR_INVALID_ARG, "%s%sunknown integrator %u", PT_WHO(who), integrator);
    return PT_OK;
}
int check_accel(uint32_t accel, const char* who) {
    if (accel > PT_ACCEL_AUTO) return fail(PT_ERR_INVALID_ARG, "%s%sunknown accel %u", PT_WHO(who), accel);
    return PT_OK;
}
int check_band_index(uint32_t band_index, uint32_t band_count) {
    if (band_index >= band_count) return fail(PT_ERR_INVALID_ARG, "band_index %u >= band_count %u", band_index, band_count);
    return PT_OK;
}
#undef PT_WHO

namespace {

using ptshape::kCountStride;
using ptshape::kDefaultMaxPaths;
constexpr size_t kLaunchLogCap = 1u << 16;       // pt_debug_launch_log keeps this many codes between two reads

int ensure_events(PtContext* c, size_t n) {
    while (c->ev_pool.size() < n) {
        Event e;
        HIP_TRY(e.create(true));
        c->ev_pool.push_back(std::move(e));
    }
    return PT_OK;
}

// ---- the launch scheduler: plan (pt_sched.h, pure) -> execute (here) -> commit
hipStream_t sched_stream(const PtContext* c, hipStream_t caller, uint32_t id) {
    return id == ptsched::kStreamCaller ? caller : id == ptsched::kStreamSide ? c->side_stream : c->lane_stream[id - ptsched::kStreamLane0];
}
hipEvent_t sched_event(const PtContext* c, const ptsched::Op& o) {
    using namespace ptsched;
    const uint32_t e = o.event;
    if (e == kEvBegin) return c->ev_begin;
    if (e == kEvEnd) return c->ev_end;
    if (e == kEvPre) return c->ev_pre;
    if (e >= kEvL0 && e < kEvResolved) return c->ev_l0[e - kEvL0];
    if (e >= kEvResolved && e < kEvLaneDone) return c->ev_resolved[e - kEvResolved];
    if (e >= kEvLaneDone && e < kEvLaneBegun) return c->lane_done[e - kEvLaneDone];
    if (e >= kEvLaneBegun && e < kEvSetFree) return c->lane_begun[e - kEvLaneBegun];
    if (e >= kEvSetFree && e < kEvPool) return c->set_free[e - kEvSetFree];
    return c->ev_pool[o.pool];
}

// An operation of a render could not be enqueued: what was enqueued before it runs to its end (or fails with the device), then
// the scheduling state starts over with nothing known to be clean (ptsched::on_failure).  The render's outputs are undefined;
// the statistics of the renders since the last collection are dropped with it.
void sched_recover(PtContext* c, hipStream_t st, const ptsched::State& planned) {
    for (int k = 0; k < kLanes; ++k) (void)hipStreamSynchronize(c->lane_stream[k]);
    (void)hipStreamSynchronize(c->side_stream);
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    ptsched::on_failure(c->sched, planned);
    c->expected_samples = 0;
    if (c->ovf_count.p && hipMemsetAsync(c->ovf_count.p, 0, kStatsWords * sizeof(uint32_t), st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
        c->sched.stats_clean = 1;
    (void)hipGetLastError();
}

// render_impl into the context's device staging, then over PCIe into the caller's host buffers (blocking)
int film_back(const PtContext* c, size_t np, float* out_linear, uint8_t* out_rgba) {
    return copy_back({{out_linear, c->host_lin.p, np * 3 * sizeof(float)}, {out_rgba, c->host_rgba.p, np * 4}});
}
int render_to_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const FilmState& fs, const ListRender* list,
                   size_t np, float* out_linear, uint8_t* out_rgba) {
    if (np == 0) return render_impl(c, cam, prm, fs, list, nullptr, nullptr);   // validates, renders nothing
    HIP_TRY(hipSetDevice(c->device));
    return render_staged(c, np * 3, out_rgba ? np * 4 : 0, [&](float* d_linear, uint8_t* d_rgba) { return render_impl(c, cam, prm, fs, list, d_linear, d_rgba); },
                         [&] { return film_back(c, np, out_linear, out_rgba); });
}
size_t tile_pixels(const PtCamera* cam, const PtRenderParams* prm) {
    return (size_t)pt_tile_rows(cam->height, prm->band_rows, prm->band_index, prm->band_count ? prm->band_count : 1) * cam->width;
}

// ---- render_impl's stages, in the order it runs them

// Statistics belong to the renders enqueued since they were last collected (pt_sync / pt_get_stats): a caller that
// pipelines several renders behind one synchronisation gets their sums (vertices, launches, kernel times), total_ms from
// the first one's start to the last one's end.  One render per synchronisation: the statistics of that render, as ever.
void begin_period(PtContext* c) {        // the first render since the last collection
    std::memset(&c->stats, 0, sizeof c->stats);
    c->primary_events.clear();
    c->expected_samples = 0;
}

// CHECK: the pieces (pt_entry.h; above the namespace) in render_impl's order.  No camera is checked where the paths are given and
// no camera ray is generated.
int check_render(const PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const ListRender* list, const float* d_linear,
                 const uint8_t* d_rgba) {
    if (!c || !cam || !prm) return fail(PT_ERR_INVALID_ARG, "render: null argument");
    const bool given = list && list->inject[0] && (!list->tile || list->no_camera);
    const uint32_t band_count = prm->band_count ? prm->band_count : 1;
    int rc;
    if ((rc = check_scene(c)) || (!given && (rc = check_camera_size(cam))) || (rc = check_spp(prm->spp)) || (rc = check_integrator(prm->integrator)) ||
        (rc = check_accel(prm->accel)) || (rc = check_band_index(prm->band_index, band_count)))
        return rc;
    if (list && !list->tile && band_count != 1) return fail(PT_ERR_INVALID_ARG, "pixel-list renders take the whole image (band_count = 1)");
    // the resolve stores a pixel's RGBA8 as one 32-bit word (a byte-offset pointer would fault on the device)
    if (d_rgba && (uintptr_t)d_rgba % 4u) return fail(PT_ERR_INVALID_ARG, "render: the RGBA8 output buffer must be 4-byte aligned");
    if (d_linear && (uintptr_t)d_linear % 4u) return fail(PT_ERR_INVALID_ARG, "render: the linear output buffer must be 4-byte aligned");
    return PT_OK;
}

// ACCEL: PT_ACCEL_AUTO -> what actually runs
uint32_t resolve_accel(PtContext* c, uint32_t accel) {
    if (accel != PT_ACCEL_AUTO) return accel;
    if (c->auto_bvh && c->tree.may_build()) {
        const std::string keep = g_err;              // a refused BVH is not an error of this call
        if (ensure_bvh(c) == PT_OK) return PT_ACCEL_BVH;
        g_err = keep;
    }
    return PT_ACCEL_LINEAR;
}

// SIZE: the level-0 form, the batches and every grid, segment and queue size (pt_shape.h, pure).  The two things it needs from
// the runtime are asked for here: whether the caller's stream is being captured, and -- once per scene and kernel, for scenes
// that take a regenerating form -- that kernel's occupancy with the scene's LDS blob.
int size_render(PtContext* c, const PtRenderParams* prm, const ListRender* list, uint64_t np64, ptshape::Shape* shape) {
    ptshape::In in{};
    in.np = np64; in.max_paths_in_flight = prm->max_paths_in_flight;
    in.spp = prm->spp; in.workgroups = prm->workgroups; in.accel = prm->accel; in.profile = prm->profile;
    in.list = list != nullptr; in.list_regen = list && list->regen; in.inject = list && list->inject[0];
    in.inject_spp = list ? list->inject_spp : 0u;
    in.n_objs = c->view.n_objs; in.blob_f4 = c->view.blob_f4; in.diffuse_only = c->view.diffuse_only;
    in.split_ok = c->split_ok; in.n_cus = c->n_cus;
    in.export_below = c->tuning.export_below; in.cont_workgroups = c->tuning.cont_workgroups; in.level0_form = c->tuning.level0_form;
    in.regen_workgroups = c->tuning.regen_workgroups; in.in_order = c->tuning.in_order;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        in.capturing = !(hipStreamIsCapturing(c->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone);
        (void)hipGetLastError();
    }
    const ptshape::Form f = ptshape::form(in);
    uint32_t* const occ = f.regen_scene ? &c->regen_occ[prm->exact_math ? 1 : 0][prm->integrator ? 1 : 0][f.split ? 1 : 0] : nullptr;   // per scene (pt_scene_upload clears it)
    *shape = ptshape::shape(in, f, occ ? *occ : 0u);
    if (shape->over_cap)
        return fail(PT_ERR_UNSUPPORTED, "tile of %llu pixels exceeds max_paths_in_flight %llu; use more bands",
                    (unsigned long long)np64, (unsigned long long)shape->cap);
    if (occ && *occ == 0u) {           // not asked yet (a refused tile never asks): the answer sizes this render and is kept
        ptk::BounceArgs q{};
        q.sc = view_for(c, prm->exact_math);
        q.integrator = prm->integrator;
        q.xchg = f.split ? reinterpret_cast<float4*>(1) : nullptr;       // selects the kernel only
        *occ = prm->exact_math ? ptk::regen_blocks_per_cu_exact(q) : ptk::regen_blocks_per_cu_fast(q);
        if (*occ != 0u) *shape = ptshape::shape(in, f, *occ);
    }
    return PT_OK;
}

// PREPARE: every buffer the render will touch, before anything is enqueued.  May turn the job into its in-order form.
int prepare(PtContext* c, const PtRenderParams* prm, const FilmState& fs, const ptshape::Shape& sh, ptsched::Job& job) {
    int rc;
    if (prm->accel && (rc = ensure_bvh(c))) return rc;
    for (int k = 0; k < 4; ++k)
        if ((rc = c->queue[k].ensure(sh.q_slots))) return rc;
    if (prm->accel && ((rc = c->bvh_aux.ensure(sh.q_slots)) || (rc = c->bvh_sray[0].ensure(sh.q_slots)) ||
                       (rc = c->bvh_sray[1].ensure(sh.q_slots))))
        return rc;
    {
        // The buffer sets the render rotates through (with lanes: up to three sample buffers of 12 B per path in flight -- 3 x 3.2 GB
        // for the reference's 400 x 400 x 3000 job at the default cap).  All of them now: an allocation in the middle of the batch
        // loop would drain the pipeline the lanes keep full, and fail with half of the render enqueued.  If the device cannot hold
        // them, the render falls back to ONE set and launches in order -- slower, same film -- instead of failing.
        uint32_t sets[4], n_sets = 0;
        ptsched::sets_of(c->sched, job, sets, &n_sets);
        for (uint32_t k = 0; k < n_sets; ++k) {
            rc = c->lsamp[sets[k]].ensure(sh.n_paths_max);
            if (rc == PT_ERR_OOM && ptsched::takes_lanes(job)) {
                job.in_order = 1;
                ptsched::sets_of(c->sched, job, sets, &n_sets);
                k = (uint32_t)-1;                       // start over with the one set of the in-order form
                continue;
            }
            if (rc) return rc;
        }
    }
    if (sh.overlap && sh.hand_off)
        for (int k = 0; k < 4; ++k)
            if ((rc = c->cqueue[k].ensure(sh.q_slots_cont))) return rc;
    if (sh.overlap && sh.hand_off && prm->accel && ((rc = c->caux.ensure(sh.q_slots_cont)) || (rc = c->csray[0].ensure(sh.q_slots_cont)) ||
                                                    (rc = c->csray[1].ensure(sh.q_slots_cont))))
        return rc;
    if (!c->ovf_count.p) {             // [render statistics | launch counters of buffer set 0 | 1 | ...], zero from the start
        if ((rc = c->ovf_count.ensure(kStatsWords + kSets * kCountStride))) return rc;
        // (on the caller's stream and waited for: a plain hipMemset runs on the legacy default stream, which the context's
        // non-blocking streams do not wait for -- the first render's counts raced with it, caught by pt_sync's own sample check)
        HIP_TRY(hipMemsetAsync(c->ovf_count.p, 0, (kStatsWords + kSets * kCountStride) * sizeof(uint32_t), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->sched.stats_clean = 1;
        for (int k = 0; k < kSets; ++k) c->sched.counters_clean[k] = 1;
    }
    if (sh.hand_off)
        for (int par = 0; par < (sh.overlap ? 2 : 1); ++par)
            for (int k = 0; k < 4; ++k)
                if ((rc = c->ovf[par][k].ensure(sh.ovf_slots))) return rc;
    if ((sh.n_batches > 1 || fs.load || fs.store) && (rc = c->film.ensure((size_t)sh.np * 3))) return rc;
    return PT_OK;
}

// tile row -> image row without a table (ptk::TileMap)
ptk::TileMap tile_map(const PtCamera* cam, const PtRenderParams* prm) {
    ptk::TileMap t{};
    const uint32_t br = prm->band_rows ? prm->band_rows : cam->height;
    t.band_rows = br;
    t.band_magic = br > 1 ? (uint32_t)(((1ull << 32) + br - 1) / br) : 0u;
    t.band_stride = br * (prm->band_count ? prm->band_count : 1);
    t.band_first = prm->band_index * br;
    return t;
}
uint32_t magic_of(uint32_t d) { return d <= 1u ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / d); }   // floor(2^32 / d) (divmod_magic)

// ARGS: the words of BounceArgs that are the same for every launch of the render
ptk::BounceArgs bounce_args(const PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const ListRender* list, uint32_t np) {
    ptk::BounceArgs a{};
    a.stats = reinterpret_cast<unsigned long long*>(c->ovf_count.p);   // hipMalloc alignment: fine for u64
    const bool tile = !list || list->tile;       // the film is the camera's tile (else: the list's slots)
    if (tile) a.tile = tile_map(cam, prm);
    a.sc = view_for(c, prm->exact_math);
    for (int k = 0; k < 3; ++k) {
        a.cam.origin[k] = (float)cam->origin[k]; a.cam.lower_left[k] = (float)cam->lower_left[k];
        a.cam.horizontal[k] = (float)cam->horizontal[k]; a.cam.vertical[k] = (float)cam->vertical[k];
    }
    a.cam.width = cam->width; a.cam.height = cam->height;
    a.pixels = tile ? nullptr : list->d_pixels;
    a.film_w = tile ? cam->width : 65536u;
    a.np = np;
    a.film_w_magic = magic_of(a.film_w);
    a.np_magic = magic_of(np);
    a.min_depth = prm->min_depth; a.max_depth = prm->max_depth;
    a.t_min = (float)prm->t_min;
    a.integrator = prm->integrator;
    a.accel = prm->accel;
    a.bvh_refill = c->tuning.bvh_refill ? std::min(64u, c->tuning.bvh_refill) : ptk::kRefillBelow;
    a.bvh_leaf = c->tuning.bvh_leaf ? c->tuning.bvh_leaf : ptk::kLeafBatch;
    return a;
}

// EXECUTE: what the operations of one render read, and what its launches leave for the commit
struct Exec {
    PtContext* c;
    const PtCamera* cam;
    const PtRenderParams* prm;         // accel resolved
    const FilmState& fs;
    const ListRender* list;
    const AdaptivePass* ad;
    const CascadePass* cas;
    const FilterPass* flt;
    float* d_linear;
    uint8_t* d_rgba;
    void* d_packed;
    const ptshape::Shape& sh;
    const ptsched::Plan& plan;
    const ptsched::State& next;        // the state the plan ends in
    ptk::BounceArgs a;                 // the render's words; a launch fills in its own
    std::vector<uint32_t> primary_events;
    uint32_t pool_begin = 0;
};
uint32_t* set_counters(const PtContext* c, uint32_t set) { return c->ovf_count.p + kStatsWords + kCountStride * set; }

int exec_launch(Exec& x, const ptsched::Op& o, hipStream_t s) {
    using namespace ptsched;
    PtContext* const c = x.c;
    ptk::BounceArgs& a = x.a;
    const ptshape::Launch l = ptshape::launch(x.sh, o.batch, o.grid, o.level, o.flags);
    uint32_t* const d_count = set_counters(c, o.set);   // [0] leftovers handed over, [64 ...] chunk counters of k_paths_regen
    const bool own = o.own_queue != 0, inject = x.sh.inject, hand_off = x.sh.hand_off;
    a.s_base = x.prm->spp_offset + l.s0;
    a.lsamp = c->lsamp[o.set].p;
    a.n_first = l.n_first;
    a.n_first_dev = o.level > 0 ? d_count : nullptr;
    a.seg_cap = l.seg_cap;
    a.src_mode = l.src_mode;
    a.export_below = l.export_below;
    a.aux = own ? c->caux.p : c->bvh_aux.p;
    a.sray0 = own ? c->csray[0].p : c->bvh_sray[0].p;
    a.sray1 = own ? c->csray[1].p : c->bvh_sray[1].p;
    for (int k = 0; k < 4; ++k) {
        a.q.q[k] = own ? c->cqueue[k].p : c->queue[k].p;
        a.ovf_out.q[k] = hand_off ? c->ovf[o.ovf_par][k].p : nullptr;
        a.ovf_in.q[k] = inject ? const_cast<float4*>(x.list->inject[k]) : (hand_off ? c->ovf[o.ovf_par][k].p : nullptr);
    }
    a.ovf_out_count = d_count;
    a.debug_tag = o.set;
    a.chunk_counter = nullptr;
    a.xchg = nullptr;
    a.posted = nullptr; a.seq = 0; a.core_blocks = 0;
    a.regen_static = l.regen_static;
    if (o.flags & kLaunchRegen) {
        a.chunk_counter = d_count + ptk::kRegenCounterStride;
        if (o.flags & kLaunchSplit) a.xchg = c->xchg.p + o.xchg_off;
        if (o.core) { a.posted = c->h_posted.dev; a.seq = o.seq; a.core_blocks = o.core; }
    }
    const uint32_t inst = x.prm->exact_math ? ptk::launch_path_kernel_exact(a, o.grid, s) : ptk::launch_path_kernel_fast(a, o.grid, s);
    HIP_TRY(hipGetLastError());
    if (c->launch_log.size() < kLaunchLogCap) c->launch_log.push_back(inst);
    if ((o.flags & kLaunchPrimary) && x.plan.profile) x.primary_events.push_back(x.pool_begin / 2u);
    return PT_OK;
}

int exec_resolve(Exec& x, const ptsched::Op& o, hipStream_t s) {
    PtContext* const c = x.c;
    const uint32_t nb = ptshape::batch_samples(x.sh, o.batch), n_batches = x.sh.n_batches;
    if (x.ad) {
        ptk::AdaptiveResolveArgs r{};
        r.f = x.ad->f;
        r.lsamp = c->lsamp[o.set].p;
        r.pixels = x.list ? x.list->d_pixels : nullptr;
        r.width = x.cam->width; r.n = x.sh.np; r.nb = nb; r.n_total = x.ad->n_total;
        r.load = o.batch > 0 || x.ad->load;
        r.finalize = o.batch + 1 == n_batches;
        if (o.zero_words) { r.zero_words = set_counters(c, o.set); r.n_zero = o.zero_words; }
        ptk::launch_resolve_adaptive(r, s);
        HIP_TRY(hipGetLastError());
        return PT_OK;
    }
    if (x.cas) {
        ptk::CascadeResolveArgs r = x.cas->r;
        r.lsamp = c->lsamp[o.set].p;
        r.np = x.sh.np; r.nb = nb;
        r.load = o.batch > 0;
        r.finalize = o.batch + 1 == n_batches;
        if (o.zero_words) { r.zero_words = set_counters(c, o.set); r.n_zero = o.zero_words; }
        ptk::launch_resolve_cascade(r, s);
        HIP_TRY(hipGetLastError());
        return PT_OK;
    }
    if (x.flt) {
        ptk::FilterResolveArgs r = x.flt->r;
        r.lsamp = c->lsamp[o.set].p;
        r.nb = nb;
        r.first_sample = x.prm->spp_offset + o.batch * x.sh.nb_max;
        r.load = o.batch > 0;
        r.finalize = o.batch + 1 == n_batches;
        if (o.zero_words) { r.zero_words = set_counters(c, o.set); r.n_zero = o.zero_words; }
        ptk::launch_resolve_filter(r, s);
        HIP_TRY(hipGetLastError());
        return PT_OK;
    }
    ptk::ResolveArgs r{};
    r.lsamp = c->lsamp[o.set].p;
    r.film = c->film.p;
    r.out_linear = x.d_linear;
    r.out_rgba = x.d_rgba;
    r.np = x.sh.np; r.nb = nb;
    r.load_film = o.batch > 0 || x.fs.load;
    r.store_film = o.batch + 1 < n_batches || x.fs.store;
    r.finalize = o.batch + 1 == n_batches;
    r.spp_div = x.fs.div ? x.fs.div : x.sh.spp;
    r.out_packed = x.d_packed;
    if (o.zero_words) { r.zero_words = set_counters(c, o.set); r.n_zero = o.zero_words; }
    ptk::launch_resolve(r, s);
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int exec_op(Exec& x, const ptsched::Op& o, size_t index) {
    using namespace ptsched;
    PtContext* const c = x.c;
    if (c->debug_fail_at >= 0 && (size_t)c->debug_fail_at == index) {
        c->debug_fail_at = -1;
        return fail(PT_ERR_HIP, "injected failure at stream operation %zu of the render (pt_debug_fail_after)", index);
    }
    hipStream_t s = sched_stream(c, c->stream, o.stream);
    switch (o.kind) {
    case kOpHostSync:
        for (int k = 0; k < kLanes; ++k) HIP_TRY(hipStreamSynchronize(c->lane_stream[k]));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return c->xchg.ensure((size_t)x.next.xchg_stride * kLanes);
    case kOpMemsetStats:
        HIP_TRY(hipMemsetAsync(c->ovf_count.p, 0, kStatsWords * sizeof(uint32_t), s));
        return PT_OK;
    case kOpMemsetCounters:
        HIP_TRY(hipMemsetAsync(set_counters(c, o.set), 0, kCountStride * sizeof(uint32_t), s));
        return PT_OK;
    case kOpRecord:
        if (o.event == kEvPool && !(o.pool & 1u)) x.pool_begin = o.pool;
        HIP_TRY(hipEventRecord(sched_event(c, o), s));
        return PT_OK;
    case kOpWait:
        HIP_TRY(hipStreamWaitEvent(s, sched_event(c, o), 0));
        return PT_OK;
    case kOpPost:
        __atomic_store_n(c->h_posted.p, o.seq, __ATOMIC_RELEASE);      // before the launch is handed to the device
        return PT_OK;
    case kOpLaunch: return exec_launch(x, o, s);
    case kOpResolve: return exec_resolve(x, o, s);
    default:
        return fail(PT_ERR_HIP, "internal: unknown stream operation %u", o.kind);
    }
}

// COMMIT: the planned state becomes the context's; the host's share of the statistics
void commit(PtContext* c, const Exec& x, const ptsched::Job& job) {
    if (!x.plan.accumulate) begin_period(c);
    c->sched = x.next;
    // (the device-side statistics are read when they are collected -- pt_sync --, not copied back per render)
    const uint64_t n = (uint64_t)x.sh.np * x.sh.spp;
    if (job.capturing) {
        // nothing ran, and the graph may be replayed any number of times: the device will have counted a multiple of these
        uint64_t a = c->capture_gcd, b = n;
        while (b) { const uint64_t t = a % b; a = b; b = t; }
        c->capture_gcd = a;
    } else {
        c->expected_samples += n;
    }
    c->stats.bounce_launches += x.plan.launches;
    c->stats.batches += x.sh.n_batches;
    c->stats.primary_launches += x.plan.primary_launches;
    c->primary_events.insert(c->primary_events.end(), x.primary_events.begin(), x.primary_events.end());
}

}  // namespace

// The render driver behind every rendering entry: everything src/main.rs:43-60 does for the tile (or, with `list`,
// for a pixel list / a set of given rays).  Enqueues on the context's streams and returns; no host synchronisation.
// Its stages are the functions above: CHECK the arguments, resolve ACCEL, SIZE the render (pt_shape.h: pure), PREPARE every
// buffer it will touch -- nothing is enqueued before PREPARE has succeeded, so an error up to there leaves the context as it
// was --, PLAN (ptsched::plan on a copy of the scheduling state: pure), fill the ARGS, EXECUTE the plan's stream operations in
// order and COMMIT the copy.  A failure during EXECUTE: sched_recover.
int render_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const FilmState& fs, const ListRender* list,
                float* d_linear, uint8_t* d_rgba, void* d_packed, const AdaptivePass* ad, const CascadePass* cas, const FilterPass* flt) {
    int rc;
    if ((rc = check_render(c, cam, prm, list, d_linear, d_rgba))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    PtRenderParams resolved = *prm;
    resolved.accel = resolve_accel(c, prm->accel);
    prm = &resolved;

    const bool tile = !list || list->tile;
    const uint64_t np64 = !tile ? list->n : (uint64_t)pt_tile_rows(cam->height, prm->band_rows, prm->band_index, prm->band_count ? prm->band_count : 1) * cam->width;
    const uint64_t tile_rows = !tile ? ((np64 + 65535u) >> 16) : np64 / cam->width;
    if (np64 == 0) {                   // empty tile: nothing to render
        if (!c->sched.stats_pending) begin_period(c);
        return PT_OK;
    }
    if (!d_linear && !d_packed) return fail(PT_ERR_INVALID_ARG, "render: the linear output buffer is null");
    if (tile && (cam->width > 65535u || tile_rows > 65535u))   // (tile row, x) share one word of the path state
        return fail(PT_ERR_UNSUPPORTED, "tile %ux%llu: width and tile rows must be < 65536", cam->width, (unsigned long long)tile_rows);
    ptshape::Shape sh;
    if ((rc = size_render(c, prm, list, np64, &sh))) return rc;
    ptsched::Job job = sh.job;         // (PREPARE may fall back to its in-order form)
    if ((rc = prepare(c, prm, fs, sh, job))) return rc;

    // ---- PLAN (pure; on a copy of the state)
    ptsched::State next = c->sched;
#ifndef PT_SCHED_FAULTS
#define PT_SCHED_FAULTS 0        // measurement / demonstration builds only: ptsched::Faults switched on in the product path
#endif
    const ptsched::Plan plan = ptsched::plan(next, job, PT_SCHED_FAULTS);
    if (plan.profile) {
        uint32_t top = 0;
        for (const ptsched::Op& o : plan.ops) if (o.kind == ptsched::kOpRecord && o.event == ptsched::kEvPool) top = std::max(top, o.pool + 1u);
        if ((rc = ensure_events(c, top))) return rc;
    }

    Exec x{c, cam, prm, fs, list, ad, cas, flt, d_linear, d_rgba, d_packed, sh, plan, next, bounce_args(c, cam, prm, list, sh.np), {}, 0};
    for (size_t i = 0; i < plan.ops.size(); ++i)
        if ((rc = exec_op(x, plan.ops[i], i))) {
            const std::string keep = g_err;
            sched_recover(c, c->stream, next);
            g_err = keep;
            return rc;
        }
    c->debug_fail_at = -1;              // (the hook is for ONE render)
    commit(c, x, job);
    return PT_OK;
}

// The renders of injected camera paths: the thin lens, the projections and the caller's rays (5q), the bakes (5r).
// The path kernels know none of them: per sample batch the source's paths form (k_source_paths, pt_kernels_rays.hip) writes the
// batch's rays as path states into the context's inject planes, and render_impl takes them up as given paths of the tile
// (ListRender::tile: the launches of pt_ray_color, the film slots, keys and bands of a plain render).  One render_impl per batch
// of nb <= max_paths_in_flight / np samples; the f64 film sums travel between the batches as they do between the increments of
// pt_render_progressive, so the film does not depend on the batching.  Everything is checked, and the planes are there, before
// the first launch; all launches are on the caller's stream, which orders batch k's level-0 launch (the planes' only reader)
// before batch k + 1's fill.  The caller has checked what is its own (the lens, the projection, the ray planes) before.
int render_injected_impl(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const ptk::RaySourceF& src, float* d_linear,
                         uint8_t* d_rgba, bool no_camera) {
    if (!c || !cam || !prm) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    int rc;
    ListRender lr;
    lr.tile = true;
    lr.no_camera = no_camera;
    lr.inject[0] = reinterpret_cast<const float4*>(1);      // (check_render only asks whether the paths are given)
    if ((rc = check_render(c, cam, prm, &lr, d_linear, d_rgba))) return rc;
    const uint64_t np64 = tile_pixels(cam, prm);
    if (np64 == 0) return render_impl(c, cam, prm, FilmState{}, nullptr, d_linear, d_rgba);      // an empty tile, as ever
    if (!d_linear) return fail(PT_ERR_INVALID_ARG, "render: the linear output buffer is null");
    if (cam->width > 65535u || np64 / cam->width > 65535u)
        return fail(PT_ERR_UNSUPPORTED, "tile %ux%llu: width and tile rows must be < 65536", cam->width, (unsigned long long)(np64 / cam->width));
    const uint64_t cap = std::min<uint64_t>(prm->max_paths_in_flight ? prm->max_paths_in_flight : kDefaultMaxPaths, ptshape::kMaxPaths);
    if (np64 > cap)
        return fail(PT_ERR_UNSUPPORTED, "tile of %llu pixels exceeds max_paths_in_flight %llu; use more bands", (unsigned long long)np64,
                    (unsigned long long)cap);
    const uint32_t np = (uint32_t)np64;
    const uint32_t nb_max = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(cap / np, 65535u), prm->spp);
    HIP_TRY(hipSetDevice(c->device));
    for (int k = 0; k < 4; ++k)
        if ((rc = c->inject[k].ensure((size_t)np * nb_max))) return rc;
    ptk::SourcePathsArgs a{};
    a.src = src;
    a.tile = tile_map(cam, prm);
    a.np = np; a.np_magic = magic_of(np); a.w_magic = magic_of(cam->width);
    for (int k = 0; k < 4; ++k) { a.q[k] = c->inject[k].p; lr.inject[k] = c->inject[k].p; }
    for (uint32_t done = 0; done < prm->spp;) {
        const uint32_t nb = std::min(nb_max, prm->spp - done);
        PtRenderParams p = *prm;
        p.spp = nb;
        p.spp_offset = prm->spp_offset + done;
        p.max_paths_in_flight = cap;      // (the cap the batches were cut for, whatever default the sizing would pick)
        a.s_base = p.spp_offset; a.done = done; a.n = np * nb;
        if (!ptk::launch_source_paths(prm->exact_math, a, c->stream)) return fail(PT_ERR_INVALID_ARG, "%s: ray source %u has no paths kernel", who, src.tag);
        HIP_TRY(hipGetLastError());
        lr.inject_spp = nb;
        FilmState fs;
        fs.load = done > 0;
        fs.store = done + nb < prm->spp;
        fs.div = prm->spp;
        if ((rc = render_impl(c, cam, &p, fs, &lr, d_linear, d_rgba))) return rc;
        done += nb;
    }
    return PT_OK;
}

int source_setup(const char* who, const PtCamera* cam, const FrameSource& src, ptk::RaySourceF* out) {
    *out = ptk::RaySourceF{};
    out->tag = src.lens ? ptk::kSrcLens : src.proj ? ptk::kSrcProjection : ptk::kSrcCamera;
    out->cam = camera_f32(cam);
    if (src.lens) return lens_setup(who, cam, src.lens, &out->lens);
    return src.proj ? projection_setup(who, cam, src.proj, &out->proj) : PT_OK;
}

int render_source_impl(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm, float* d_linear,
                       uint8_t* d_rgba) {
    if (!c || !cam || !prm || (!src.lens && !src.proj)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    ptk::RaySourceF s;
    if (int rc = source_setup(who, cam, src, &s)) return rc;
    return render_injected_impl(who, c, cam, prm, s, d_linear, d_rgba);
}

extern "C" {

int pt_render_lens_device(PtContext* c, const PtCamera* cam, const PtLens* lens, const PtRenderParams* prm, float* d_linear, uint8_t* d_rgba) {
    return render_source_impl("pt_render_lens_device", c, cam, {lens, nullptr}, prm, d_linear, d_rgba);
}

int pt_render_lens_host(PtContext* c, const PtCamera* cam, const PtLens* lens, const PtRenderParams* prm, float* out_linear, uint8_t* out_rgba) {
    if (!c || !cam || !lens || !prm || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_lens_host: null argument");
    ptk::LensF checked;
    if (int bad = lens_setup("pt_render_lens_host", cam, lens, &checked)) return bad;      // before the staging is touched
    const size_t np = tile_pixels(cam, prm);
    if (np == 0) return render_source_impl("pt_render_lens_host", c, cam, {lens, nullptr}, prm, nullptr, nullptr);   // validates, renders nothing
    HIP_TRY(hipSetDevice(c->device));
    return render_staged(c, np * 3, out_rgba ? np * 4 : 0,
                         [&](float* d_linear, uint8_t* d_rgba) { return render_source_impl("pt_render_lens_host", c, cam, {lens, nullptr}, prm, d_linear, d_rgba); },
                         [&] { return film_back(c, np, out_linear, out_rgba); });
}

int pt_render_device(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, float* d_linear, uint8_t* d_rgba) {
    return render_impl(c, cam, prm, FilmState{}, nullptr, d_linear, d_rgba);
}
// The same render with the film written as ONE 16-byte record per tile pixel (12 B linear RGB + 4 B RGBA8): the send buffer of
// the multi-GPU gather, straight from the resolve (what pt_film_pack makes of the two planes in a launch of its own).
int pt_render_device_packed(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, void* d_packed) {
    if (!d_packed) return fail(PT_ERR_INVALID_ARG, "pt_render_device_packed: the output buffer is null");
    if ((uintptr_t)d_packed % 16u) return fail(PT_ERR_INVALID_ARG, "pt_render_device_packed: the output buffer must be 16-byte aligned");
    return render_impl(c, cam, prm, FilmState{}, nullptr, nullptr, nullptr, d_packed);
}

int pt_render_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, float* out_linear, uint8_t* out_rgba) {
    if (!c || !cam || !prm || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_host: null argument");
    return render_to_host(c, cam, prm, FilmState{}, nullptr, tile_pixels(cam, prm), out_linear, out_rgba);
}

// The progressive preview of the reference (main.rs:79-90 redraws World.data every 16 ms while
// the rayon loop fills it): the same render in increments of spp_step samples; after each increment
// the film holds the mean of the samples so far.  The last frame is bit-identical to pt_render_host.
int pt_render_progressive(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t spp_step,
                          PtProgressFn fn, void* user, float* out_linear, uint8_t* out_rgba) {
    if (!c || !cam || !prm || !out_linear || !out_rgba)
        return fail(PT_ERR_INVALID_ARG, "pt_render_progressive: null argument");
    if (int rc = check_spp(prm->spp)) return rc;
    if (spp_step == 0) spp_step = prm->spp;
    const size_t np = tile_pixels(cam, prm);
    int rc = PT_OK;
    for (uint32_t done = 0; done < prm->spp && rc == PT_OK;) {
        const uint32_t n = std::min(spp_step, prm->spp - done);
        PtRenderParams p = *prm;
        p.spp = n;
        p.spp_offset = prm->spp_offset + done;
        FilmState fs;                   // the f64 sums of the film stay on the device between increments
        fs.load = done > 0;
        fs.store = done + n < prm->spp;
        fs.div = done + n;
        rc = render_to_host(c, cam, &p, fs, nullptr, np, out_linear, out_rgba);
        done += n;
        if (rc == PT_OK && np != 0 && fn && fn(user, done, prm->spp, out_rgba, out_linear) != 0) break;   // caller asked to stop
    }
    return rc;
}

int pt_render_pixels(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const uint32_t* xy, uint32_t n,
                     float* out_linear, uint8_t* out_rgba, float* out_samples) {
    if (!c || !cam || !prm || (n && (!xy || !out_linear))) return fail(PT_ERR_INVALID_ARG, "pt_render_pixels: null argument");
    for (uint32_t i = 0; i < n; ++i)
        if (xy[2 * i] >= cam->width || xy[2 * i + 1] >= cam->height)
            return fail(PT_ERR_INVALID_ARG, "pixel %u = (%u, %u) is outside the %ux%u image", i, xy[2 * i], xy[2 * i + 1], cam->width, cam->height);
    ListRender lr;
    if (n) {
        HIP_TRY(hipSetDevice(c->device));
        int rc = c->pixel_list.ensure(n);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));            // an earlier list may still be in use
        HIP_TRY(hipMemcpy(c->pixel_list.p, xy, (size_t)n * sizeof(uint2), hipMemcpyHostToDevice));
        lr.d_pixels = c->pixel_list.p;
    }
    lr.n = n;
    if (out_samples && n) {
        const uint64_t cap = std::min<uint64_t>(prm->max_paths_in_flight ? prm->max_paths_in_flight : kDefaultMaxPaths, 1ull << 30);
        if ((uint64_t)n * prm->spp > cap || prm->spp > 65535u)
            return fail(PT_ERR_UNSUPPORTED, "pt_render_pixels: out_samples needs n * spp = %llu paths in one sample batch (limit %llu, spp < 65536)",
                        (unsigned long long)n * prm->spp, (unsigned long long)cap);
    }
    int rc = render_to_host(c, cam, prm, FilmState{}, &lr, n, out_linear, out_rgba);
    if (rc || !out_samples || !n) return rc;
    // the batch's per-path radiance buffer, index = sample * n + pixel  ->  [pixel][sample][rgb]
    std::vector<ptk::Rgb> ls((size_t)n * prm->spp);
    HIP_TRY(hipMemcpy(ls.data(), c->lsamp[0].p, ls.size() * sizeof(ptk::Rgb), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t sidx = 0; sidx < prm->spp; ++sidx) {
            const ptk::Rgb v = ls[(size_t)sidx * n + i];
            float* o = out_samples + ((size_t)i * prm->spp + sidx) * 3;
            o[0] = v.r; o[1] = v.g; o[2] = v.b;
        }
    return PT_OK;
}

}  // extern "C"

// Adaptive sampling: pass 0 gives every pixel spp_min samples (the full-frame kernels); then, while pixels are left whose
// last check failed (pt_adaptive.h), k_adaptive_select compacts them into a list and the next pass gives them spp_step more
// (the regenerating kernel's LIST instances where the scene takes that kernel).  Every pass is a render_impl whose resolve
// is k_resolve_adaptive.  A pixel's samples are spp_offset .. spp_offset + n - 1 and its f64 sums are added in sample order,
// so it is bit-identical to a uniform render of that pixel with spp = n.
// The passes are waited for: the film is left in c->host_lin / c->host_rgba and the per-pixel state in
// c->ad_* on the device.  The context holds that state (ad_valid, ad_width, ad_height) for pt_adaptive_variance_device
// until the next adaptive render is asked for; one that fails, on its arguments or later, leaves none.
int render_adaptive_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtAdaptive* ad) {
    c->ad_valid = false;
    if (ad->spp_min < 2) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: spp_min %u < 2 (the variance needs two samples)", ad->spp_min);
    if (ad->spp_step == 0) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: spp_step must be > 0");
    if (prm->spp < ad->spp_min) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: spp (= spp_max) %u < spp_min %u", prm->spp, ad->spp_min);
    if (!(ad->rel_tol >= 0.0) || !std::isfinite(ad->rel_tol)) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: rel_tol must be finite and >= 0");
    if (!(ad->abs_floor > 0.0)) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: abs_floor must be > 0");
    int rc;
    if ((rc = check_whole_image("pt_render_adaptive", ": renders", "", prm)) || (rc = check_scene(c)) || (rc = check_camera_size(cam)) ||
        (rc = check_pixel_count("pt_render_adaptive", cam->width, cam->height)))
        return rc;
    const uint32_t np = cam->width * cam->height, spp_max = prm->spp, W = cam->width;
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    if ((rc = c->ad_sums.ensure(5 * (size_t)np)) || (rc = c->ad_count.ensure(np)) || (rc = c->ad_conv.ensure(np)) ||
        (rc = c->ad_err.ensure(np)) || (rc = c->ad_list[0].ensure(np)) || (rc = c->ad_list[1].ensure(np)) ||
        (rc = c->ad_words.ensure(1 + (np + ptk::kSelectTile - 1) / ptk::kSelectTile)) || (rc = c->host_lin.ensure(3 * (size_t)np)) ||
        (rc = c->host_rgba.ensure(4 * (size_t)np)))
        return rc;
    AdaptivePass pass;
    pass.f.sums = c->ad_sums.p; pass.f.count = c->ad_count.p; pass.f.rel_err = c->ad_err.p; pass.f.conv = c->ad_conv.p;
    pass.f.out_linear = c->host_lin.p; pass.f.out_rgba = c->host_rgba.p;
    pass.f.rel_tol = ad->rel_tol; pass.f.abs_floor = ad->abs_floor;
    PtRenderParams p = *prm;
    p.band_count = 1; p.band_index = 0; p.band_rows = 0;
    // pass 0: the whole image, full-frame kernels; list slot = image pixel
    p.spp = ad->spp_min;
    pass.load = false; pass.n_total = ad->spp_min;
    if ((rc = render_impl(c, cam, &p, FilmState{}, nullptr, c->host_lin.p, c->host_rgba.p, nullptr, &pass))) return rc;
    uint32_t done = ad->spp_min, n_cur = np, which = 0;
    const uint2* cur = nullptr;                 // the last pass's list (null: every pixel, image order)
    uint32_t* const d_n = c->ad_words.p;
    while (done < spp_max) {
        ptk::launch_adaptive_select(cur, n_cur, W, c->ad_conv.p, c->ad_words.p + 1, c->ad_list[which].p, d_n, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c->h_ovf.p, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const uint32_t n_next = c->h_ovf.p[0];
        if (n_next == 0) break;
        const uint32_t step = std::min(ad->spp_step, spp_max - done);
        ListRender lr;
        lr.d_pixels = c->ad_list[which].p; lr.n = n_next; lr.regen = true;
        p.spp = step; p.spp_offset = prm->spp_offset + done;
        pass.load = true; pass.n_total = done + step;
        if ((rc = render_impl(c, cam, &p, FilmState{}, &lr, c->host_lin.p, c->host_rgba.p, nullptr, &pass))) return rc;
        done += step;
        cur = c->ad_list[which].p; n_cur = n_next; which ^= 1u;
    }
    if ((rc = pt_sync(c))) return rc;
    c->ad_valid = true; c->ad_width = cam->width; c->ad_height = cam->height;
    return PT_OK;
}

extern "C" {

int pt_render_adaptive(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtAdaptive* ad, float* out_linear,
                       uint8_t* out_rgba, uint32_t* out_spp, float* out_rel_err) {
    if (!c || !cam || !prm || !ad || !out_linear) return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: null argument");
    int rc;
    if ((rc = render_adaptive_impl(c, cam, prm, ad))) return rc;
    const size_t np = (size_t)cam->width * cam->height;
    return copy_back({{out_linear, c->host_lin.p, 3 * np * sizeof(float)}, {out_rgba, c->host_rgba.p, 4 * np},
                      {out_spp, c->ad_count.p, np * sizeof(uint32_t)}, {out_rel_err, c->ad_err.p, np * sizeof(float)}});
}

int pt_ray_color(PtContext* c, const PtRenderParams* prm, const double* rays, const uint32_t* xy, uint32_t n, float* out_rgb) {
    if (!c || !prm || (n && (!rays || !xy || !out_rgb))) return fail(PT_ERR_INVALID_ARG, "pt_ray_color: null argument");
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the paths in queue form (pt_kernels.h): depth 0, throughput 1, no radiance yet, film slot = ray index
    std::vector<float4> plane[4];
    for (auto& pl : plane) pl.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float o[3] = {(float)rays[6 * (size_t)i], (float)rays[6 * (size_t)i + 1], (float)rays[6 * (size_t)i + 2]};
        float d[3] = {(float)rays[6 * (size_t)i + 3], (float)rays[6 * (size_t)i + 4], (float)rays[6 * (size_t)i + 5]};
        // Ray::new normalises (camera.rs:10-16): Vector3::normalize in the f32 arithmetic of the device's exact mode
        const float len = std::sqrt(std::fmaf(d[2], d[2], std::fmaf(d[1], d[1], d[0] * d[0])));
        if (len > 0.0f) { const float inv = 1.0f / len; d[0] *= inv; d[1] *= inv; d[2] *= inv; }
        const uint32_t slot = i, sd = 0u;     // (tile_row << 16 | x) of a 65536-wide film; (s_local << 16 | depth)
        float fslot, fsd;
        std::memcpy(&fslot, &slot, 4); std::memcpy(&fsd, &sd, 4);
        plane[0][i] = make_float4(o[0], o[1], o[2], d[0]);
        plane[1][i] = make_float4(d[1], d[2], fslot, fsd);
        plane[2][i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);      // throughput 1, pdf_prev 0
        plane[3][i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);      // no radiance yet, eta_ratio 1 (camera.rs:14)
    }
    int rc;
    if ((rc = c->pixel_list.ensure(n))) return rc;
    for (int k = 0; k < 4; ++k) if ((rc = c->inject[k].ensure(n))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->pixel_list.p, xy, (size_t)n * sizeof(uint2), hipMemcpyHostToDevice));
    ListRender lr;
    lr.d_pixels = c->pixel_list.p; lr.n = n;
    for (int k = 0; k < 4; ++k) {
        HIP_TRY(hipMemcpy(c->inject[k].p, plane[k].data(), (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
        lr.inject[k] = c->inject[k].p;
    }
    PtCamera cam{};                     // no camera rays are generated
    cam.width = cam.height = 2;
    return render_to_host(c, &cam, prm, FilmState{}, &lr, n, out_rgb, nullptr);
}

}  // extern "C"
