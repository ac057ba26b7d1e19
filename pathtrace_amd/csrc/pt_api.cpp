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

#include "pt_context.h"

namespace {

constexpr uint64_t kDefaultMaxPaths = 1ull << 26;
// ... where the level-0 launch keeps its paths in registers (k_paths_regen) a path in flight costs 12 bytes of sample buffer
// instead of 76, and every batch ends in a ~0.3 ms tail: larger batches (C3: 16 instead of 64)
constexpr uint64_t kDefaultMaxPathsRegen = 1ull << 28;
// Default number of workgroups.  What matters is that the queue segments of the RESIDENT waves fit the 256 MiB
// Infinity Cache (and that the dispatcher has enough workgroups to balance the end of the launch; much smaller
// segments pay more low-occupancy tail passes).  Scene in LDS, 6 waves/SIMD = 6144 resident waves: ~672 paths
// (42 KiB of queue) per wave -- measured at 67 M paths: 8192 workgroups 10.31 ms, 12288 10.12, 16384 9.86,
// 24576 9.61 (best), 32768 9.69.  Tiled scan and BVH kernels (4-5 waves/SIMD): ~1024 paths per wave (measured at
// 4 waves/SIMD: 2048 workgroups 11.6 ms, 8192 10.7, 16384 10.2 (best), 32768 10.6, 65536 11.7).
constexpr uint32_t kPathsPerWaveLds = 672;
constexpr uint32_t kPathsPerWave = 1024;
constexpr uint32_t kMinGrid = 256 * 8;         // level-0 launches: at least this many workgroups (small renders)
// continuation launches: their paths are sparse survivors, and a wave-iteration costs the same however few of its
// lanes carry a path, so more, emptier segments cost time -- and so do too few waves (latency of ~35 dependent passes).
// Measured on C2 / C1, ms of the continuation launch: 96 workgroups 1.75 / 5.0, 192 0.98 / 2.7, 384 0.60 / 1.6,
// 768 0.44 / 1.16, 1024 0.46, 1536 0.51 / 1.19, 3072 0.69 (round 1: 6144 -> +0.8).
constexpr uint32_t kContGrid = 1024;
#ifndef PT_REGEN_EXPORT
#define PT_REGEN_EXPORT 1
#endif
constexpr uint32_t kCountStride = (1 + ptk::kRegenCounters) * ptk::kRegenCounterStride;   // uint32 per batch parity: leftover count + chunk counters
#ifndef PT_SPLIT_BY_DEFAULT
#define PT_SPLIT_BY_DEFAULT 1
#endif
constexpr bool kSplitByDefault = PT_SPLIT_BY_DEFAULT != 0;   // scenes with a minority of Mirror objects: k_paths_regen_split (else the queue form)
#ifndef PT_REGEN_STATIC16
#define PT_REGEN_STATIC16 4
#endif
constexpr uint32_t kRegenStatic16 = PT_REGEN_STATIC16;   // k_paths_regen: sixteenths of a batch's chunks dealt round-robin, the rest by the counters
constexpr uint32_t kRegenExportBelow = PT_REGEN_EXPORT;  // ... and its waves hand over once the batch is used up and fewer paths than this are alive
                                               // (1: they run dry themselves and no continuation launch follows)
constexpr uint32_t kExportSmall = 64;          // a wave hands its segment over when fewer paths than this are left
                                               // (measured 32 ... 256: no difference beyond noise on C1 and C2)
// Tail hand-off: in launches of more than kExportMinPaths paths a wave whose segment falls below one chunk
// exports its leftovers to the overflow queue instead of walking them alone; the next launch takes them up.
// Measured (C2 / C1 ms per 1024^2 x 64 render): no hand-off 10.33 / 18.5; threshold 2^18 (3-4 levels) 11.2 / 16.9;
// 2^22 (2 levels) 10.28 / 15.65; exporting below 32 or 16 paths instead of 64 is slower.
#ifndef PT_EXPORT_MIN_LOG2
#define PT_EXPORT_MIN_LOG2 22
#endif
constexpr uint32_t kExportMinPaths = 1u << PT_EXPORT_MIN_LOG2;
// batches of more paths than this take the regenerating level-0 kernel (where the scene allows it)
#ifndef PT_REGEN_MIN_LOG2
#define PT_REGEN_MIN_LOG2 17
#endif
constexpr uint32_t kRegenMinPaths = 1u << PT_REGEN_MIN_LOG2;
constexpr uint32_t kWavesPerBlock = ptk::kBlock / 64;
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
int render_to_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const FilmState& fs, const ListRender* list,
                   size_t np, float* out_linear, uint8_t* out_rgba) {
    if (np == 0) return render_impl(c, cam, prm, fs, list, nullptr, nullptr);   // validates, renders nothing
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->host_lin.ensure(np * 3))) return rc;
    if (out_rgba && (rc = c->host_rgba.ensure(np * 4))) return rc;
    rc = render_impl(c, cam, prm, fs, list, c->host_lin.p, out_rgba ? c->host_rgba.p : nullptr);
    if (!rc) rc = pt_sync(c);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_linear, c->host_lin.p, np * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, c->host_rgba.p, np * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}
size_t tile_pixels(const PtCamera* cam, const PtRenderParams* prm) {
    return (size_t)pt_tile_rows(cam->height, prm->band_rows, prm->band_index, prm->band_count ? prm->band_count : 1) * cam->width;
}

}  // namespace

// The render driver behind every rendering entry: everything src/main.rs:43-60 does for the tile (or, with `list`,
// for a pixel list / a set of given rays).  Enqueues on the context's streams and returns; no host synchronisation.
// Three steps: PREPARE (validate, size, allocate every buffer the render will touch -- nothing is enqueued yet, so an
// error here leaves the context as it was), PLAN (ptsched::plan on a copy of the scheduling state: pure), EXECUTE (the
// plan's stream operations in order) and COMMIT of the copy.  A failure during EXECUTE: sched_recover.
int render_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const FilmState& fs, const ListRender* list,
                float* d_linear, uint8_t* d_rgba, void* d_packed, const AdaptivePass* ad) {
    if (!c || !cam || !prm) return fail(PT_ERR_INVALID_ARG, "render: null argument");
    if (!c->has_scene) return fail(PT_ERR_INVALID_ARG, "render: no scene uploaded");
    const bool inject = list && list->inject[0];
    if (!inject && (cam->width < 2 || cam->height < 2))   // get_ray_with_offset divides by width-1 / height-1 (camera.rs:140-141)
        return fail(PT_ERR_INVALID_ARG, "camera %ux%u: width and height must be >= 2", cam->width, cam->height);
    if (prm->spp == 0) return fail(PT_ERR_INVALID_ARG, "spp must be > 0");
    if (prm->integrator > PT_INTEGRATOR_BRDF_ONLY) return fail(PT_ERR_INVALID_ARG, "unknown integrator %u", prm->integrator);
    if (prm->accel > PT_ACCEL_AUTO) return fail(PT_ERR_INVALID_ARG, "unknown accel %u", prm->accel);
    const uint32_t band_count = prm->band_count ? prm->band_count : 1;
    if (prm->band_index >= band_count) return fail(PT_ERR_INVALID_ARG, "band_index %u >= band_count %u", prm->band_index, band_count);
    if (list && band_count != 1) return fail(PT_ERR_INVALID_ARG, "pixel-list renders take the whole image (band_count = 1)");
    // the resolve stores a pixel's RGBA8 as one 32-bit word (a byte-offset pointer would fault on the device)
    if (d_rgba && (uintptr_t)d_rgba % 4u) return fail(PT_ERR_INVALID_ARG, "render: the RGBA8 output buffer must be 4-byte aligned");
    if (d_linear && (uintptr_t)d_linear % 4u) return fail(PT_ERR_INVALID_ARG, "render: the linear output buffer must be 4-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    PtRenderParams resolved = *prm;      // PT_ACCEL_AUTO -> what actually runs
    if (prm->accel == PT_ACCEL_AUTO) {
        resolved.accel = PT_ACCEL_LINEAR;
        if (c->auto_bvh && !c->bvh_refused && !c->bvh_failed) {
            const std::string keep = g_err;              // a refused BVH is not an error of this call
            if (ensure_bvh(c) == PT_OK) resolved.accel = PT_ACCEL_BVH;
            else g_err = keep;
        }
    }
    prm = &resolved;

    const uint64_t np64 = list ? list->n : (uint64_t)pt_tile_rows(cam->height, prm->band_rows, prm->band_index, band_count) * cam->width;
    const uint64_t tile_rows = list ? ((np64 + 65535u) >> 16) : np64 / cam->width;
    // Statistics belong to the renders enqueued since they were last collected (pt_sync / pt_get_stats): a caller that
    // pipelines several renders behind one synchronisation gets their sums (vertices, launches, kernel times), total_ms from
    // the first one's start to the last one's end.  One render per synchronisation: the statistics of that render, as ever.
    auto begin_period = [c]() {        // the first render since the last collection
        std::memset(&c->stats, 0, sizeof c->stats);
        c->primary_events.clear();
        c->expected_samples = 0;
    };
    if (np64 == 0) {                   // empty tile: nothing to render
        if (!c->sched.stats_pending) begin_period();
        return PT_OK;
    }
    if (!d_linear && !d_packed) return fail(PT_ERR_INVALID_ARG, "render: the linear output buffer is null");
    if (!list && (cam->width > 65535u || tile_rows > 65535u))   // (tile row, x) share one word of the path state
        return fail(PT_ERR_UNSUPPORTED, "tile %ux%llu: width and tile rows must be < 65536", cam->width, (unsigned long long)tile_rows);
    // scene / job that can take the regenerating level-0 kernel (decided below, once the batch size is known)
    // level0_form 3 / default for scenes with a minority of Mirror objects: the regenerating form with the Mirror vertices batched
    // (a list takes the regenerating kernel only where its caller asks for it, and never the split form)
    const bool lds_job = (!list || list->regen) && !prm->accel && c->view.n_objs <= ptk::kSmallObjs && c->view.blob_f4 != 0;
    const bool split = lds_job && !list && (c->tuning.level0_form == 3 || (c->tuning.level0_form == 0 && c->split_ok && kSplitByDefault));
    // default (round 3): every scene in LDS takes a regenerating form -- compiled for its material set (diffuse only; no
    // Mirror; everything); with the Mirror vertices batched where they are the exception (split, above).  The queue form
    // is level0_form = 1 (all-Mirror Cornell scene: queue form 12.6 ms, regenerating 10.0, split 13.8; tools/r03/mirror_forms.py)
    const bool regen_scene = split || ((c->tuning.level0_form == 2 || c->tuning.level0_form == 0) && lds_job);
    uint64_t cap = prm->max_paths_in_flight ? prm->max_paths_in_flight : (regen_scene ? kDefaultMaxPathsRegen : kDefaultMaxPaths);
    if (cap > (1ull << 30)) cap = 1ull << 30;
    if (np64 > cap)
        return fail(PT_ERR_UNSUPPORTED, "tile of %llu pixels exceeds max_paths_in_flight %llu; use more bands",
                    (unsigned long long)np64, (unsigned long long)cap);
    const uint32_t np = (uint32_t)np64;
    const uint32_t spp = inject ? 1u : prm->spp;
    uint32_t nb_max = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(cap / np, 65535u), spp);
    if (nb_max == 0) nb_max = 1;
    const size_t n_paths_max = (size_t)np * nb_max;
    const uint32_t n_batches = (spp + nb_max - 1) / nb_max;

    // Queue segments: one per wave of the (fixed) grid; pass 0 deals 64-path chunks round-robin, so a segment holds
    // at most ceil(chunks / waves) chunks.
    const uint32_t export_small = c->tuning.export_below ? std::min(256u, std::max(1u, c->tuning.export_below)) : kExportSmall;
    const uint32_t chunks_max = (uint32_t)((n_paths_max + 63) / 64);
    uint32_t grid = prm->workgroups;
    const bool small_scene = c->view.n_objs <= ptk::kSmallObjs || prm->accel;     // the tiled scan exports per workgroup (< 256 paths)
    const uint32_t paths_per_wave = (c->view.n_objs <= ptk::kSmallObjs && !prm->accel) ? kPathsPerWaveLds : kPathsPerWave;
    if (!grid) {
        const uint64_t want = (n_paths_max + (uint64_t)paths_per_wave * kWavesPerBlock - 1) / ((uint64_t)paths_per_wave * kWavesPerBlock);
        grid = (uint32_t)std::max<uint64_t>(want, kMinGrid);
    }
    grid = std::min<uint32_t>(grid, (chunks_max + kWavesPerBlock - 1) / kWavesPerBlock);
    if (grid == 0) grid = 1;
    const uint32_t nw = grid * kWavesPerBlock;
    const uint32_t seg_cap = ((chunks_max + nw - 1) / nw) * 64u;
    // Tail hand-off: the level-0 launch of a large batch exports what its waves have left below one chunk; ONE
    // continuation launch of fixed size takes that queue up.  It reads the count on the device.
    // (scenes that take a regenerating level-0 kernel have their own threshold: that launch needs no continuation launch)
    const bool hand_off = !inject && n_paths_max > (regen_scene ? kRegenMinPaths : kExportMinPaths);
    // Such a batch over a scene in LDS takes the regenerating level-0 kernel: paths live in registers, a lane whose
    // path ends takes the next one of the batch; grid = the waves the device holds at once (k_paths_regen).
    const bool regen = regen_scene && hand_off;
    // its grid = the workgroups the device holds at once: the kernel's occupancy with THIS scene's LDS blob (a 128-object
    // scene leaves room for fewer workgroups per CU than the compile-time figure)
    uint32_t regen_per_cu = split ? ptk::kRegenWavesSplit : c->view.diffuse_only ? ptk::kRegenWavesDiffuse : ptk::kRegenWavesGeneric;
    if (regen_scene) {
        ptk::BounceArgs q{};
        q.sc = view_for(c, prm->exact_math);
        q.integrator = prm->integrator;
        q.xchg = split ? reinterpret_cast<float4*>(1) : nullptr;       // selects the kernel only
        uint32_t& occ = c->regen_occ[prm->exact_math ? 1 : 0][prm->integrator ? 1 : 0][split ? 1 : 0];   // per scene (pt_scene_upload clears it)
        if (occ == 0u) occ = prm->exact_math ? ptk::regen_blocks_per_cu_exact(q) : ptk::regen_blocks_per_cu_fast(q);
        if (occ != 0u) regen_per_cu = std::min(regen_per_cu, occ);
    }
    const uint32_t regen_capacity = c->n_cus * regen_per_cu;          // workgroups the device holds at once
    const uint32_t regen_grid = std::min(65536u, prm->workgroups ? prm->workgroups : c->tuning.regen_workgroups ? c->tuning.regen_workgroups : regen_capacity);
    const uint32_t cont_grid = c->tuning.cont_workgroups ? std::min(65536u, c->tuning.cont_workgroups) : kContGrid;
    const uint32_t nw_cont = cont_grid * kWavesPerBlock;
    // leftovers per wave of the level-0 launch: < export_small from a wave-private segment, < 256 per workgroup
    // (= 64 per wave) from a workgroup-shared one
    const size_t ovf_slots = (size_t)(regen ? regen_grid * kWavesPerBlock : nw) * std::max(export_small, 64u) + 64u;
    const uint32_t seg_cap_cont = (uint32_t)((((ovf_slots + 63) / 64 + nw_cont - 1) / nw_cont) * 64u);
    const size_t q_slots_cont = hand_off ? (size_t)nw_cont * seg_cap_cont : 0;
    const size_t q_slots = regen ? std::max<size_t>(q_slots_cont, 64) : std::max((size_t)nw * seg_cap, q_slots_cont);
    const uint32_t regen_export = split ? 1u : c->tuning.export_below ? std::min(export_small, 64u) : kRegenExportBelow;   // the split form has no hand-over
    // (sized by the grid the launch really takes: never more workgroups than the largest batch has chunks for)
    const uint32_t regen_launch_grid = std::min<uint32_t>(regen_grid, (chunks_max + kWavesPerBlock - 1) / kWavesPerBlock);

    // ---- the job as the scheduler sees it (pt_sched.h)
    ptsched::Job job;
    job.n_batches = n_batches;
    job.regen = regen; job.split = regen && split; job.hand_off = hand_off; job.regen_export = regen_export;
    job.profile = prm->profile != 0; job.in_order = c->tuning.in_order != 0;
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        job.capturing = !(hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone);
        (void)hipGetLastError();
    }
    job.grid = grid; job.regen_grid = regen_launch_grid; job.cont_grid = cont_grid;
    job.regen_capacity = regen_capacity;
    job.fixed_grid = prm->workgroups != 0 || c->tuning.regen_workgroups != 0;
    job.counter_words = kCountStride;
    job.xchg_need = job.split ? (size_t)regen_launch_grid * kWavesPerBlock * ptk::kRegenSplitF4PerWave + 1024 : 0;   // + slack: a violated stack invariant (reported) stays inside the buffer

    // ---- PREPARE: every buffer the render will touch, before anything is enqueued
    int rc;
    if (prm->accel && (rc = ensure_bvh(c))) return rc;
    for (int k = 0; k < 4; ++k)
        if ((rc = c->queue[k].ensure(q_slots))) return rc;
    if (prm->accel && ((rc = c->bvh_aux.ensure(q_slots)) || (rc = c->bvh_sray[0].ensure(q_slots)) ||
                       (rc = c->bvh_sray[1].ensure(q_slots))))
        return rc;
    {
        // The buffer sets the render rotates through (with lanes: up to three sample buffers of 12 B per path in flight -- 3 x 3.2 GB
        // for the reference's 400 x 400 x 3000 job at the default cap).  All of them now: an allocation in the middle of the batch
        // loop would drain the pipeline the lanes keep full, and fail with half of the render enqueued.  If the device cannot hold
        // them, the render falls back to ONE set and launches in order -- slower, same film -- instead of failing.
        uint32_t sets[4], n_sets = 0;
        ptsched::sets_of(c->sched, job, sets, &n_sets);
        for (uint32_t k = 0; k < n_sets; ++k) {
            rc = c->lsamp[sets[k]].ensure(n_paths_max);
            if (rc == PT_ERR_OOM && ptsched::takes_lanes(job)) {
                job.in_order = 1;
                ptsched::sets_of(c->sched, job, sets, &n_sets);
                k = (uint32_t)-1;                       // start over with the one set of the in-order form
                continue;
            }
            if (rc) return rc;
        }
    }
    const bool overlap = n_batches > 1 && !regen;
    if (overlap && hand_off)
        for (int k = 0; k < 4; ++k)
            if ((rc = c->cqueue[k].ensure(q_slots_cont))) return rc;
    if (overlap && hand_off && prm->accel && ((rc = c->caux.ensure(q_slots_cont)) || (rc = c->csray[0].ensure(q_slots_cont)) ||
                                              (rc = c->csray[1].ensure(q_slots_cont))))
        return rc;
    if (!c->ovf_count.p) {             // [render statistics | launch counters of buffer set 0 | 1 | ...], zero from the start
        if ((rc = c->ovf_count.ensure(kStatsWords + kSets * kCountStride))) return rc;
        // (on the caller's stream and waited for: a plain hipMemset runs on the legacy default stream, which the context's
        // non-blocking streams do not wait for -- the first render's counts raced with it, caught by pt_sync's own sample check)
        HIP_TRY(hipMemsetAsync(c->ovf_count.p, 0, (kStatsWords + kSets * kCountStride) * sizeof(uint32_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        c->sched.stats_clean = 1;
        for (int k = 0; k < kSets; ++k) c->sched.counters_clean[k] = 1;
    }
    if (hand_off)
        for (int par = 0; par < (overlap ? 2 : 1); ++par)
            for (int k = 0; k < 4; ++k)
                if ((rc = c->ovf[par][k].ensure(ovf_slots))) return rc;
    if ((n_batches > 1 || fs.load || fs.store) && (rc = c->film.ensure((size_t)np * 3))) return rc;

    ptk::BounceArgs a{};
    unsigned long long* const d_stats = reinterpret_cast<unsigned long long*>(c->ovf_count.p);   // hipMalloc alignment: fine for u64
    a.stats = d_stats;
    if (!list) {   // tile row -> image row without a table (ptk::TileMap)
        const uint32_t br = prm->band_rows ? prm->band_rows : cam->height;
        a.tile.band_rows = br;
        a.tile.band_magic = br > 1 ? (uint32_t)(((1ull << 32) + br - 1) / br) : 0u;
        a.tile.band_stride = br * band_count;
        a.tile.band_first = prm->band_index * br;
    }
    a.sc = view_for(c, prm->exact_math);
    for (int k = 0; k < 3; ++k) {
        a.cam.origin[k] = (float)cam->origin[k]; a.cam.lower_left[k] = (float)cam->lower_left[k];
        a.cam.horizontal[k] = (float)cam->horizontal[k]; a.cam.vertical[k] = (float)cam->vertical[k];
    }
    a.cam.width = cam->width; a.cam.height = cam->height;
    a.pixels = list ? list->d_pixels : nullptr;
    a.film_w = list ? 65536u : cam->width;
    a.np = np;
    auto magic = [](uint32_t d) { return d <= 1u ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / d); };
    a.film_w_magic = magic(a.film_w);
    a.np_magic = magic(np);
    a.min_depth = prm->min_depth; a.max_depth = prm->max_depth;
    a.t_min = (float)prm->t_min;
    a.integrator = prm->integrator;
    a.accel = prm->accel;
    a.bvh_refill = c->tuning.bvh_refill ? std::min(64u, c->tuning.bvh_refill) : ptk::kRefillBelow;
    a.bvh_leaf = c->tuning.bvh_leaf ? c->tuning.bvh_leaf : ptk::kLeafBatch;

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

    // ---- EXECUTE
    std::vector<uint32_t> primary_events;
    uint32_t pool_begin = 0;
    auto exec = [&](const ptsched::Op& o, size_t index) -> int {
        using namespace ptsched;
        if (c->debug_fail_at >= 0 && (size_t)c->debug_fail_at == index) {
            c->debug_fail_at = -1;
            return fail(PT_ERR_HIP, "injected failure at stream operation %zu of the render (pt_debug_fail_after)", index);
        }
        hipStream_t s = sched_stream(c, st, o.stream);
        switch (o.kind) {
        case kOpHostSync:
            for (int k = 0; k < kLanes; ++k) HIP_TRY(hipStreamSynchronize(c->lane_stream[k]));
            HIP_TRY(hipStreamSynchronize(st));
            if (int r2 = c->xchg.ensure((size_t)next.xchg_stride * kLanes)) return r2;
            return PT_OK;
        case kOpMemsetStats:
            HIP_TRY(hipMemsetAsync(c->ovf_count.p, 0, kStatsWords * sizeof(uint32_t), s));
            return PT_OK;
        case kOpMemsetCounters:
            HIP_TRY(hipMemsetAsync(c->ovf_count.p + kStatsWords + kCountStride * o.set, 0, kCountStride * sizeof(uint32_t), s));
            return PT_OK;
        case kOpRecord:
            if (o.event == kEvPool && !(o.pool & 1u)) pool_begin = o.pool;
            HIP_TRY(hipEventRecord(sched_event(c, o), s));
            return PT_OK;
        case kOpWait:
            HIP_TRY(hipStreamWaitEvent(s, sched_event(c, o), 0));
            return PT_OK;
        case kOpPost:
            __atomic_store_n(c->h_posted.p, o.seq, __ATOMIC_RELEASE);      // before the launch is handed to the device
            return PT_OK;
        case kOpLaunch: {
            const uint32_t s0 = o.batch * nb_max, nb = std::min(nb_max, spp - s0);
            uint32_t* const d_count = c->ovf_count.p + kStatsWords + kCountStride * o.set;   // [0] leftovers handed over, [64 ...] chunk counters of k_paths_regen
            const bool own = o.own_queue != 0;
            a.s_base = prm->spp_offset + s0;
            a.lsamp = c->lsamp[o.set].p;
            // Level 0 traces the batch's paths (every bounce, see k_paths); in a large batch its waves hand their sparse
            // tails to the overflow queue, which level 1 -- same kernel, fixed grid, count read on the device -- finishes.
            // (a regenerating launch whose waves run dry themselves leaves nothing for a continuation launch)
            a.n_first = np * nb;
            a.n_first_dev = nullptr;
            a.seg_cap = ((((a.n_first + 63u) / 64u) + nw - 1) / nw) * 64u;
            a.src_mode = inject ? 1u : 0u;
            a.export_below = hand_off ? (small_scene ? export_small : ptk::kBlock) : 1u;
            if (o.level > 0) {
                a.n_first = 0; a.n_first_dev = d_count;
                a.seg_cap = seg_cap_cont;
                a.src_mode = 1u;
                a.export_below = 1u;
            }
            a.aux = own ? c->caux.p : c->bvh_aux.p;
            a.sray0 = own ? c->csray[0].p : c->bvh_sray[0].p;
            a.sray1 = own ? c->csray[1].p : c->bvh_sray[1].p;
            for (int k = 0; k < 4; ++k) {
                a.q.q[k] = own ? c->cqueue[k].p : c->queue[k].p;
                a.ovf_out.q[k] = hand_off ? c->ovf[o.ovf_par][k].p : nullptr;
                a.ovf_in.q[k] = inject ? const_cast<float4*>(list->inject[k]) : (hand_off ? c->ovf[o.ovf_par][k].p : nullptr);
            }
            a.ovf_out_count = d_count;
            a.debug_tag = o.set;
            a.chunk_counter = nullptr;
            a.xchg = nullptr;
            a.posted = nullptr; a.seq = 0; a.core_blocks = 0;
            a.regen_static = 0;
            if (o.flags & kLaunchRegen) {
                a.chunk_counter = d_count + ptk::kRegenCounterStride;
                if (o.flags & kLaunchSplit) a.xchg = c->xchg.p + o.xchg_off;
                a.export_below = regen_export;
                // the first kRegenStatic16 / 16 of the chunks are dealt statically (none with lanes: a workgroup of this launch that
                // only finds room when the previous launch's last waves end would carry its dealt share as a serial tail)
                const uint32_t nwr = o.grid * kWavesPerBlock, nch = (a.n_first + 63u) / 64u;
                if (o.flags & kLaunchStaticDeal) a.regen_static = (uint32_t)(((uint64_t)nch * kRegenStatic16 / 16) / nwr) * nwr;
                if (o.core) { a.posted = c->h_posted.dev; a.seq = o.seq; a.core_blocks = o.core; }
            }
            const uint32_t inst = prm->exact_math ? ptk::launch_path_kernel_exact(a, o.grid, s) : ptk::launch_path_kernel_fast(a, o.grid, s);
            HIP_TRY(hipGetLastError());
            if (c->launch_log.size() < kLaunchLogCap) c->launch_log.push_back(inst);
            if ((o.flags & kLaunchPrimary) && plan.profile) primary_events.push_back(pool_begin / 2u);
            return PT_OK;
        }
        case kOpResolve: {
            const uint32_t s0 = o.batch * nb_max, nb = std::min(nb_max, spp - s0);
            if (ad) {
                ptk::AdaptiveResolveArgs r{};
                r.f = ad->f;
                r.lsamp = c->lsamp[o.set].p;
                r.pixels = list ? list->d_pixels : nullptr;
                r.width = cam->width; r.n = np; r.nb = nb; r.n_total = ad->n_total;
                r.load = o.batch > 0 || ad->load;
                r.finalize = o.batch + 1 == n_batches;
                if (o.zero_words) { r.zero_words = c->ovf_count.p + kStatsWords + kCountStride * o.set; r.n_zero = o.zero_words; }
                ptk::launch_resolve_adaptive(r, s);
                HIP_TRY(hipGetLastError());
                return PT_OK;
            }
            ptk::ResolveArgs r{};
            r.lsamp = c->lsamp[o.set].p;
            r.film = c->film.p;
            r.out_linear = d_linear;
            r.out_rgba = d_rgba;
            r.np = np; r.nb = nb;
            r.load_film = o.batch > 0 || fs.load;
            r.store_film = o.batch + 1 < n_batches || fs.store;
            r.finalize = o.batch + 1 == n_batches;
            r.spp_div = fs.div ? fs.div : spp;
            r.out_packed = d_packed;
            if (o.zero_words) { r.zero_words = c->ovf_count.p + kStatsWords + kCountStride * o.set; r.n_zero = o.zero_words; }
            ptk::launch_resolve(r, s);
            HIP_TRY(hipGetLastError());
            return PT_OK;
        }
        default:
            return fail(PT_ERR_HIP, "internal: unknown stream operation %u", o.kind);
        }
    };
    for (size_t i = 0; i < plan.ops.size(); ++i)
        if ((rc = exec(plan.ops[i], i))) {
            const std::string keep = g_err;
            sched_recover(c, st, next);
            g_err = keep;
            return rc;
        }

    c->debug_fail_at = -1;              // (the hook is for ONE render)

    // ---- COMMIT
    if (!plan.accumulate) begin_period();
    c->sched = next;
    // (the device-side statistics are read when they are collected -- pt_sync --, not copied back per render)
    if (job.capturing) {
        // nothing ran, and the graph may be replayed any number of times: the device will have counted a multiple of these
        const uint64_t n = (uint64_t)np * spp;
        uint64_t x = c->capture_gcd, y = n;
        while (y) { const uint64_t t = x % y; x = y; y = t; }
        c->capture_gcd = x;
    } else {
        c->expected_samples += (uint64_t)np * spp;
    }
    c->stats.bounce_launches += plan.launches;
    c->stats.batches += n_batches;
    c->stats.primary_launches += plan.primary_launches;
    c->primary_events.insert(c->primary_events.end(), primary_events.begin(), primary_events.end());
    return PT_OK;
}

extern "C" {

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
    if (prm->spp == 0) return fail(PT_ERR_INVALID_ARG, "spp must be > 0");
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
    if ((prm->band_count ? prm->band_count : 1) != 1 || prm->band_index != 0)
        return fail(PT_ERR_INVALID_ARG, "pt_render_adaptive: renders the whole image (band_count = 1)");
    if (!c->has_scene) return fail(PT_ERR_INVALID_ARG, "render: no scene uploaded");
    if (cam->width < 2 || cam->height < 2) return fail(PT_ERR_INVALID_ARG, "camera %ux%u: width and height must be >= 2", cam->width, cam->height);
    const uint64_t np64 = (uint64_t)cam->width * cam->height;
    if (np64 > (1ull << 30)) return fail(PT_ERR_UNSUPPORTED, "pt_render_adaptive: %llu pixels", (unsigned long long)np64);
    const uint32_t np = (uint32_t)np64, spp_max = prm->spp, W = cam->width;
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    int rc;
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
    HIP_TRY(hipMemcpy(out_linear, c->host_lin.p, 3 * np * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, c->host_rgba.p, 4 * np, hipMemcpyDeviceToHost));
    if (out_spp) HIP_TRY(hipMemcpy(out_spp, c->ad_count.p, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_rel_err) HIP_TRY(hipMemcpy(out_rel_err, c->ad_err.p, np * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
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
