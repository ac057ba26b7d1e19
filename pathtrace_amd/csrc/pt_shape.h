// pt_shape.h -- the launch sizing of a render as PURE functions: (scene facts, parameters, tuning, device) -> which level-0 form
// the render takes, how many batches, every grid, segment and queue size, and the per-launch words of BounceArgs.
//
// pt_api.cpp's render_impl gathers the inputs (the occupancy query and the capture status are HIP calls: they stay there and come
// in as values), calls form(), shape() and, per planned launch, launch(); it allocates and launches with what they return.
// The arithmetic carries most of the tuning measured in docs/EXPERIMENTS.md, and a slip in it shows as an overrun or a slowdown,
// not as a different film -- so it is stated once, here, and checked without a GPU: pt_debug_render_shape
// (include/pathtrace_amd.h) exposes it, tests/test_launch_shape_cpu.py holds it to a restatement and to the conditions
//   n_first <= waves * seg_cap  (a batch fits its queue segments)  and  ovf_slots <= nw_cont * seg_cap_cont  (what is handed
//   over fits the continuation launch's),
// tests/tools/launch_shape_san.cpp walks it under the sanitizers.
//
// No HIP, no allocation.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "pt_kernel_consts.h"
#include "pt_sched.h"

namespace ptshape {

constexpr uint64_t kDefaultMaxPaths = 1ull << 26;
// ... where the level-0 launch keeps its paths in registers (k_paths_regen) a path in flight costs 12 bytes of sample buffer
// instead of 76, and every batch ends in a ~0.3 ms tail: larger batches (C3: 16 instead of 64)
constexpr uint64_t kDefaultMaxPathsRegen = 1ull << 28;
constexpr uint64_t kMaxPaths = 1ull << 30;     // max_paths_in_flight is clamped to this
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

// What the sizing reads.  Plain words: the debug entry takes the same struct (PtShapeIn).
struct In {
    uint64_t np;                    // pixels of the tile / entries of the list (> 0)
    uint64_t max_paths_in_flight;   // PtRenderParams
    uint32_t spp, workgroups;
    uint32_t accel;                 // resolved: PT_ACCEL_LINEAR / PT_ACCEL_BVH
    uint32_t profile;
    uint32_t list, list_regen, inject;          // ListRender: given, may take the regenerating kernel, brings its paths
    uint32_t n_objs, blob_f4, diffuse_only;     // ptk::SceneView
    uint32_t split_ok;              // PtContext: a minority of the objects is Mirror
    uint32_t n_cus;
    uint32_t export_below, cont_workgroups, level0_form, regen_workgroups, in_order;   // PtTuning
    uint32_t capturing;             // the caller's stream is being captured into a graph
    uint32_t inject_spp;            // inject: samples per pixel the given paths bring, state s_local * np + pixel (0: one, as pt_ray_color's)
    uint32_t reserved;
};

// Which level-0 form the scene and the job can take (decided for the render by shape(), once the batch size is known).
struct Form {
    bool lds_job;        // the scene is in LDS and the job may regenerate
    bool split;          // ... with the Mirror vertices batched (k_paths_regen_split)
    bool regen_scene;    // ... in one of the regenerating forms
};
inline Form form(const In& in) {
    Form f;
    // level0_form 3 / default for scenes with a minority of Mirror objects: the regenerating form with the Mirror vertices batched
    // (a list takes the regenerating kernel only where its caller asks for it, and never the split form)
    f.lds_job = (!in.list || in.list_regen) && !in.accel && in.n_objs <= ptk::kSmallObjs && in.blob_f4 != 0;
    f.split = f.lds_job && !in.list && (in.level0_form == 3 || (in.level0_form == 0 && in.split_ok && kSplitByDefault));
    // default (round 3): every scene in LDS takes a regenerating form -- compiled for its material set (diffuse only; no
    // Mirror; everything); with the Mirror vertices batched where they are the exception (split, above).  The queue form
    // is level0_form = 1 (all-Mirror Cornell scene: queue form 12.6 ms, regenerating 10.0, split 13.8; tools/r03/mirror_forms.py)
    f.regen_scene = f.split || ((in.level0_form == 2 || in.level0_form == 0) && f.lds_job);
    return f;
}

struct Shape {
    bool over_cap;                  // the tile has more pixels than cap: nothing below is filled in
    uint64_t cap;
    uint32_t np, spp;               // spp: inject_spp (0: 1) for given paths
    uint32_t nb_max, n_batches;     // samples per pixel in a batch; batches
    uint64_t n_paths_max;           // paths of the largest batch
    uint32_t export_small, paths_per_wave;
    bool small_scene, hand_off, regen, inject, overlap;
    uint32_t grid, nw, seg_cap;     // queue-form level-0 launch: workgroups, waves, slots per wave
    uint32_t regen_per_cu, regen_capacity, regen_grid, regen_launch_grid;
    uint32_t cont_grid, nw_cont, seg_cap_cont;
    uint64_t ovf_slots, q_slots_cont, q_slots;
    uint32_t regen_export;
    ptsched::Job job;
};

// occupancy: workgroups per CU of the form's regenerating kernel with THIS scene's LDS blob as the runtime reports it (a
// 128-object scene leaves room for fewer than the compile-time figure); 0 = unknown, or not a regenerating scene.
inline Shape shape(const In& in, const Form& f, uint32_t occupancy) {
    Shape s{};
    s.cap = in.max_paths_in_flight ? in.max_paths_in_flight : (f.regen_scene ? kDefaultMaxPathsRegen : kDefaultMaxPaths);
    if (s.cap > kMaxPaths) s.cap = kMaxPaths;
    s.over_cap = in.np > s.cap;
    if (s.over_cap) return s;
    const uint32_t np = s.np = (uint32_t)in.np;
    s.inject = in.inject != 0;
    const uint32_t spp = s.spp = s.inject ? std::max(1u, in.inject_spp) : in.spp;
    s.nb_max = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(s.cap / np, 65535u), spp);
    if (s.nb_max == 0) s.nb_max = 1;
    s.n_paths_max = (uint64_t)np * s.nb_max;
    s.n_batches = (spp + s.nb_max - 1) / s.nb_max;       // (32-bit as ever: wraps for spp within 65534 of 2^32)

    // Queue segments: one per wave of the (fixed) grid; pass 0 deals 64-path chunks round-robin, so a segment holds
    // at most ceil(chunks / waves) chunks.
    s.export_small = in.export_below ? std::min(256u, std::max(1u, in.export_below)) : kExportSmall;
    const uint32_t chunks_max = (uint32_t)((s.n_paths_max + 63) / 64);
    s.grid = in.workgroups;
    s.small_scene = in.n_objs <= ptk::kSmallObjs || in.accel;     // the tiled scan exports per workgroup (< 256 paths)
    s.paths_per_wave = (in.n_objs <= ptk::kSmallObjs && !in.accel) ? kPathsPerWaveLds : kPathsPerWave;
    if (!s.grid) {
        const uint64_t want = (s.n_paths_max + (uint64_t)s.paths_per_wave * kWavesPerBlock - 1) / ((uint64_t)s.paths_per_wave * kWavesPerBlock);
        s.grid = (uint32_t)std::max<uint64_t>(want, kMinGrid);
    }
    s.grid = std::min<uint32_t>(s.grid, (chunks_max + kWavesPerBlock - 1) / kWavesPerBlock);
    if (s.grid == 0) s.grid = 1;
    s.nw = s.grid * kWavesPerBlock;
    s.seg_cap = ((chunks_max + s.nw - 1) / s.nw) * 64u;
    // Tail hand-off: the level-0 launch of a large batch exports what its waves have left below one chunk; ONE
    // continuation launch of fixed size takes that queue up.  It reads the count on the device.
    // (scenes that take a regenerating level-0 kernel have their own threshold: that launch needs no continuation launch)
    s.hand_off = !s.inject && s.n_paths_max > (f.regen_scene ? kRegenMinPaths : kExportMinPaths);
    // Such a batch over a scene in LDS takes the regenerating level-0 kernel: paths live in registers, a lane whose
    // path ends takes the next one of the batch; grid = the waves the device holds at once (k_paths_regen).
    s.regen = f.regen_scene && s.hand_off;
    // its grid = the workgroups the device holds at once: the kernel's occupancy with THIS scene's LDS blob
    s.regen_per_cu = f.split ? ptk::kRegenWavesSplit : in.diffuse_only ? ptk::kRegenWavesDiffuse : ptk::kRegenWavesGeneric;
    if (f.regen_scene && occupancy != 0u) s.regen_per_cu = std::min(s.regen_per_cu, occupancy);
    s.regen_capacity = in.n_cus * s.regen_per_cu;          // workgroups the device holds at once
    s.regen_grid = std::min(65536u, in.workgroups ? in.workgroups : in.regen_workgroups ? in.regen_workgroups : s.regen_capacity);
    s.cont_grid = in.cont_workgroups ? std::min(65536u, in.cont_workgroups) : kContGrid;
    s.nw_cont = s.cont_grid * kWavesPerBlock;
    // leftovers per wave of the level-0 launch: < export_small from a wave-private segment, < 256 per workgroup
    // (= 64 per wave) from a workgroup-shared one
    s.ovf_slots = (uint64_t)(s.regen ? s.regen_grid * kWavesPerBlock : s.nw) * std::max(s.export_small, 64u) + 64u;
    s.seg_cap_cont = (uint32_t)((((s.ovf_slots + 63) / 64 + s.nw_cont - 1) / s.nw_cont) * 64u);
    s.q_slots_cont = s.hand_off ? (uint64_t)s.nw_cont * s.seg_cap_cont : 0;
    s.q_slots = s.regen ? std::max<uint64_t>(s.q_slots_cont, 64) : std::max((uint64_t)s.nw * s.seg_cap, s.q_slots_cont);
    s.regen_export = f.split ? 1u : in.export_below ? std::min(s.export_small, 64u) : kRegenExportBelow;   // the split form has no hand-over
    // (sized by the grid the launch really takes: never more workgroups than the largest batch has chunks for)
    s.regen_launch_grid = std::min<uint32_t>(s.regen_grid, (chunks_max + kWavesPerBlock - 1) / kWavesPerBlock);
    s.overlap = s.n_batches > 1 && !s.regen;

    // ---- the job as the scheduler sees it (pt_sched.h)
    ptsched::Job& job = s.job;
    job.n_batches = s.n_batches;
    job.regen = s.regen; job.split = s.regen && f.split; job.hand_off = s.hand_off; job.regen_export = s.regen_export;
    job.profile = in.profile != 0; job.in_order = in.in_order != 0; job.capturing = in.capturing != 0;
    job.grid = s.grid; job.regen_grid = s.regen_launch_grid; job.cont_grid = s.cont_grid;
    job.regen_capacity = s.regen_capacity;
    job.fixed_grid = in.workgroups != 0 || in.regen_workgroups != 0;
    job.counter_words = kCountStride;
    job.xchg_need = job.split ? (uint64_t)s.regen_launch_grid * kWavesPerBlock * ptk::kRegenSplitF4PerWave + 1024 : 0;   // + slack: a violated stack invariant (reported) stays inside the buffer
    return s;
}

// The words of BounceArgs that depend on the launch: batch, grid, level and flags of the planned operation (ptsched::Op).
struct Launch {
    uint32_t s0, nb;                // the batch's first sample and its samples per pixel (the resolve's too)
    uint32_t n_first, seg_cap, src_mode, export_below, regen_static;
};
inline uint32_t batch_samples(const Shape& s, uint32_t batch) { return std::min(s.nb_max, s.spp - batch * s.nb_max); }   // the last batch may be short
inline Launch launch(const Shape& s, uint32_t batch, uint32_t grid, uint32_t level, uint32_t flags) {
    Launch l;
    l.s0 = batch * s.nb_max;
    l.nb = batch_samples(s, batch);
    // Level 0 traces the batch's paths (every bounce, see k_paths); in a large batch its waves hand their sparse
    // tails to the overflow queue, which level 1 -- same kernel, fixed grid, count read on the device -- finishes.
    // (a regenerating launch whose waves run dry themselves leaves nothing for a continuation launch)
    l.n_first = s.np * l.nb;
    l.seg_cap = ((((l.n_first + 63u) / 64u) + s.nw - 1) / s.nw) * 64u;
    l.src_mode = s.inject ? 1u : 0u;
    l.export_below = s.hand_off ? (s.small_scene ? s.export_small : ptk::kBlock) : 1u;
    if (level > 0) {
        l.n_first = 0;              // (read on the device: the counter the level-0 launch's waves added their leftovers to)
        l.seg_cap = s.seg_cap_cont;
        l.src_mode = 1u;
        l.export_below = 1u;
    }
    l.regen_static = 0;
    if (flags & ptsched::kLaunchRegen) {
        l.export_below = s.regen_export;
        // the first kRegenStatic16 / 16 of the chunks are dealt statically (none with lanes: a workgroup of this launch that
        // only finds room when the previous launch's last waves end would carry its dealt share as a serial tail)
        const uint32_t nwr = grid * kWavesPerBlock, nch = (l.n_first + 63u) / 64u;
        if (flags & ptsched::kLaunchStaticDeal) l.regen_static = (uint32_t)(((uint64_t)nch * kRegenStatic16 / 16) / nwr) * nwr;
    }
    return l;
}

}  // namespace ptshape
