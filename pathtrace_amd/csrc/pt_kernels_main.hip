// pt_kernels_main.hip -- HIP kernels of the wavefront path tracer, gfx950 (wave64): the main translation unit
// (pt_kernels_unit.h lists the units; this comment is the overview of all of them).
//
// Every path vertex is one level of MisStrategy::ray_color / BrdfOnlyStrategy::ray_color
// (src/rendering.rs:34-142, 214-265) in the iterative order of SURVEY 3.5:
//     closest hit of the path ray            World::hit_scene      world.rs:270-290
//     miss -> retire; emitter -> credit (MIS look-ahead weight), retire
//     NEE: pick light, sample its surface    World::sample_light_point  world.rs:251-267
//          shadow scan, BSDF eval, MIS weight                      rendering.rs:55-81
//     BSDF sample, throughput, Russian roulette                    rendering.rs:83-102
//     survivors are compacted in place into the wave's own queue segment (wave64 ballot
//     + prefix popcount, no atomics); retired paths store their radiance to lsamp[pid].
// (vertex_begin / vertex_end, pt_kernels_vertex.h; shared by every path kernel.)
//
// Kernels:
//   k_paths<MODE, MIS, OVF>   one launch traces a whole sample batch, every bounce; hit_scene is the reference's
//                             linear scan, out of LDS (MODE = kModeLds, scenes <= 128 objects) or streamed through
//                             an LDS tile (kModeTiled).  Pass 0 generates the camera rays (camera.rs:139-147,
//                             world.rs:299) or, in a continuation launch (OVF), takes over the overflow queue.
//   k_paths_regen<MIS, MATS>  level-0 launch of a batch of > 2^17 paths over a scene in LDS: a path stays in its lane's registers,
//                             a lane whose path ends takes the batch's next one (chunk counters); compiled per material set.
//                             A vertex's visibility ray and the next path ray go through the scene in one pass (scan_closest2);
//                             a one-light scene of at most 16 Lambertian spheres is scanned without the run records (SPHERES) and
//                             shaded by a vertex stage compiled for sphere hits and Lambertian surfaces (LAMBERT).
//   k_paths_regen_split<..>   (pt_kernels_split.hip) the same for scenes with a few Mirror objects (the reference's own): a wave's Mirror vertices are
//                             set aside on a per-wave stack and shaded 64 at a time.
//   k_paths_bvh<MIS, OVF>     (pt_kernels_bvh.hip) the queue form for PtRenderParams.accel = 1: hit_scene by traversal of a 4-wide BVH, each pass cut
//                             into extend / connect / occlude / shade stages with per-lane ray refill.
//   k_scene_setup             per-object constants (a triangle's unit normal and 1 / area) at pt_scene_upload.
//   k_resolve                 film: per-pixel f64 sum in sample order, mean, gamma, RGBA8 (world.rs:311-332).
//   k_debug_hit[_bvh]         hit_scene on arbitrary rays (parity tests).
//
// Data layout: path state = 4 float4 planes (SoA of float4 -> every lane moves 16 B per instruction, 1 KiB per
// wave-instruction); small scenes live in LDS and are read by all 64 lanes at the same address (broadcast,
// conflict-free).  Grids are persistent (one queue segment per wave), so no host round trip sits between bounces.
#include "pt_kernels_scan.h"
#include "pt_kernels_vertex.h"

namespace PTK_IMPL {

// ------------------------------------------------------------------ the path kernel
// Queue organisation.  The path queue is cut into one PRIVATE segment per wave
// (segment w = slots [w*seg_cap, (w+1)*seg_cap)).  A wave reads its segment 64
// slots at a time (one coalesced 1 KiB access per plane), advances those paths by
// one vertex and writes the survivors back INTO THE SAME SEGMENT at its running
// output position: rank = popcount(ballot(alive) & lanemask_lt), position kept in
// a wave-uniform register.  Writes never pass the read position (out <= in), so
// the compaction is in place, needs no second queue and no global atomic.  (A
// single shared tail counter costs one returning atomic per wave per iteration:
// measured 59 ms of a 60 ms render at 1024^2 x 64 spp.)
//
// Because no wave ever touches another wave's slots, nothing forces the waves to
// advance bounce by bounce in lockstep: ONE launch runs every bounce of a batch.
// Each wave loops { pass over its segment = one more vertex for each of its paths }
// until its segment is empty.  (One launch per bounce cost ~2.5 of 13.2 ms in launch
// gaps, host polling and under-filled tail launches.)  Pass 0 deals 64-path chunks
// round-robin to the waves (chunk k -> wave k % nw) and generates the camera rays
// (Camera::get_ray_with_offset), so every segment samples the whole image and the
// waves finish together.
//
// Memory access of one iteration: the chunk's state is loaded at the top (4 x 16 B per lane, coalesced) and the
// survivors are stored at the bottom; with a scene in LDS nothing else touches global memory.  (An earlier version
// requested the NEXT chunk's state one iteration ahead.  The register allocator had to keep those 16 registers
// somewhere for a whole vertex, placed the copies -- and so the wait -- right after the loads anyway, and the
// pressure cost a wave of occupancy: without it the kernel needs 80-90 VGPRs instead of 115-128 and runs 6 waves
// per SIMD, C2 10.14 -> 9.78 ms, C1 16.1 -> 14.9 ms.)
// minimum waves per SIMD the register allocator must leave room for.  Scene in LDS: 80 VGPRs (the DIFFUSE variant
// without spilling, the generic one with 8 spilled dwords); measured 4 / 5 / 6 / 7 waves: C2 10.14 / 9.84 / 9.78 /
// 10.04 ms, C1 16.1 / 15.2 / 14.9 ms.  Tiled scan: 5 waves (96 VGPRs + 21 spilled dwords, 30 KiB tile so that five
// workgroups fit a CU): C4 1214 -> 1106 ms; 6 waves with a 24 KiB tile: the same.
#ifndef PT_BOUNCE_WAVES_LDS
#define PT_BOUNCE_WAVES_LDS 6
#endif
#ifndef PT_BOUNCE_WAVES_TILED
#define PT_BOUNCE_WAVES_TILED 5
#endif
// ... and the generic-material instances of the LDS form (GGX + OrenNayar code in the kernel): what pixel lists, pt_ray_color and
// batches of <= 2^17 paths take on the reference's own scene.  At 6 waves (80 VGPRs) they spill 14-18 registers.
#ifndef PT_BOUNCE_WAVES_LDS_GENERIC
#define PT_BOUNCE_WAVES_LDS_GENERIC 5      // round 5: 93-95 VGPRs, no spills; small jobs on World::new() 6-9 % faster than at 6 waves (profiles/r05/ab_generic_waves.txt)
#endif
template <int MODE, bool MIS, bool OVF, bool DIFFUSE, bool LIST>   // OVF: continuation launch, pass 0 reads the overflow queue
__global__ void __launch_bounds__(kBlock, MODE == kModeLds ? (DIFFUSE ? PT_BOUNCE_WAVES_LDS : PT_BOUNCE_WAVES_LDS_GENERIC) : PT_BOUNCE_WAVES_TILED)
k_paths(BounceArgs a) {
    // SMALL = "the waves of a workgroup are independent" (no barrier inside the scan): wave-private queue
    // segments.  The tiled scan ties the four waves of a workgroup together.  (kModeBvh: k_paths_bvh.)
    static_assert(MODE == kModeLds || MODE == kModeTiled, "linear-scan kernel");
    constexpr bool SMALL = MODE == kModeLds;
    extern __shared__ float4 lds[];
    __shared__ uint32_t s_iters[kBlock / 64];
    __shared__ WgTotals s_totals;
    if (threadIdx.x == 0u) wg_totals_init(s_totals);
    if (MODE != kModeLds) __syncthreads();      // (kModeLds: stage_scene's barrier publishes it)
    const SceneRef sc = stage_scene<MODE>(a.sc, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t nw = gridDim.x * (kBlock / 64);
    // SMALL: one private segment per wave.  Tiled: the four waves of a workgroup advance in lockstep anyway
    // (barriers in the scan), so they share ONE segment and compact at workgroup level: chunk c of a pass
    // goes to wave c % 4 and only the last chunk of a pass is partial (every pass costs a full scan of the
    // whole scene per wave, however few lanes are alive).
    const uint32_t wib = threadIdx.x >> 6;                       // wave in block
    uint32_t n_first, seg_cap;
    launch_shape<OVF>(a, nw, n_first, seg_cap);
    const uint32_t seg_base = SMALL ? wave * seg_cap : blockIdx.x * (kBlock / 64) * seg_cap;
    const uint32_t n_chunks = (n_first + 63u) >> 6;                // pass 0: 64-path chunks of the batch
    const uint32_t W = a.film_w;
    uint32_t n_in = 0;                     // wave-uniform: queued paths of this wave's segment
    uint32_t wave_shadow = 0, wave_vertices = 0;
    uint32_t wave_samples = 0;             // wave-uniform: paths whose radiance this wave has written to lsamp (finished samples)
    uint32_t wave_depth = 0;               // wave-uniform: deepest vertex this wave has processed
    constexpr bool from_overflow = OVF;

    for (uint32_t pass = 0;; ++pass) {
    const bool first = pass == 0u;
    // SMALL: n_in = paths of this wave's segment; tiled: n_in = paths of the workgroup's segment (same in all waves)
    const uint32_t n_iter = first ? (n_chunks + nw - 1u) / nw : (SMALL ? (n_in + 63u) >> 6 : (n_in + kBlock - 1u) / kBlock);
    if (n_iter == 0u) break;               // SMALL: this wave is done; tiled: the whole workgroup is (uniform)
    uint32_t out_n = 0;                    // wave-uniform: survivors written so far in this pass

    const uint32_t lane_off = SMALL ? lane : wib * 64u + lane;   // position inside a chunk (64 or 256 slots)
    const uint32_t chunk_slots = SMALL ? 64u : kBlock;

    for (uint32_t it = 0; it < n_iter; ++it) {
        bool active;
        PathState p;

        if (first) {
            p = parked_state();
            const uint32_t chunk = it * nw + wave;
            const uint32_t pid = chunk * 64u + lane;
            active = chunk < n_chunks && pid < n_first;
            if (active) {
                if (from_overflow) {
                    // continuation launch: the paths are the leftovers an earlier launch exported
                    unpack_ray(p, a.ovf_in.q[0][pid], a.ovf_in.q[1][pid]);
                } else {
                    uint32_t pix;
                    divmod_magic(pid, a.np, a.np_magic, p.s_local, pix);
                    divmod_magic(pix, W, a.film_w_magic, p.yl, p.px);
                }
            }
        } else {
            // every lane loads its slot (the last chunk of a pass reads stale slots of the segment: in bounds, and a
            // lane without a path only needs a ray that hits nothing -- its other fields are never looked at)
            active = it * chunk_slots + lane_off < n_in;
            const uint32_t s0 = seg_base + it * chunk_slots + lane_off;
            unpack_ray(p, a.q.q[0][s0], a.q.q[1][s0]);
            if (!active) { p.o = parked_origin(); p.d = parked_dir(); }
        }
        uint32_t kx, py;                                  // key of the path's RNG stream = (x, y), main.rs:51
        pixel_key<LIST>(a, p, active, kx, py);
        const uint32_t sample = a.s_base + p.s_local;

        if (first && !from_overflow && active) camera_ray(a.cam, sample, kx, py, p.o, p.d);
        // the CARRY part of the state (throughput, radiance, previous pdf, incoming eta) of the slot this lane works on
        auto load_carry = [&]() {
            if (!first || from_overflow) {
                const Queue& src = first ? a.ovf_in : a.q;
                const uint32_t s1 = first ? (it * nw + wave) * 64u + lane : seg_base + it * chunk_slots + lane_off;
                if (!first || active) unpack_carry(p, src.q[2][s1], src.q[3][s1]);
            }
        };

        wave_vertices += (uint32_t)__popcll(__ballot(active));
        // deepest vertex: in a level-0 launch every path of pass p is at depth p; only a continuation launch
        // mixes depths inside a wave and has to look at the lanes
        if (!from_overflow) {
            wave_depth = pass;
        } else if (__ballot(active && p.depth > wave_depth) != 0ull) {
            uint32_t v = active ? p.depth : 0u;
            for (int off = 32; off > 0; off >>= 1) { const uint32_t w2 = (uint32_t)__shfl_xor((int)v, off); v = w2 > v ? w2 : v; }
            wave_depth = __builtin_amdgcn_readfirstlane(v);
        }

        // ---- scan #1: closest hit of the path ray (rendering.rs:41)
        int id; float t;
        scan_closest<MODE, false>(sc, p.o, p.d, a.t_min, kInf, id, t);
        Vertex v;
        vertex_begin<MIS, DIFFUSE>(sc, p, active, id, t, sample, kx, py, v);

        // ---- scan #2: visibility (rendering.rs:62-65); skipped when no lane needs it
        bool visible = false;
        if (MIS) {
            bool any_shadow = SMALL ? (__ballot(v.need_shadow) != 0ull) : (__syncthreads_or(v.need_shadow) != 0);
            if (any_shadow) {
                // Ray::new (rendering.rs:62) would normalise light_dir a second time; the f32
                // arithmetic specification normalises a direction once
                f3 sdir = v.need_shadow ? v.light_dir : parked_dir();
                f3 sorg = v.need_shadow ? v.hit.point : parked_origin();
                int sid; float st;
                scan_closest<MODE, true>(sc, sorg, sdir, a.t_min, v.distance - a.t_min, sid, st);   // any-hit form
                visible = v.need_shadow && sid < 0;
                wave_shadow += (uint32_t)__popcll(__ballot(v.need_shadow));
            }
        }
        // ---- the carry part only now: none of it was needed -- or occupied a register -- during the two scans.
        // (The compiler barrier keeps the loads down here.)
        asm volatile("" ::: "memory");
        load_carry();
        const bool alive = vertex_end<MIS, DIFFUSE, SMALL>(sc, p, v, visible, sample, kx, py, a.min_depth, a.max_depth);

        // ---- retire, or compact in place into the wave's own segment
        if (active && !alive) a.lsamp[p.s_local * a.np + p.yl * W + p.px] = Rgb{p.L.x, p.L.y, p.L.z};
        wave_samples += (uint32_t)__popcll(__ballot(active && !alive));
        const unsigned long long mask = __ballot(alive);
        uint32_t cnt_before = 0, cnt_all = (uint32_t)__popcll(mask);
        if (!SMALL) {
            // workgroup-level prefix of the survivor counts (s_iters is free: the next write to it is an
            // iteration away, behind the barriers of two scans)
            if (lane == 0u) s_iters[wib] = cnt_all;
            __syncthreads();
            cnt_all = 0;
            for (uint32_t k = 0; k < kBlock / 64; ++k) { cnt_before += k < wib ? s_iters[k] : 0u; cnt_all += s_iters[k]; }
        }
        if (alive) store_state(a.q, seg_base + out_n + cnt_before + lane_rank(mask), p);
        out_n += cnt_all;
    }
    n_in = out_n;
    // the next pass reads (from other lanes of this wave -- tiled: of this workgroup) what this pass stored
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    if (!SMALL) __syncthreads();
    if (n_in < a.export_below) break;      // export_below >= 1: an empty segment always ends the wave (tiled:
    }   // pass loop                       // n_in and export_below are workgroup-uniform)

    // Tail hand-off.  Below one chunk a wave would run every further pass mostly empty (and one path trapped
    // in a glass sphere keeps it alive for 50 passes).  Instead it appends what is left to the global
    // overflow queue -- one atomic per wave per launch -- and retires; the host launches this kernel again
    // on that queue (from_overflow), where the leftovers of ~65 000 waves form dense chunks again.
    if (SMALL && n_in != 0u) {
        uint32_t base = 0;
        if (lane == 0u) base = atomicAdd(a.ovf_out_count, n_in);
        base = __shfl(base, 0);
        for (uint32_t j = lane; j < n_in; j += 64u) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) { const float4 t = a.q.q[k][seg_base + j]; a.ovf_out.q[k][base + j] = t; }
        }
    }
    if (!SMALL && n_in != 0u) {            // tiled: the workgroup exports its shared segment (< 256 paths)
        if (threadIdx.x == 0u) s_iters[0] = atomicAdd(a.ovf_out_count, n_in);
        __syncthreads();
        const uint32_t base = s_iters[0];
        if (threadIdx.x < n_in) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) { const float4 t = a.q.q[k][seg_base + threadIdx.x]; a.ovf_out.q[k][base + threadIdx.x] = t; }
        }
    }
    // totals for the host: shadow rays, vertices (= loop iterations summed over paths), deepest vertex, finished samples
    if (lane == 0u) wave_totals<MIS, !OVF>(s_totals, kBlock / 64, a.stats, wave_shadow, wave_vertices, wave_samples, wave_depth);
}

// ------------------------------------------------------------------ the path kernel, regenerating form
// Level-0 launch of a large batch over a diffuse scene in LDS (the throughput case: C2, C3, C5).  k_paths keeps a path's
// state in the queue and moves it through HBM once per vertex; here a path stays in its lane's registers from
// its camera ray to its end, and a lane whose path has ended takes the next path of the batch on the spot
// (regeneration; Novak et al. 2010).  So every lane of every wave carries a path until the batch runs out -- no
// partially filled chunks, no queue traffic, no compaction -- and the only global accesses of the loop are the
// 12 bytes a finished sample writes and the chunk counters.
//   * Work: 64-path chunks of the batch (path id = s_local * np + pixel, as in k_paths).  The first regen_static chunks
//     are dealt round-robin (chunk k -> wave k % nw), the rest is handed out by kRegenCounters global counters (counter c
//     owns the chunks = c mod kRegenCounters; one returning atomic per chunk), so that the waves finish together: they
//     do not run equally fast -- a SIMD serves its oldest wave first -- (a static deal of 15/16 of the chunks: 7.63 ms,
//     of 1/2: 6.87, of 1/4: 6.36).  ONE counter for every chunk saturates: the chip consumes ~150 chunks per microsecond and a single address takes ~85 atomics per
//     microsecond (C2 12.3 instead of 8.0 ms).
//   * Camera rays are generated for a whole chunk at a time, all 64 lanes busy, into a per-wave ring in LDS (direction +
//     film position, 20 bytes; the origin is the camera's); a lane that needs a path pops the entry of its rank among
//     the needy lanes.  Generating rays only for the lanes that need one would run the Philox + normalise code at
//     ~20 % lane utilisation in every iteration.
//   * End of the batch: when the counters are used up and a wave's ring is empty, its lanes run dry one by one.  By
//     default (export_below = 1) the wave ends with its last path and no continuation launch follows; with a larger
//     threshold it appends what is alive below it to the overflow queue, as k_paths does (measured: not faster).
//   * The results do not depend on which lane traced which path: the RNG is addressed by (pixel, sample, depth), every
//     sample has its own slot of lsamp, and the statistics are sums.
//   * Order of an iteration (MIS instances).  The visibility ray of vertex k and the path ray of vertex k + 1 both start at the
//     hit point of vertex k, and nothing of vertex k but its NEE term reads `visible` (the BSDF sample, throughput and roulette
//     do not).  So the two rays share ONE pass over the scene (scan_closest2), at the top of the NEXT iteration:
//         refill vacant lanes -> joint scan (A: pending visibility ray, B: path ray) -> vertex_finish: the pending term of
//         vertex k, L += beta_k * (visible ? direct : 0) -> vertex_begin of vertex k + 1 -> vertex_end<DEFER>: everything else
//         of vertex k + 1; its own term (old beta, direct as if visible) goes into LDS (s_park) until the next scan is through.
//     Per path the operations and their operands are those of k_paths, which keeps the two scans apart (the bit-exactness
//     oracle: test_level0_forms_give_the_same_film, the fuzz and instance tests, tests/test_gpu_joint_scan.py).  A path that
//     ends by miss, emitter or roulette has no term pending and retires at once; one that ends WITH a term pending (black
//     throughput, depth limit) keeps its lane for one more scan -- the lane is not vacant and counts as busy -- and retires
//     after vertex_finish.  When the loop ends, the terms still pending get a visibility scan of their own before the hand-over,
//     so the state a continuation launch resumes is what it always was.  wave_shadow counts a ray where its vertex asks for it.
//     BRDF-only instances have no visibility ray: one scan per iteration, as before.
//   * First vertex at the fill (DENSE0: the MIS diffuse instances, image and LIST).  A lane fresh from the ring has nothing pending:
//     in the joint scan its ray A is empty, and one lane in 4.9 is in that state.  So the chunk a wave takes from the batch runs its
//     first vertex on the spot -- 64 camera paths, a one-ray scan, vertex_begin, vertex_end<DEFER>: the main loop's functions and
//     arguments, the same bits -- and the ring holds paths at their SECOND vertex (19 words, DenseWave).  A path that ends there by
//     miss, emitter or roulette stores its radiance at once and never enters the ring (it counts as taken and finished); one that
//     ends with its term pending enters with depth 0 and takes a lane for one scan, as ever.  A chunk is taken only when lanes are
//     vacant and the ring is empty, so the ring never holds more than one chunk's survivors (64 entries), and while the chunk's
//     vertex runs the empty ring keeps twelve registers of every lane's own path.  LDS 25.6 KB per workgroup + the scene: six
//     workgroups per CU for scenes up to 78 float4 (C2: 62); VALU per launch on C2 -4.8 %, C2 +5.0 %, C3 +5.2 % (docs/EXPERIMENTS.md).
//     The other material sets keep the loop above: their entry would need the incoming eta, and they are at 95-96 VGPRs already.
// Occupancy the variants are compiled for (pt_kernels.h: the host sizes the grid by it): the DIFFUSE variant needs 80 VGPRs
// (6 waves per SIMD), the generic ones 95-96 (5; reached only with PtTuning.level0_form = 2); none spills.
// Finished samples (stats[4]; pt_sync compares the sum with pixels x spp).  The queue-form kernels count the lanes that write their
// radiance to the sample buffer (a ballot at the store).  In the regenerating kernels a lane's ONLY transition from "has a path" to
// "has none" is that store, and paths enter a wave only from its ring, so finished = (entries taken from the ring) - (paths handed
// over at the end): one scalar add per iteration on a number the loop computes anyway.  (Counting at the store itself was measured:
// a per-lane count packed into the depth word cost 1.5 % on C2 -- profiles/r05/ab_count_finished.txt; a ballot per iteration
// costs the split form two more spilled registers.)
// Workgroup size of k_paths_regen.  Its waves share nothing but the LDS copy of the scene, so a workgroup could be ONE wave --
// a wave that ends would free a slot the next launch (pt_api.cpp, lanes) can take at once, where a four-wave workgroup needs
// four slots of a CU at the same moment.  Measured (round 4, profiles/r04/ab_regen_block_64.txt): one rank's share of C2 at 8
// ranks 0.94 -> 1.00 ms, the whole image unchanged: rejected, 256 stays; the knob remains for measurements.
#ifndef PT_REGEN_BLOCK
#define PT_REGEN_BLOCK 256
#endif
constexpr uint32_t kRegenBlock = PT_REGEN_BLOCK;
// DIFFUSE = the material set the kernel is compiled for (kMatsDiffuse / kMatsNoMirror / kMatsAll); round 3 added the
// middle one: a scene with OrenNayar but no Mirror surface (material.rs:166-296) takes this kernel too by default.
// LIST (pt_render_adaptive's passes): the batch's paths come from a pixel list -- list slot pid % np, sample pid / np (the
// sample-major order of every list render); film slot i = (tile_row << 16) | x of a 65536-wide film, camera pixel and RNG
// key = pixels[i], like pixel_key<true>.
// DENSE0 (the body's own parameter; the kernel below chooses it): a path's first vertex runs where its chunk is taken from the
// batch, all 64 lanes on camera paths with a ONE-ray scan, instead of in the main loop, where a lane fresh from the ring occupies
// a slot of the joint scan with an empty ray A.  The ring then holds paths at their second vertex (DenseWave, pt_kernels_vertex.h).
// ONE_LIGHT (the body's own parameter too, chosen per launch by a wave-uniform branch on the scene's light count; DENSE0 instances
// only): the scene's one light is read once, here, into scalar registers (OneLight, pt_kernels_vertex.h) and every vertex takes it
// from there -- no lights[] read, no material and shape record of the light through per-lane addresses, no second emission read, the
// sphere-or-triangle choice a scalar branch.  Scenes with no light or several take the per-lane code.  The two forms are two
// copies of the loop in one kernel (a launch runs one of them); they share the workgroup's LDS, which is why it is declared in
// paths_regen_body and handed down (RegenLds).
// SPHERES (chosen with ONE_LIGHT, by the same wave-uniform branch): the scan array is one run of at most kSpheresOnlyMax spheres at
// offset 0, first object 0 (SceneView::spheres_only, decided at upload).  The scans enter the run's sphere code with those constants
// and the count (scan_closest / scan_closest2 <.., SPHERES>, pt_kernels_scan.h): no loop over runs, no run record out of LDS and its
// four readfirstlane, no dispatch on the tag, no triangle code in the loop; same tests, same order, same bits.  vertex_begin finishes
// every hit as a sphere's, without the shape tag of the material word.
// LAMBERT (chosen with the two above, by the same branch): every object is Lambertian or an Emissive that emits
// (SceneView::lambert_surfaces, decided at upload), so a path that goes on past a vertex stands on a Lambertian surface there.
// vertex_end re-reads the colour alone and enters the BSDF code with the tag a constant: no Emissive arms, no select of the sampled
// direction, no second normalisation, no eta (pt_kernels_vertex.h).  The kernel holds TWO loops: <ONE_LIGHT, SPHERES, LAMBERT> for
// one-light scenes of Lambertian spheres only (C2, C3, C5) and the generic per-lane one for every other scene -- a third copy (one
// light with triangles, as before the spheres form existed) spills two to five VGPRs at 80, so such scenes take the generic loop
// again, and so does a spheres-only one-light scene with a black Emissive object (docs/EXPERIMENTS.md, "A spheres-only scene ...",
// "Sphere hits and Lambertian surfaces ...").
struct RegenLds {            // one wave's parts of the workgroup's LDS
    float4* pool_d;          // !DENSE0: the ring of camera rays
    uint32_t* pool_s;
    float4 *park0, *park1;   // the lane's parked NEE term (DENSE0: park0 and park1d)
    float2* park1d;
    DenseWave* dw;           // DENSE0: ring entries and parked terms
    WgTotals* totals;
};
template <bool MIS, int DIFFUSE, bool LIST, bool DENSE0, bool ONE_LIGHT, bool SPHERES, bool LAMBERT>
PT_DEV void paths_regen_run(const BounceArgs& a, const SceneRef& sc, const RegenLds& w);

template <bool MIS, int DIFFUSE, bool LIST, bool DENSE0>
PT_DEV void paths_regen_body(const BounceArgs& a) {
    // DENSE0 rebuilds a popped path's incoming eta (1) and its pending throughput (1, 1, 1) instead of storing them: true of a
    // first vertex on a surface without refraction only
    static_assert(!DENSE0 || (MIS && DIFFUSE == kMatsDiffuse), "the dense first vertex is written for the MIS diffuse instances");
    extern __shared__ float4 lds[];
    __shared__ float4 s_pool_d[DENSE0 ? 1 : kRegenBlock / 64][DENSE0 ? 1 : kPool];      // (d.x, d.y, d.z, bits(tile_row << 16 | x))
    __shared__ uint32_t s_pool_s[DENSE0 ? 1 : kRegenBlock / 64][DENSE0 ? 1 : kPool];    // s_local << 16 (depth 0)
    __shared__ WgTotals s_totals;
    // MIS: the pending NEE term of every lane (Pending::beta, ::direct) sits here during the joint scan instead of in six registers
    // (2 KB per wave; a lane reads only what it wrote itself: no barrier)
    __shared__ float4 s_park[MIS && !DENSE0 ? kRegenBlock / 64 : 1][2][DENSE0 ? 1 : 64];
    // DENSE0: ring entries (paths at their second vertex) and the parked terms (six floats per lane), per wave
    __shared__ DenseWave s_dense[DENSE0 ? kRegenBlock / 64 : 1];
    if (threadIdx.x == 0u) wg_totals_init(s_totals);
    // Spare workgroups (BounceArgs.posted): in a sequence of overlapping launches only the first core_blocks of a launch work -- two
    // launches then sit side by side and the third fills the slots the first frees while it runs dry -- but the LAST launches of
    // a sequence, and a launch on its own, would leave half of the device empty.  So every launch brings a full device's worth of
    // workgroups, and a spare one asks, when it gets its slot, whether successors are waiting for it: yes -> it ends at once.
    if (a.posted != nullptr && blockIdx.x >= a.core_blocks) {
        __shared__ uint32_t s_posted;
        if (threadIdx.x == 0u) s_posted = __hip_atomic_load(a.posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __syncthreads();
        if (s_posted - a.seq >= 2u) return;
    }
    const SceneRef sc = stage_scene<kModeLds>(a.sc, lds);          // (its barrier also publishes the words above)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    RegenLds w;
    w.pool_d = s_pool_d[DENSE0 ? 0u : wib];
    w.pool_s = s_pool_s[DENSE0 ? 0u : wib];
    w.park0 = DENSE0 ? &s_dense[DENSE0 ? wib : 0u].park0[lane] : &s_park[MIS && !DENSE0 ? wib : 0u][0][DENSE0 ? 0u : lane];
    w.park1 = &s_park[MIS && !DENSE0 ? wib : 0u][1][DENSE0 ? 0u : lane];
    w.park1d = &s_dense[DENSE0 ? wib : 0u].park1[lane];
    w.dw = &s_dense[DENSE0 ? wib : 0u];
    w.totals = &s_totals;
    if constexpr (DENSE0) {
        if (sc.n_lights == 1u && sc.n_spheres != 0u && sc.lambert_surfaces != 0u) { paths_regen_run<MIS, DIFFUSE, LIST, DENSE0, true, true, true>(a, sc, w); return; }
    }
    paths_regen_run<MIS, DIFFUSE, LIST, DENSE0, false, false, false>(a, sc, w);
}

template <bool MIS, int DIFFUSE, bool LIST, bool DENSE0, bool ONE_LIGHT, bool SPHERES, bool LAMBERT>
PT_DEV void paths_regen_run(const BounceArgs& a, const SceneRef& sc_staged, const RegenLds& w) {
    SceneRef sc = sc_staged;
    OneLight ol = OneLight{};
    if constexpr (ONE_LIGHT) { sc.n_lights = 1u; ol = load_one_light(sc); }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    float4* const pool_d = w.pool_d;
    uint32_t* const pool_s = w.pool_s;
    float4* const park0 = w.park0;
    float4* const park1 = w.park1;
    float2* const park1d = w.park1d;
    DenseWave& dw = *w.dw;
    WgTotals& s_totals = *w.totals;
    const uint32_t n_first = a.n_first;
    const uint32_t n_chunks = (n_first + 63u) >> 6;
    const uint32_t W = a.film_w;
    const f3 cam_o = mk(a.cam.origin[0], a.cam.origin[1], a.cam.origin[2]);

    const uint32_t wave = blockIdx.x * (kRegenBlock / 64) + wib, nw = gridDim.x * (kRegenBlock / 64);
    uint32_t st_next = wave;               // wave-uniform: next chunk of the static deal
    uint32_t ctr = blockIdx.x % kRegenCounters, ctr_dry = 0;   // wave-uniform: counter in use, counters found used up
    uint32_t pool_head = 0, pool_cnt = 0;  // wave-uniform: ring read position, entries
    bool exhausted = false;                // wave-uniform: the batch has no more chunks
    uint32_t wave_shadow = 0, wave_vertices = 0;
    uint32_t wave_taken = 0;               // wave-uniform: paths this wave's lanes took from the ring (finished = taken - handed over)
    uint32_t dmax = 0;                     // per lane: deepest vertex of the paths this lane finished
    PathState p = parked_state();
    bool alive = false;
    // MIS: the NEE term of the lane's previous vertex, waiting for the visibility its ray (sdir, bound smax, from p.o) finds in
    // the joint scan of the next iteration.  pd.on && !alive: the path ended at that vertex; the lane takes no new path until the
    // term is in and the radiance stored.
    Pending pd;
    pd.on = false; pd.beta = mk(0.f, 0.f, 0.f); pd.direct = mk(0.f, 0.f, 0.f);
    f3 sdir = parked_dir();
    float smax = -1.0f;
    // a finished path: radiance to its sample slot, the lane parked until it gets its next path (end of the batch: for good)
    auto park = [&]() {
        *park0 = make_float4(pd.beta.x, pd.beta.y, pd.beta.z, pd.direct.x);
        if constexpr (DENSE0) *park1d = make_float2(pd.direct.y, pd.direct.z);
        else *park1 = make_float4(pd.direct.y, pd.direct.z, 0.0f, 0.0f);
    };
    auto unpark = [&]() {
        asm volatile("" ::: "memory");          // a real read after the scan, not the values kept alive across it
        const float4 k0 = *park0;
        float2 k1;
        if constexpr (DENSE0) k1 = *park1d;
        else { const float4 k = *park1; k1 = make_float2(k.x, k.y); }
        pd.beta = mk(k0.x, k0.y, k0.z); pd.direct = mk(k0.w, k1.x, k1.y);
    };
    auto retire = [&]() {
        a.lsamp[p.s_local * a.np + p.yl * W + p.px] = Rgb{p.L.x, p.L.y, p.L.z};
        dmax = p.depth > dmax ? p.depth : dmax;
        p.o = parked_origin(); p.d = parked_dir();
    };
#ifdef PT_DRAIN_TIMING      // measurement build: when does the batch run out under the waves, when does the last wave end
    const unsigned long long t_begin = wall_clock64();
    unsigned long long t_exhausted = 0ull;
#endif

    for (;;) {
#ifdef PT_DRAIN_TIMING
        if (exhausted && t_exhausted == 0ull) t_exhausted = wall_clock64();
#endif
        // the batch's next chunk for this wave (false: there is none left)
        auto take_chunk = [&](uint32_t& chunk) {
            if (st_next < a.regen_static) {            // dealt round-robin, like pass 0 of k_paths
                chunk = st_next; st_next += nw;
                return true;
            }
            // the shared rest: chunk regen_static + ticket * kRegenCounters + c from counter c; a wave starts at the
            // counter of its workgroup and moves on to the next one when that is used up
            for (;;) {
                uint32_t got = 0;
                if (lane == 0u) got = atomicAdd(a.chunk_counter + ctr * kRegenCounterStride, 1u);
                chunk = a.regen_static + __builtin_amdgcn_readfirstlane(got) * kRegenCounters + ctr;
                if (chunk < n_chunks) return true;
                ctr = ctr + 1u == kRegenCounters ? 0u : ctr + 1u;
                if (++ctr_dry == kRegenCounters) { exhausted = true; return false; }
            }
        };
        if constexpr (DENSE0) {
        // ---- lanes without a path take the ring's entries, in lane order; while some stay vacant, the batch's next chunk runs
        // its first vertex here, all 64 lanes on camera paths (one-ray scan, vertex_begin, vertex_end<DEFER>: the main loop's
        // functions and arguments at depth 0), and what goes on from there enters the (then empty) ring at depth 1.
        for (;;) {
            const bool vacant = !alive && !pd.on;
            const unsigned long long need = __ballot(vacant);
            const uint32_t r = lane_rank(need);
            if (vacant && r < pool_cnt) {
                const uint32_t e = pool_head + r;
                const float4 e0 = dw.e4[0][e], e1 = dw.e4[1][e], e2 = dw.e4[2][e], e3 = dw.e4[3][e];
                const uint32_t xy = dw.e1[1][e], sd = dw.e1[2][e];
                p.o = mk(e0.x, e0.y, e0.z); p.d = mk(e0.w, e1.x, e1.y);
                p.beta = mk(e1.z, e1.w, e2.x); p.pdf_prev = e2.y;
                p.L = mk(0.f, 0.f, 0.f); p.eta_in = 1.0f;     // nothing was credited at the first vertex; no refracting surface
                sdir = mk(e3.y, e3.z, e3.w); smax = __uint_as_float(dw.e1[0][e]);
                p.yl = xy >> 16; p.px = xy & 0xFFFFu;
                p.s_local = sd >> 16; p.depth = sd & 0xFFFFu;
                alive = p.depth != 0u;                         // depth 0: the path ended at its first vertex, its term is still owed
                pd.on = true; pd.beta = mk(1.f, 1.f, 1.f); pd.direct = mk(e2.z, e2.w, e3.x);
                park();
            }
            const uint32_t n_need = (uint32_t)__popcll(need);
            const uint32_t n_take = n_need < pool_cnt ? n_need : pool_cnt;
            pool_head += n_take; pool_cnt -= n_take;
            wave_taken += n_take;
            if (n_need == n_take || exhausted) break;
            uint32_t chunk;
            if (!take_chunk(chunk)) break;
            // (lanes stay vacant only when the ring ran empty: the chunk's entries start at slot 0 and never exceed 64)
            __builtin_amdgcn_wave_barrier();
            const uint32_t pid = chunk * 64u + lane;
            const uint32_t valid = n_first - chunk * 64u < 64u ? n_first - chunk * 64u : 64u;
            const bool qa = lane < valid;
            PathState q = parked_state();
            uint32_t qkx = 0u, qpy = 0u;
            if (qa) {
                uint32_t pix;
                divmod_magic(pid, a.np, a.np_magic, q.s_local, pix);
                divmod_magic(pix, W, a.film_w_magic, q.yl, q.px);
                if constexpr (LIST) { const uint2 k = a.pixels[pix]; qkx = k.x; qpy = k.y; }
                else { qkx = q.px; qpy = image_row(a.tile, q.yl); }
                camera_ray(a.cam, a.s_base + q.s_local, qkx, qpy, q.o, q.d);
            }
            // (every lane starts at the camera, so the origin stays wave-uniform through the scan; a lane past the chunk's end
            // sends the parked direction from there, and whatever it hits is not looked at)
            q.o = cam_o;
            // The lanes' own paths wait in the empty ring meanwhile -- radiance, throughput, pdf, visibility ray: twelve registers
            // the first vertex would otherwise push into scratch -- and come back before the chunk's entries are written.
            dw.e4[0][lane] = make_float4(p.L.x, p.L.y, p.L.z, p.pdf_prev);
            dw.e4[1][lane] = make_float4(p.beta.x, p.beta.y, p.beta.z, smax);
            dw.e4[2][lane] = make_float4(sdir.x, sdir.y, sdir.z, 0.0f);
            const uint32_t qsample = a.s_base + q.s_local;
            int qid; float qt;
            scan_closest<kModeLds, false, false, SPHERES>(sc, q.o, q.d, a.t_min, kInf, qid, qt);
            Vertex qv;
            vertex_begin<MIS, DIFFUSE, ONE_LIGHT, SPHERES>(sc, q, qa, qid, qt, qsample, qkx, qpy, qv, &ol);
            wave_vertices += valid;
            wave_shadow += (uint32_t)__popcll(__ballot(qv.need_shadow));
            Pending qpd;
            qpd.on = false; qpd.beta = mk(0.f, 0.f, 0.f); qpd.direct = mk(0.f, 0.f, 0.f);
            const bool qalive = vertex_end<MIS, DIFFUSE, true, true, ONE_LIGHT, LAMBERT>(sc, q, qv, false, qsample, qkx, qpy, a.min_depth, a.max_depth, &qpd, &ol);
            // miss, emitter, roulette: the sample is finished (depth 0: dmax stays); it never was in the ring, so it counts here
            const bool qdone = qa && !qalive && !qpd.on;
            if (qdone) a.lsamp[q.s_local * a.np + q.yl * W + q.px] = Rgb{q.L.x, q.L.y, q.L.z};
            wave_taken += (uint32_t)__popcll(__ballot(qdone));
            {
                asm volatile("" ::: "memory");          // a real read, not the values kept alive across the vertex
                const float4 k0 = dw.e4[0][lane], k1 = dw.e4[1][lane], k2 = dw.e4[2][lane];
                p.L = mk(k0.x, k0.y, k0.z); p.pdf_prev = k0.w;
                p.beta = mk(k1.x, k1.y, k1.z); smax = k1.w;
                sdir = mk(k2.x, k2.y, k2.z);
            }
            __builtin_amdgcn_wave_barrier();
            const bool keep = qalive || qpd.on;
            const unsigned long long km = __ballot(keep);
            if (keep) {
                const uint32_t e = lane_rank(km);
                const f3 ld = qv.light_dir;
                dw.e4[0][e] = make_float4(q.o.x, q.o.y, q.o.z, q.d.x);
                dw.e4[1][e] = make_float4(q.d.y, q.d.z, q.beta.x, q.beta.y);
                dw.e4[2][e] = make_float4(q.beta.z, q.pdf_prev, qpd.direct.x, qpd.direct.y);
                dw.e4[3][e] = make_float4(qpd.direct.z, ld.x, ld.y, ld.z);
                dw.e1[0][e] = __float_as_uint(qv.distance - a.t_min);
                dw.e1[1][e] = (q.yl << 16) | q.px;
                dw.e1[2][e] = (q.s_local << 16) | q.depth;
            }
            pool_head = 0u; pool_cnt = (uint32_t)__popcll(km);
            __builtin_amdgcn_wave_barrier();
        }
        } else {
        // ---- keep at least one chunk of camera rays in the ring
        while (!exhausted && pool_cnt < 64u) {
            uint32_t chunk;
            if (!take_chunk(chunk)) break;
            const uint32_t pid = chunk * 64u + lane;
            const uint32_t valid = n_first - chunk * 64u < 64u ? n_first - chunk * 64u : 64u;
            if (lane < valid) {
                uint32_t s_local, pix, yl, px;
                divmod_magic(pid, a.np, a.np_magic, s_local, pix);
                divmod_magic(pix, W, a.film_w_magic, yl, px);
                f3 o, d;
                if constexpr (LIST) { const uint2 k = a.pixels[pix]; camera_ray(a.cam, a.s_base + s_local, k.x, k.y, o, d); }
                else camera_ray(a.cam, a.s_base + s_local, px, image_row(a.tile, yl), o, d);
                const uint32_t e = (pool_head + pool_cnt + lane) & (kPool - 1u);
                pool_d[e] = make_float4(d.x, d.y, d.z, __uint_as_float((yl << 16) | px));
                pool_s[e] = s_local << 16;
            }
            pool_cnt += valid;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- lanes without a path take the ring's next entries, in lane order
        {
            const bool vacant = !alive && !(MIS && pd.on);
            const unsigned long long need = __ballot(vacant);
            const uint32_t r = lane_rank(need);
            if (vacant && r < pool_cnt) {
                const uint32_t e = (pool_head + r) & (kPool - 1u);
                const float4 q = pool_d[e];
                const uint32_t sd = pool_s[e];
                p.o = cam_o; p.d = mk(q.x, q.y, q.z);
                const uint32_t xy = __float_as_uint(q.w);
                p.yl = xy >> 16; p.px = xy & 0xFFFFu;
                p.s_local = sd >> 16; p.depth = 0u;
                p.beta = mk(1.f, 1.f, 1.f); p.L = mk(0.f, 0.f, 0.f);
                p.pdf_prev = 0.0f; p.eta_in = 1.0f;
                alive = true;
            }
            const uint32_t n_need = (uint32_t)__popcll(need);
            const uint32_t n_take = n_need < pool_cnt ? n_need : pool_cnt;
            pool_head += n_take; pool_cnt -= n_take;
            wave_taken += n_take;
        }
        }   // !DENSE0
        __builtin_amdgcn_wave_barrier();
        const uint32_t n_alive = (uint32_t)__popcll(__ballot(alive));
        // running dry (only once the batch is exhausted): hand the rest over.  A lane that still owes its ended path the NEE term
        // counts as busy: it took no new path above, and that must not look like the batch running out.
        const uint32_t n_busy = MIS ? (uint32_t)__popcll(__ballot(alive || pd.on)) : n_alive;
        if (n_busy < a.export_below) break;            // export_below >= 1: a wave without paths ends

        const bool active = alive;
        uint32_t kx = p.px, py = image_row(a.tile, p.yl);
        if constexpr (LIST) pixel_key<true>(a, p, active, kx, py);
        const uint32_t sample = a.s_base + p.s_local;
        wave_vertices += n_alive;

        if constexpr (MIS) {
            // ---- ONE pass over the scene for two rays from p.o: A = visibility of the previous vertex's light point (rendering.rs:62-65),
            // B = closest hit of the path ray (rendering.rs:41).  A lane with nothing pending sends its path ray as A with an empty
            // range (nothing is accepted, and its discriminants are B's: no root part runs that B's would not run anyway).
            const bool shadow = pd.on && sc.n_lights > 0u;
            int id, sid = -1; float t;
            if (__ballot(shadow) != 0ull)
                scan_closest2<kModeLds, SPHERES>(sc, p.o, shadow ? sdir : p.d, shadow ? smax : -1.0f, p.d, a.t_min, kInf, sid, id, t);
            else
                scan_closest<kModeLds, false, false, SPHERES>(sc, p.o, p.d, a.t_min, kInf, id, t);
            // ---- the previous vertex's NEE term, now that its visibility is known; a path that ended there retires
            const bool ended = pd.on && !alive;
            unpark();
            vertex_finish(p, pd, shadow && sid < 0);
            if (ended) retire();
            // ---- the new vertex up to the point where its own visibility is needed
            Vertex v;
            vertex_begin<MIS, DIFFUSE, ONE_LIGHT, SPHERES>(sc, p, active, id, t, sample, kx, py, v, &ol);
            wave_shadow += (uint32_t)__popcll(__ballot(v.need_shadow));
            alive = vertex_end<MIS, DIFFUSE, true, true, ONE_LIGHT, LAMBERT>(sc, p, v, false, sample, kx, py, a.min_depth, a.max_depth, &pd, &ol);
            sdir = v.light_dir; smax = v.distance - a.t_min;
            park();
            if (active && !alive && !pd.on) retire();
        } else {
            int id; float t;
            scan_closest<kModeLds, false, false, SPHERES>(sc, p.o, p.d, a.t_min, kInf, id, t);
            Vertex v;
            vertex_begin<MIS, DIFFUSE>(sc, p, active, id, t, sample, kx, py, v);
            alive = vertex_end<MIS, DIFFUSE, true>(sc, p, v, false, sample, kx, py, a.min_depth, a.max_depth);
            if (active && !alive) retire();
        }
    }

    // ---- the terms still pending when the loop ends (the batch ran out, or a path ended at the wave's last vertex): their
    // visibility scan on its own, as k_paths runs it
    if constexpr (MIS) {
        if (__ballot(pd.on) != 0ull) {
            const bool shadow = pd.on && sc.n_lights > 0u;
            int sid = -1; float st;
            if (__ballot(shadow) != 0ull)
                scan_closest<kModeLds, true, false, SPHERES>(sc, shadow ? p.o : parked_origin(), shadow ? sdir : parked_dir(), a.t_min, smax, sid, st);
            const bool ended = pd.on && !alive;
            unpark();
            vertex_finish(p, pd, shadow && sid < 0);
            if (ended) retire();
        }
    }

    // ---- hand-over of the paths still alive (none unless the batch ran out under them)
    {
        const unsigned long long mask = __ballot(alive);
        const uint32_t n_left = (uint32_t)__popcll(mask);
        if (n_left != 0u) {
            uint32_t base = 0;
            if (lane == 0u) base = atomicAdd(a.ovf_out_count, n_left);
            base = __builtin_amdgcn_readfirstlane(base);
            if (alive) {
                store_state(a.ovf_out, base + lane_rank(mask), p);
                const uint32_t done = p.depth ? p.depth - 1u : 0u;   // deepest vertex it has been through (0: none yet)
                dmax = done > dmax ? done : dmax;
            }
        }
        wave_taken -= n_left;
    }
    const uint32_t wave_samples = wave_taken;
    for (int off = 32; off > 0; off >>= 1) { const uint32_t w2 = (uint32_t)__shfl_xor((int)dmax, off); dmax = w2 > dmax ? w2 : dmax; }
    if (lane == 0u) {
        wave_totals<MIS>(s_totals, kRegenBlock / 64, a.stats, wave_shadow, wave_vertices, wave_samples, dmax);
#ifdef PT_DRAIN_TIMING      // stats[8..12] (beyond the 8 words the host reads): ~begin (min), ~exhausted (min), exhausted (max), end (max), sum of per-wave drain times
        const unsigned long long t_end = wall_clock64();
        if (t_exhausted == 0ull) t_exhausted = t_end;
        atomicMax(&a.stats[8], ~t_begin); atomicMax(&a.stats[9], ~t_exhausted); atomicMax(&a.stats[10], t_exhausted);
        atomicMax(&a.stats[11], t_end); atomicAdd(&a.stats[12], t_end - t_exhausted);
        // per wave: (begin, out of work, end) stamps and the vertices it processed, into the (unused) hand-over queue
        if (a.ovf_out.q[0]) a.ovf_out.q[a.debug_tag & 3u][wave] = make_float4(__uint_as_float((uint32_t)t_begin), __uint_as_float((uint32_t)t_exhausted),
                                                               __uint_as_float((uint32_t)t_end), __uint_as_float(wave_vertices));
#endif
    }
}

template <bool MIS, int DIFFUSE, bool LIST = false>
__global__ void __launch_bounds__(kRegenBlock, DIFFUSE == kMatsDiffuse ? kRegenWavesDiffuse : kRegenWavesGeneric) k_paths_regen(BounceArgs a) {
    paths_regen_body<MIS, DIFFUSE, LIST, MIS && DIFFUSE == kMatsDiffuse>(a);
}

static int scene_mode(const SceneView& sc, uint32_t accel) {
    return accel ? kModeBvh : (sc.n_objs <= kSmallObjs ? kModeLds : kModeTiled);
}
static size_t scene_lds_bytes(const SceneView& sc, int mode) {
    if (mode == kModeBvh) return (size_t)(kBvhStack + 3u) * kBlock * sizeof(uint32_t);   // + 3 rows: the traversal stores a visit's (up to) three far children before it knows how many there are
    return (mode == kModeLds ? (sc.blob_f4 ? sc.blob_f4 : 1u) : kTileF4) * sizeof(float4);
}
// the launchers return the instance code (pt_kernels.h) of the kernel they enqueue
template <int MODE, bool DIFFUSE, bool LIST>
static uint32_t launch_paths_mode(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st) {
    const bool mis = a.integrator == 0;
    const bool ovf = a.src_mode != 0u;     // continuation launch
    const dim3 g(grid), b(kBlock);
    if (mis && !ovf) hipLaunchKernelGGL((k_paths<MODE, true, false, DIFFUSE, LIST>), g, b, lds, st, a);
    else if (mis) hipLaunchKernelGGL((k_paths<MODE, true, true, DIFFUSE, LIST>), g, b, lds, st, a);
    else if (!ovf) hipLaunchKernelGGL((k_paths<MODE, false, false, DIFFUSE, LIST>), g, b, lds, st, a);
    else hipLaunchKernelGGL((k_paths<MODE, false, true, DIFFUSE, LIST>), g, b, lds, st, a);
    return instance_code(kInstPaths, MODE, mis, ovf, DIFFUSE, LIST, kExactMath);
}

}  // namespace PTK_IMPL
namespace ptk {
using namespace PTK_IMPL;
// the regenerating level-0 kernel a launch takes: compiled for the scene's material set; with the Mirror vertices batched
// (k_paths_regen_split, its own translation unit) when the host passes exchange memory
typedef void (*RegenKernel)(BounceArgs);
static RegenKernel regen_kernel(const BounceArgs& a, uint32_t* code = nullptr) {
    const bool mis = a.integrator == 0;
    if (code) *code = instance_code(kInstRegen, 0, mis, false, a.sc.diffuse_only ? kMatsDiffuse : a.sc.no_mirror ? kMatsNoMirror : kMatsAll,
                                    a.pixels != nullptr, kExactMath);
    if (a.pixels) {          // pt_render_adaptive's list passes
        if (a.sc.diffuse_only) return mis ? k_paths_regen<true, kMatsDiffuse, true> : k_paths_regen<false, kMatsDiffuse, true>;
        if (a.sc.no_mirror) return mis ? k_paths_regen<true, kMatsNoMirror, true> : k_paths_regen<false, kMatsNoMirror, true>;
        return mis ? k_paths_regen<true, kMatsAll, true> : k_paths_regen<false, kMatsAll, true>;
    }
    if (a.sc.diffuse_only) return mis ? k_paths_regen<true, kMatsDiffuse> : k_paths_regen<false, kMatsDiffuse>;
    if (a.sc.no_mirror) return mis ? k_paths_regen<true, kMatsNoMirror> : k_paths_regen<false, kMatsNoMirror>;
    return mis ? k_paths_regen<true, kMatsAll> : k_paths_regen<false, kMatsAll>;
}
// Workgroups of that kernel one CU holds at once, given the scene's LDS blob (0 if the query fails: the caller falls back
// to the compile-time occupancy).  The launch must not be larger than what is resident: the statically dealt quarter of
// the chunks of a wave that starts late is a serial tail.
uint32_t PT_LAUNCH(regen_blocks_per_cu)(const BounceArgs& a) {
    int n = 0;
    const size_t lds = scene_lds_bytes(a.sc, kModeLds);
    const uint32_t block = a.xchg ? kBlock : kRegenBlock;        // (the form that batches Mirror vertices keeps four waves per workgroup)
    if (a.xchg) n = PT_LAUNCH(regen_split_blocks_per_cu)(a, lds);
    else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, regen_kernel(a), (int)block, lds) != hipSuccess) n = -1;
    if (n < 0) return 0u;
    return (uint32_t)n * block / kBlock;                         // in units of four waves, like the grid the host passes
}
uint32_t PT_LAUNCH(launch_path_kernel)(const BounceArgs& a, uint32_t grid, hipStream_t st) {
    const int mode = scene_mode(a.sc, a.accel);
    const size_t lds = scene_lds_bytes(a.sc, mode);
    const bool diffuse = a.sc.diffuse_only != 0u;
    if (a.pixels && !(mode == kModeLds && a.chunk_counter)) {   // pixel-list renders: the generic kernels (debug / replay entries)
        if (mode == kModeLds) return launch_paths_mode<kModeLds, false, true>(a, grid, lds, st);
        if (mode == kModeTiled) return launch_paths_mode<kModeTiled, false, true>(a, grid, lds, st);
        return PT_LAUNCH(launch_paths_bvh)(a, grid, lds, st, false, true);
    }
    if (mode == kModeLds && a.chunk_counter) {   // level-0 launch of a large batch: paths stay in registers (k_paths_regen*)
        const uint32_t block = a.xchg ? kBlock : kRegenBlock;    // grid = number of 4-wave units
        BounceArgs b = a;
        b.core_blocks = a.core_blocks * kBlock / block;          // (given in four-wave units like the grid)
        const uint32_t blocks = std::max(1u, grid * kBlock / block);
        if (a.xchg) return PT_LAUNCH(launch_regen_split)(b, blocks, lds, st);
        uint32_t code = 0;
        hipLaunchKernelGGL(regen_kernel(a, &code), dim3(blocks), dim3(block), lds, st, b);
        return code;
    }
    if (mode == kModeLds) return diffuse ? launch_paths_mode<kModeLds, true, false>(a, grid, lds, st) : launch_paths_mode<kModeLds, false, false>(a, grid, lds, st);
    if (mode == kModeTiled) return launch_paths_mode<kModeTiled, false, false>(a, grid, lds, st);   // scan-dominated: the variant buys nothing (measured)
    return PT_LAUNCH(launch_paths_bvh)(a, grid, lds, st, diffuse, false);
}
}  // namespace ptk
namespace PTK_IMPL {

// ------------------------------------------------------------------ film resolve
// World::render_pixel's tail (world.rs:311-332).  One thread per tile pixel; the
// nb samples of the batch are added in sample order into an f64 sum, so the film
// does not depend on how paths were scheduled.
#ifndef PT_RESOLVE_UNROLL
#define PT_RESOLVE_UNROLL 4     // k_resolve: samples whose loads are in flight together (32 VGPRs: what is free beside six 80-VGPR waves;
#endif                          // 8 -> 56 VGPRs and C1 1.3 % slower; a raised wave priority: nothing.  profiles/r04/ab_resolve_variants.txt)
__global__ void __launch_bounds__(kBlock) k_resolve(ResolveArgs a) {
    // (With lanes -- pt_api.cpp -- a resolve becomes ready while the NEXT batch's regenerating launch holds every wave slot of
    // the device: it gets none until that launch runs dry (22 us of work took ~1 ms; a raised wave priority changes nothing,
    // the workgroups are simply not placed).  Hence the three buffer sets there: nobody waits for the resolve.)
    if (blockIdx.x == 0u && a.zero_words)
        for (uint32_t k = threadIdx.x; k < a.n_zero; k += kBlock) a.zero_words[k] = 0u;
    uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.np) return;
    double r = 0.0, g = 0.0, b = 0.0;
    if (a.load_film) { r = a.film[3 * (size_t)p]; g = a.film[3 * (size_t)p + 1]; b = a.film[3 * (size_t)p + 2]; }
    uint32_t s = 0;
#if PT_RESOLVE_UNROLL > 1
    // several samples' loads in flight before the (ordered) additions: beside resident path-kernel waves a resolve wave gets few
    // issue slots, and every exposed memory round trip counts
    for (; s + PT_RESOLVE_UNROLL <= a.nb; s += PT_RESOLVE_UNROLL) {
        Rgb v[PT_RESOLVE_UNROLL];
#pragma unroll
        for (int k = 0; k < PT_RESOLVE_UNROLL; ++k) v[k] = a.lsamp[(size_t)(s + k) * a.np + p];
#pragma unroll
        for (int k = 0; k < PT_RESOLVE_UNROLL; ++k) { r += (double)v[k].r; g += (double)v[k].g; b += (double)v[k].b; }
    }
#endif
    for (; s < a.nb; ++s) {
        const Rgb v = a.lsamp[(size_t)s * a.np + p];
        r += (double)v.r; g += (double)v.g; b += (double)v.b;                     // world.rs:311
    }
    if (a.store_film) { a.film[3 * (size_t)p] = r; a.film[3 * (size_t)p + 1] = g; a.film[3 * (size_t)p + 2] = b; }
    if (!a.finalize) return;
    double c[3] = {r / (double)a.spp_div, g / (double)a.spp_div, b / (double)a.spp_div};   // world.rs:315
    const bool want8 = a.out_rgba != nullptr || a.out_packed != nullptr;
    uint32_t q8 = 0xFF000000u;                                                    // alpha 255, world.rs:331
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (want8) {
            double gm = __builtin_sqrt(c[k]);                                     // gamma 2.0, world.rs:322-324
            double cl = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);                   // clamp keeps NaN
            double q = cl * 255.0;
            q8 |= (uint32_t)((q != q) ? (uint8_t)0 : (uint8_t)q) << (8 * k);      // `as u8`: truncation, NaN -> 0
        }
    }
    if (a.out_packed) {       // the multi-GPU send record: both film planes of the pixel in one 16-byte store
        reinterpret_cast<uint4*>(a.out_packed)[p] = make_uint4(__float_as_uint((float)c[0]), __float_as_uint((float)c[1]),
                                                               __float_as_uint((float)c[2]), q8);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.out_linear[3 * (size_t)p + k] = (float)c[k];   // luminance_data, world.rs:318-319
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * (size_t)p) = q8;
}
}  // namespace PTK_IMPL
namespace ptk {
#if !PT_MATH_EXACT      // k_resolve has no division or sqrt in f32: the fast unit's copy serves both modes
void launch_resolve(const ResolveArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(PTK_IMPL::k_resolve, dim3((a.np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
#endif
}  // namespace ptk
namespace PTK_IMPL {

// ------------------------------------------------------------------ debug: hit_scene on arbitrary rays
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_debug_hit(SceneView scv, const float* __restrict__ rays6, uint32_t n,
                                                      float t_min, float t_max, int32_t* out_id, float* out_t, float* out_rec) {
    extern __shared__ float4 lds[];
    const SceneRef sc = stage_scene<MODE>(scv, lds);
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        uint32_t i = base + threadIdx.x;
        bool active = i < n;
        f3 o = parked_origin(), d = parked_dir();
        if (active) {
            o = mk(rays6[6 * (size_t)i], rays6[6 * (size_t)i + 1], rays6[6 * (size_t)i + 2]);
            d = normalize(mk(rays6[6 * (size_t)i + 3], rays6[6 * (size_t)i + 4], rays6[6 * (size_t)i + 5]));
        }
        int id; float t;
        scan_closest<MODE>(sc, o, d, t_min, t_max, id, t);
        if (active) { out_id[i] = id; out_t[i] = id >= 0 ? t : 0.0f; }
        if (active && out_rec) store_hit_record(sc, id, o, d, t, out_rec + 8 * (size_t)i);
    }
}
// ------------------------------------------------------------------ debug: the per-vertex functions on arbitrary inputs
// One thread per item; the SAME device functions the path kernels inline (pt_device.h, sample_light_point, camera_ray).
//   kFnBsdfEval    Material::bsdf_pdf (material.rs:86-91,139-148,221-265; mirror.rs:179-198)
//                  in[10] = dir_in3, wo3, normal3, eta -> out[4] = f3, pdf
//   kFnBsdfSample  Material::bsdf_pdf_sample (material.rs:29-40, mirror.rs:200-305)
//                  in[7] = dir_in3, normal3, eta; words[4] = r1, r2, lobe u, - -> out[8] = wo3, f3, pdf, cos
//   kFnShapeSample Shape::sample_surface_from_point (shape.rs:91-145, 200-242)
//                  in[9] = from3, target3, r1, r2, with_target -> out[8] = point3, pdf_omega, light_dir3, distance
//                  (direction and distance as rendering.rs:58-60 forms them)
//   kFnLightPoint  World::sample_light_point (world.rs:251-267)
//                  in[3] = from3; words[4] = index word, r1 word, r2 word, - -> out[8] = point3, emission3, pdf, light object
//   kFnCameraRay   Camera::get_ray_with_offset with the sample's jitter draws (camera.rs:139-147, world.rs:299)
//                  words[4] = x, y (top-down film row), sample, - -> out[8] = origin3, direction3, ox, oy
__global__ void __launch_bounds__(kBlock) k_debug_fn(DebugFnArgs a) {
    extern __shared__ float4 lds[];
    const SceneRef sc = stage_scene<kModeBvh>(a.sc, lds);      // records from global memory, nothing staged
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float* in = a.in + (size_t)i * a.in_stride;
    const uint32_t* w = a.words ? a.words + 4 * (size_t)i : nullptr;
    float* out = a.out + (size_t)i * a.out_stride;
    if (a.op == kFnBsdfEval) {
        const Mat m = load_mat(sc.mat, (int)a.obj);
        f3 f; float pdf;
        bsdf_pdf(m, mk(in[0], in[1], in[2]), in[9], mk(in[3], in[4], in[5]), mk(in[6], in[7], in[8]), f, pdf);
        out[0] = f.x; out[1] = f.y; out[2] = f.z; out[3] = pdf;
    } else if (a.op == kFnBsdfSample) {
        const Mat m = load_mat(sc.mat, (int)a.obj);
        f3 wo, f; float pdf, c;
        bsdf_pdf_sample(m, mk(in[0], in[1], in[2]), in[6], mk(in[3], in[4], in[5]), w[0], w[1], w[2], wo, f, pdf, c);
        out[0] = wo.x; out[1] = wo.y; out[2] = wo.z; out[3] = f.x; out[4] = f.y; out[5] = f.z; out[6] = pdf; out[7] = c;
    } else if (a.op == kFnShapeSample) {
        const Mat m = load_mat(sc.mat, (int)a.obj);
        const f3 from = mk(in[0], in[1], in[2]);
        f3 point, dir = mk(0.f, 0.f, 0.f); float pdf, dist = 0.0f;
        const bool with_target = in[8] != 0.0f;
        shape_sample(sc.shape, sc.mat, (int)a.obj, m.shape_tag, from, with_target, mk(in[3], in[4], in[5]), in[6], in[7], point, pdf, dir, dist);
        if (with_target) {                   // look-ahead form: the sampler produces no direction; report the point's
            const f3 to_light = point - from;
            dir = normalize(to_light); dist = length(to_light);
        }
        out[0] = point.x; out[1] = point.y; out[2] = point.z; out[3] = pdf;
        out[4] = dir.x; out[5] = dir.y; out[6] = dir.z; out[7] = dist;
    } else if (a.op == kFnLightPoint) {
        f3 point = mk(0.f, 0.f, 0.f), le = point, ld = point; float pdf = 0.0f, ll = 0.0f; int lobj = -1;
        if (sc.n_lights > 0u) sample_light_point<false>(sc, mk(in[0], in[1], in[2]), w[0], w[1], w[2], point, lobj, le, pdf, ld, ll);
        out[0] = point.x; out[1] = point.y; out[2] = point.z; out[3] = le.x; out[4] = le.y; out[5] = le.z;
        out[6] = pdf; out[7] = (float)lobj;
    } else if (a.op == kFnCameraRay) {
        f3 o, d;
        camera_ray(a.cam, w[2], w[0], w[1], o, d);
        uint32_t dc[4];
        philox4x32_draw(w[0], w[1], w[2], kDepthCamera, BLK_SURFACE, 0u, dc);
        out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = d.x; out[4] = d.y; out[5] = d.z;
        out[6] = u01(dc[0]); out[7] = u01(dc[1]);
    }
}

// kFnJointScan: scan_closest2 (k_paths_regen's joint scan) beside the two scans it stands for, on arbitrary ray pairs out of LDS.
//   in[12] = origin3, dir_a3, dir_b3 (taken as given: not normalised), t_max_a, t_min, t_max_b
//   -> out[6] = joint (bits(id_a >= 0), bits(id_b), t_b), separate (bits(id >= 0) of scan_closest<ANY>, bits(id), t of scan_closest)
__global__ void __launch_bounds__(kBlock) k_debug_scan2(DebugFnArgs a) {
    extern __shared__ float4 lds[];
    const SceneRef sc = stage_scene<kModeLds>(a.sc, lds);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool active = i < a.n;
    f3 o = parked_origin(), da = parked_dir(), db = parked_dir();
    float t_max_a = -1.0f, t_min = 0.0f, t_max_b = kInf;
    if (active) {
        const float* in = a.in + (size_t)i * a.in_stride;
        o = mk(in[0], in[1], in[2]); da = mk(in[3], in[4], in[5]); db = mk(in[6], in[7], in[8]);
        t_max_a = in[9]; t_min = in[10]; t_max_b = in[11];
    }
    int ja, jb, sa, sb; float jt, st, unused;
    scan_closest2<kModeLds>(sc, o, da, t_max_a, db, t_min, t_max_b, ja, jb, jt);
    asm volatile("" ::: "memory");
    scan_closest<kModeLds, true>(sc, o, da, t_min, t_max_a, sa, unused);
    scan_closest<kModeLds, false>(sc, o, db, t_min, t_max_b, sb, st);
    if (active) {
        float* out = a.out + (size_t)i * a.out_stride;
        out[0] = __int_as_float(ja >= 0 ? 1 : 0); out[1] = __int_as_float(jb); out[2] = jt;
        out[3] = __int_as_float(sa >= 0 ? 1 : 0); out[4] = __int_as_float(sb); out[5] = st;
    }
}

// ------------------------------------------------------------------ per-object constants (pt_scene_upload)
// One thread per object: a triangle's unit normal into the spare w components of its shape record, 1 / area into the spare
// component of its material record (pt_device.h "scene records").  Evaluated by the expressions the per-vertex code
// used to run (triangle_constants), in this translation unit's arithmetic mode, on that mode's copy of the records.
__global__ void k_scene_setup(float4* shape, float4* mat, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t bits = __float_as_uint(mat[2 * i].x);
    if (((bits >> 8) & 0xFFu) != SHAPE_TRIANGLE) return;
    float4 r0 = shape[3 * i], r1 = shape[3 * i + 1], r2 = shape[3 * i + 2];
    f3 normal; float pdf_area;
    triangle_constants(mk(r1.x, r1.y, r1.z), mk(r2.x, r2.y, r2.z), normal, pdf_area);
    r0.w = normal.x; r1.w = normal.y; r2.w = normal.z;
    shape[3 * i] = r0; shape[3 * i + 1] = r1; shape[3 * i + 2] = r2;
    mat[2 * i + 1].w = pdf_area;
}
}  // namespace PTK_IMPL
namespace ptk {
using namespace PTK_IMPL;
void PT_LAUNCH(launch_scene_setup)(float4* shape, float4* mat, uint32_t n, hipStream_t st) {
    if (n == 0u) return;
    hipLaunchKernelGGL(k_scene_setup, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, shape, mat, n);
}
void PT_LAUNCH(launch_debug_fn)(const DebugFnArgs& a, hipStream_t st) {
    if (a.n == 0u) return;
    if (a.op == kFnJointScan) {
        hipLaunchKernelGGL(k_debug_scan2, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), scene_lds_bytes(a.sc, kModeLds), st, a);
        return;
    }
    hipLaunchKernelGGL(k_debug_fn, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void PT_LAUNCH(launch_debug_hit)(const SceneView& sc, uint32_t accel, const float* rays6, uint32_t n, float t_min,
                                 float t_max, float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st) {
    const int mode = scene_mode(sc, accel);
    const size_t lds = scene_lds_bytes(sc, mode);
    uint32_t grid = (n + kBlock - 1) / kBlock;
    if (grid > 2048u) grid = 2048u;
    if (grid == 0u) grid = 1u;
    if (mode == kModeLds)
        hipLaunchKernelGGL(k_debug_hit<kModeLds>, dim3(grid), dim3(kBlock), lds, st, sc, rays6, n, t_min, t_max, out_id, out_t, out_rec);
    else if (mode == kModeTiled)
        hipLaunchKernelGGL(k_debug_hit<kModeTiled>, dim3(grid), dim3(kBlock), lds, st, sc, rays6, n, t_min, t_max, out_id, out_t, out_rec);
    else
        PT_LAUNCH(launch_debug_hit_bvh)(sc, grid, lds, rays6, n, t_min, t_max, scratch, out_id, out_t, out_rec, st);
}
}  // namespace ptk
