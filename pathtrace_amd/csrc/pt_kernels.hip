// pt_kernels.hip -- HIP kernels of the wavefront path tracer, gfx950 (wave64).
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
// (vertex_begin / vertex_end below; shared by both path kernels.)
//
// Kernels:
//   k_paths<MODE, MIS, OVF>   one launch traces a whole sample batch, every bounce; hit_scene is the reference's
//                             linear scan, out of LDS (MODE = kModeLds, scenes <= 128 objects) or streamed through
//                             an LDS tile (kModeTiled).  Pass 0 generates the camera rays (camera.rs:139-147,
//                             world.rs:299) or, in a continuation launch (OVF), takes over the overflow queue.
//   k_paths_regen<MIS, MATS>  level-0 launch of a batch of > 2^17 paths over a scene in LDS: a path stays in its lane's registers,
//                             a lane whose path ends takes the batch's next one (chunk counters); compiled per material set.
//                             A vertex's visibility ray and the next path ray go through the scene in one pass (scan_closest2).
//   k_paths_regen_split<..>   the same for scenes with a few Mirror objects (the reference's own): a wave's Mirror vertices are
//                             set aside on a per-wave stack and shaded 64 at a time.
//   k_paths_bvh<MIS, OVF>     the queue form for PtRenderParams.accel = 1: hit_scene by traversal of a 4-wide BVH, each pass cut
//                             into extend / connect / occlude / shade stages with per-lane ray refill.
//   k_scene_setup             per-object constants (a triangle's unit normal and 1 / area) at pt_scene_upload.
//   k_resolve                 film: per-pixel f64 sum in sample order, mean, gamma, RGBA8 (world.rs:311-332).
//   k_debug_hit[_bvh]         hit_scene on arbitrary rays (parity tests).
//
// Data layout: path state = 4 float4 planes (SoA of float4 -> every lane moves 16 B per instruction, 1 KiB per
// wave-instruction); small scenes live in LDS and are read by all 64 lanes at the same address (broadcast,
// conflict-free).  Grids are persistent (one queue segment per wave), so no host round trip sits between bounces.
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_adaptive.h"

using namespace PTD_NS;
using namespace ptk;

#if PT_MATH_EXACT
#define PTK_IMPL ptk_exact_impl
#define PT_LAUNCH(name) name##_exact
#else
#define PTK_IMPL ptk_fast_impl
#define PT_LAUNCH(name) name##_fast
#endif

// Translation units (round 5).  The library builds this file three times per arithmetic mode, each with the compiler options its kernels
// measured best with (Makefile; profiles/r05/ab_noslp.txt, ab_bvh_slp.txt, ab_compiler_flags2.txt):
//   PT_TU = 1  everything but the two below                       -fno-slp-vectorize (C2 launch -2.6 %)
//   PT_TU = 2  k_paths_regen_split and its launcher               -fno-slp-vectorize, scheduling strategy max-ilp (C1 -1.2 %; C2 would pay 1.6 %)
//   PT_TU = 3  the BVH form (k_paths_bvh, k_debug_hit_bvh)        with the SLP vectoriser (its 4-wide box tests pack well: +2 % without)
//   PT_TU = 0  all of it in one unit (tools/resources.py, tools/build_variant.sh)
// Kernel templates are instantiated where their launcher is; the launchers that cross units are declared in pt_kernels.h.
#ifndef PT_TU
#define PT_TU 0
#endif
#define PT_TU_MAIN (PT_TU == 0 || PT_TU == 1)
#define PT_TU_SPLIT (PT_TU == 0 || PT_TU == 2)
#define PT_TU_BVH (PT_TU == 0 || PT_TU == 3)
namespace PTK_IMPL {

// ------------------------------------------------------------------ primitive tests
// SphereShape::hit (shape.rs:53-82) against the running closest t.  s = (center, r^2).
// Every ray the scans see is a unit vector (Ray::new normalises, camera.rs:10-16; so do the entries that take rays
// from outside), so the reference's a = d.d is 1 up to rounding and the f32 arithmetic specification takes a = 1: no
// multiplication by a or 1/a (SURVEY 8a row a5 prices the test that way: "16 if a = 1 and r^2 cached").
// ORDERED (BVH traversal, which meets the primitives in tree order): among equal t the highest object index
// wins -- what the scan's "accept t <= closest" gives when it walks the objects in index order.
// ANY (visibility scans): only "is anything accepted" is asked (rendering.rs:62-65 tests is_none()), and the first
// accepted object of the shrinking scan is tested against the initial t_max, so every test runs against that fixed
// bound and nothing is tracked but a flag: id >= 0.
template <bool ORDERED = false, bool ANY = false>
PT_DEV void sphere_test(float4 s, f3 o, f3 d, float t_min, float& closest, int& id, int obj) {
    f3 oc = o - mk(s.x, s.y, s.z);
    float half_b = dot(oc, d);
    // half_b^2 - c cancels catastrophically in f32 for a small sphere far from the origin;
    // same quantity, robust form: r^2 - |oc - half_b d|^2  (Ray Tracing Gems ch. 7)
    f3 l = madd(d, -half_b, oc);
    float disc = s.w - dot(l, l);
    if (disc < 0.0f) return;                       // NaN falls through, as in the reference (Q10)
    float sqrtd = pt_sqrt(disc);
    float root1 = -half_b - sqrtd;
    float root2 = -half_b + sqrtd;
    // shape.rs:76-82: take the near root unless it is out of range, then the far one.  root2 >= root1,
    // so "closest < root1" already rejects both; hence the candidate is root2 only when root1 < t_min.
    float c = root1 < t_min ? root2 : root1;
    if (c < t_min || closest < c) return;          // NaN is accepted, as in the reference
    if (ANY) { id = 0; return; }
    if (ORDERED && c == closest && obj < id) return;
    closest = c;
    id = obj;
}
// RangeInclusive(0.0..=1.0).contains(u) (shape.rs:176): true for -0.0, false for NaN.  Evaluated as "the median of (u, 0, 1) is u"
// -- one v_med3 + one compare instead of two compares and a scalar AND of their masks (the scalar ALU is one per CU; round 5: C1 launch
// 7.04-7.07 -> 7.00-7.04 ms).  Equivalent for every input: a NaN is not equal to itself, and med3(-0, 0, 1) compares equal to -0 whichever
// zero it returns.
PT_DEV bool in_unit_range(float u) {
    return __builtin_amdgcn_fmed3f(u, 0.0f, 1.0f) == u;
}
// TriangleShape::hit (shape.rs:161-192).  The reference runs Moeller-Trumbore per ray (two cross products, three dot
// products with the edges); the f32 specification evaluates the same u, v, t from per-triangle constants built once at
// upload (ptbvh::triangle_scan_record: plane normal n = e1 x e2 and the barycentric gradients N1, N2):
//     a = e1.(d x e2) = -(d.n)        t = f e2.(s x e1) = -(s.n)/(d.n)        u = (s + t d).N1        v = (s + t d).N2
// -- 19 instead of 30 arithmetic instructions and no cross product.  The accept rules are the reference's, predicate
// for predicate: |a| < 1e-8 rejects (:169), u outside [0, 1] rejects, NaN included (RangeInclusive::contains, :176),
// v < 0 or u + v > 1 rejects (:183), t outside [t_min, closest] rejects (:190); t == closest is accepted (last wins).
// They form one conjunction, so testing the t range first (it is known first here) changes nothing.
// Record: r0 = (n, N1.x), r1 = (v0, N1.y), r2 = (N1.z, N2.xyz) -- one 16-byte read per stage of the test.
template <bool ORDERED = false, bool ANY = false>
PT_DEV void triangle_test(float4 r0, float4 r1, float4 r2, f3 o, f3 d, float t_min, float& closest, int& id, int obj) {
    const f3 n = mk(r0.x, r0.y, r0.z);
    const float det = dot(d, n);
    if (__builtin_fabsf(det) < 1e-8f) return;
    const f3 s = o - mk(r1.x, r1.y, r1.z);
    const float t = pt_div(-dot(s, n), det);
    if (t < t_min || t > closest) return;
    const f3 p = madd(d, t, s);                      // hit point relative to v0
    const float u = dot(p, mk(r0.w, r1.w, r2.x));
    if (!in_unit_range(u)) return;                 // RangeInclusive::contains: NaN rejected
    const float v = dot(p, mk(r2.y, r2.z, r2.w));
    if (v < 0.0f || u + v > 1.0f) return;
    if (ANY) { id = 0; return; }
    if (ORDERED && t == closest && obj < id) return;
    closest = t;
    id = obj;
}

// Two consecutive triangles with the same v0 and the same plane normal bit for bit (kRunTrianglePair, pt_kernels.h): what
// triangle_test would compute twice -- determinant, t, the range test, the hit point -- is computed once.  The second test's
// range check "t <= closest" holds either way: closest is unchanged, or the first triangle was just accepted at this t (and
// the second, accepted too, wins the tie as the later object: world.rs:281-287).  Same results as two triangle_test calls.
// Record (pt_scene_upload): r0 = (n, -), r1 = (v0, -), r2 = (N1, N2.x), r3 = (N2.y, N2.z, N1'.x, N1'.y), r4 = (N1'.z, N2').
template <bool ANY = false>
PT_DEV void tripair_test(float4 r0, float4 r1, float4 r2, float4 r3, float4 r4, f3 o, f3 d, float t_min, float& closest, int& id, int obj) {
    const f3 n = mk(r0.x, r0.y, r0.z);
    const float det = dot(d, n);
    if (__builtin_fabsf(det) < 1e-8f) return;
    const f3 s = o - mk(r1.x, r1.y, r1.z);
    const float t = pt_div(-dot(s, n), det);
    if (t < t_min || t > closest) return;
    const f3 p = madd(d, t, s);
    const float u0 = dot(p, mk(r2.x, r2.y, r2.z));
    if (in_unit_range(u0)) {
        const float v0 = dot(p, mk(r2.w, r3.x, r3.y));
        if (!(v0 < 0.0f || u0 + v0 > 1.0f)) {
            if (ANY) { id = 0; return; }
            closest = t; id = obj;
        }
    }
    const float u1 = dot(p, mk(r3.z, r3.w, r4.x));
    if (in_unit_range(u1)) {
        const float v1 = dot(p, mk(r4.y, r4.z, r4.w));
        if (!(v1 < 0.0f || u1 + v1 > 1.0f)) {
            if (ANY) { id = 0; return; }
            closest = t; id = obj + 1;
        }
    }
}

// sphere_test in two halves: the part every sphere pays (half_b, discriminant) and the part an accepted discriminant
// pays.  Same operations in the same order per sphere; split so that a group of four can run the first halves
// back to back (four independent dependency chains) before the divergent second halves.
PT_DEV void sphere_pre(float4 s, f3 o, f3 d, float& half_b, float& disc) {
    f3 oc = o - mk(s.x, s.y, s.z);
    half_b = dot(oc, d);
    f3 l = madd(d, -half_b, oc);
    disc = s.w - dot(l, l);
}
template <bool ANY>
PT_DEV void sphere_post(float half_b, float disc, float t_min, float& closest, int& id, int obj) {
    if (disc < 0.0f) return;
    float sqrtd = pt_sqrt(disc);
    float root1 = -half_b - sqrtd;
    float root2 = -half_b + sqrtd;
    float c = root1 < t_min ? root2 : root1;
    if (c < t_min || closest < c) return;
    if (ANY) { id = 0; return; }
    closest = c;
    id = obj;
}
// disc of SphereShape::hit only (the part every sphere pays), see sphere_test
PT_DEV float sphere_disc(float4 s, f3 o, f3 d) {
    f3 oc = o - mk(s.x, s.y, s.z);
    f3 l = madd(d, -dot(oc, d), oc);
    return s.w - dot(l, l);
}

// GROUPED (large scenes, where a given sphere is rarely hit): four discriminants, ONE wave-uniform
// branch "did any lane hit any of the four?" instead of a divergent branch per sphere; the exact
// sequential tests run only then.  max() drops NaNs unless all four are NaN, which is exactly the
// NaN-ray case the reference lets through (Q10), so a NaN still reaches sphere_test.
template <bool GROUPED, bool ANY = false, bool PF = false>      // PF: the next pair's normal requested one pair ahead (the split kernel only)
PT_DEV void scan_run(const float4* __restrict__ p, uint32_t tag, uint32_t n, int first_obj, f3 o, f3 d, float t_min,
                     float& closest, int& id) {
    if (tag == SHAPE_SPHERE) {
        // four LDS reads in flight per wait instead of one
        uint32_t i = 0;
        for (; i + 4u <= n; i += 4u) {
            float4 s0 = p[i], s1 = p[i + 1], s2 = p[i + 2], s3 = p[i + 3];
            if (GROUPED) {
                float m = __builtin_fmaxf(__builtin_fmaxf(sphere_disc(s0, o, d), sphere_disc(s1, o, d)),
                                          __builtin_fmaxf(sphere_disc(s2, o, d), sphere_disc(s3, o, d)));
                if (__ballot(!(m < 0.0f)) == 0ull) continue;
            }
            if (!GROUPED) {
                // the four discriminants first, then the four root parts: four independent dependency chains for the
                // scheduler instead of one test after the other (same arithmetic; same-box A/B on C2: -0.8 %)
                float h0, h1, h2, h3, d0, d1, d2, d3;
                sphere_pre(s0, o, d, h0, d0); sphere_pre(s1, o, d, h1, d1); sphere_pre(s2, o, d, h2, d2); sphere_pre(s3, o, d, h3, d3);
                sphere_post<ANY>(h0, d0, t_min, closest, id, first_obj + (int)i);
                sphere_post<ANY>(h1, d1, t_min, closest, id, first_obj + (int)i + 1);
                sphere_post<ANY>(h2, d2, t_min, closest, id, first_obj + (int)i + 2);
                sphere_post<ANY>(h3, d3, t_min, closest, id, first_obj + (int)i + 3);
                continue;
            }
            sphere_test<false, ANY>(s0, o, d, t_min, closest, id, first_obj + (int)i);
            sphere_test<false, ANY>(s1, o, d, t_min, closest, id, first_obj + (int)i + 1);
            sphere_test<false, ANY>(s2, o, d, t_min, closest, id, first_obj + (int)i + 2);
            sphere_test<false, ANY>(s3, o, d, t_min, closest, id, first_obj + (int)i + 3);
        }
        // of the last (n mod 4) records two reads in flight at once instead of one read per test (round 5: C2's ten spheres are two
        // groups and two; launch 5.58 -> 5.52 ms, profiles/r05/ab_lds_latency.txt; three at once for n mod 4 = 3 spills four registers)
        if (!GROUPED && i + 2u <= n) {
            const float4 s0 = p[i], s1 = p[i + 1];
            float h0, h1, d0, d1;
            sphere_pre(s0, o, d, h0, d0); sphere_pre(s1, o, d, h1, d1);
            sphere_post<ANY>(h0, d0, t_min, closest, id, first_obj + (int)i);
            sphere_post<ANY>(h1, d1, t_min, closest, id, first_obj + (int)i + 1);
            i += 2u;
        }
        for (; i < n; ++i) sphere_test<false, ANY>(p[i], o, d, t_min, closest, id, first_obj + (int)i);
    } else if (tag == kRunTriangle) {
        for (uint32_t i = 0; i < n; ++i) {
            float4 a0 = p[3 * i], a1 = p[3 * i + 1], a2 = p[3 * i + 2];
            triangle_test<false, ANY>(a0, a1, a2, o, d, t_min, closest, id, first_obj + (int)i);
        }
    } else {
        if (PF) {
            // the next pair's plane normal is requested while this pair is tested (one of the three dependent LDS latencies of a pair
            // test off the critical path, for three registers: kernels with registers to spare only -- k_paths_regen_split; round 5:
            // C1 launch 7.16 -> 7.07 ms, profiles/r05/ab_lds_latency.txt)
            float4 a0n = p[0];
            for (uint32_t i = 0; i < n; ++i) {
                const float4 a0 = a0n;
                float4 a1 = p[5 * i + 1];
                if (i + 1u < n) a0n = p[5 * i + 5];
                float4 a2 = p[5 * i + 2], a3 = p[5 * i + 3], a4 = p[5 * i + 4];
                tripair_test<ANY>(a0, a1, a2, a3, a4, o, d, t_min, closest, id, first_obj + 2 * (int)i);
            }
        } else {
            for (uint32_t i = 0; i < n; ++i) {
                float4 a0 = p[5 * i], a1 = p[5 * i + 1], a2 = p[5 * i + 2], a3 = p[5 * i + 3], a4 = p[5 * i + 4];
                tripair_test<ANY>(a0, a1, a2, a3, a4, o, d, t_min, closest, id, first_obj + 2 * (int)i);
            }
        }
    }
}

// How a kernel finds the closest hit:
//   kModeLds    scenes of <= kSmallObjs objects: everything is in LDS (the blob of SceneView, copied once per
//               workgroup), linear scan
//   kModeTiled  larger scenes: the scan array streams through one LDS tile (block-uniform loop, barriers), the
//               per-object records are gathered from global memory, linear scan
//   kModeBvh    accel = 1: per-lane BVH traversal out of global memory / L2 (stack in LDS, no barriers)
// (kModeLds = 0, kModeTiled = 1, kModeBvh = 2: pt_kernels.h, which the launch log's instance codes share)
struct SceneRef {
    const float4* scan;     // SMALL: LDS scan array; else: the LDS tile buffer
    const float4* shape;
    const float4* mat;
    const Run* runs;
    const uint32_t* lights;
    const float4* scan_global;
    const Run* runs_global;
    uint32_t n_runs, n_lights;
    BvhView bvh;
    uint32_t* stack;        // kModeBvh: LDS traversal stack, entry e of thread t at stack[e * kBlock + t]
};
template <int MODE>
PT_DEV SceneRef stage_scene(const SceneView& sc, float4* lds) {
    SceneRef r;
    r.n_runs = sc.n_runs; r.n_lights = sc.n_lights;
    r.scan_global = sc.scan;
    r.runs_global = sc.runs;
    r.bvh = sc.bvh;
    r.stack = reinterpret_cast<uint32_t*>(lds);
    if (MODE == kModeLds) {
        for (uint32_t k = threadIdx.x; k < sc.blob_f4; k += blockDim.x) lds[k] = sc.blob[k];      // (k_paths_regen runs smaller workgroups)
        __syncthreads();
        r.scan = lds;
        r.shape = lds + sc.scan_f4;
        r.mat = lds + sc.scan_f4 + 3u * sc.n_objs;
        r.runs = reinterpret_cast<const Run*>(lds + sc.scan_f4 + 5u * sc.n_objs);
        r.lights = reinterpret_cast<const uint32_t*>(lds + sc.scan_f4 + 5u * sc.n_objs + sc.n_runs);
    } else {
        r.scan = lds;
        r.shape = sc.shape; r.mat = sc.mat; r.runs = sc.runs; r.lights = sc.lights;
    }
    return r;
}

// hit_scene by BVH traversal (traverse_segment below).  Every primitive whose test the linear scan would have
// accepted is still tested: a subtree is skipped only if the ray misses its box, enlarged by `pad` on every
// side, inside [t_min, closest].  pad = 2^-15 (|o|_1 + scene extent) is ~100x the rounding error of the
// primitive tests (their error scales with the distance between ray origin and primitive), so a hit that exists
// only through rounding (a grazing ray) is inside the padded box as well.  Rays with a non-finite coordinate or
// a zero direction (the reference lets NaN through its sphere test, Q10) take the linear scan, from global
// memory (scan_global).  A visibility query only uses "is there a hit": the lane stops at its first accepted
// primitive.
constexpr float kBvhPad = 1.0f / 32768.0f;
PT_DEV void scan_global(const SceneRef& sc, f3 o, f3 d, float t_min, float t_max, int& id_out, float& t_out);

// World::hit_scene (world.rs:270-290): linear scan in object order with a
// shrinking t_max.  kModeLds: the whole scan array already sits in LDS.  kModeTiled:
// every run is streamed through one LDS tile; the loop is block-uniform (all
// threads of the workgroup call this together, active or not).
template <int MODE, bool ANY = false, bool PF = false>
PT_DEV void scan_closest(const SceneRef& sc, f3 o, f3 d, float t_min, float t_max, int& id_out, float& t_out) {
    constexpr bool SMALL = MODE == kModeLds;
    float closest = t_max;
    int id = -1;
    for (uint32_t r = 0; r < sc.n_runs; ++r) {
        Run run = sc.runs[r];
        // the run record is the same in every lane: keep it (and the loop counters and object indices derived
        // from it) in scalar registers
        run.tag = __builtin_amdgcn_readfirstlane(run.tag); run.first_obj = __builtin_amdgcn_readfirstlane(run.first_obj);
        run.count = __builtin_amdgcn_readfirstlane(run.count); run.off4 = __builtin_amdgcn_readfirstlane(run.off4);
        const uint32_t per = run_entry_f4(run.tag);
        if (SMALL) {
            scan_run<false, ANY, PF>(sc.scan + run.off4, run.tag, run.count, (int)run.first_obj, o, d, t_min, closest, id);
        } else {
            float4* tile = const_cast<float4*>(sc.scan);
            const uint32_t tile_prims = kTileF4 / per;
            for (uint32_t p0 = 0; p0 < run.count; p0 += tile_prims) {
                uint32_t np = run.count - p0 < tile_prims ? run.count - p0 : tile_prims;
                __syncthreads();
                const float4* src = sc.scan_global + run.off4 + p0 * per;
                for (uint32_t k = threadIdx.x; k < np * per; k += kBlock) tile[k] = src[k];
                __syncthreads();
                scan_run<true, ANY>(tile, run.tag, np, (int)(run.first_obj + p0 * (run.tag == kRunTrianglePair ? 2u : 1u)), o, d, t_min, closest, id);
            }
        }
    }
    id_out = id;
    t_out = closest;
}
// ------------------------------------------------------------------ two rays from one origin in one pass over the scene
// k_paths_regen's visibility ray of vertex k and path ray of vertex k + 1 both start at the hit point of vertex k.  scan_closest2
// takes them through the records together: ray A is the visibility query (ANY: fixed bound t_max_a, only "anything accepted":
// id_a >= 0), ray B the closest-hit query (shrinking bound, (id, t)).  Per record and per ray the operations are those of
// scan_run<false, true> / scan_run<false, false>, in the same order, with the same NaN and tie rules; shared are the record read
// and oc = o - centre (s = o - v0 for triangles): the same subtraction of the same operands, so identical bits.  The scheduler gets
// two independent dependency chains per record.
PT_DEV void sphere_pre2(float4 s, f3 o, f3 da, f3 db, float& half_a, float& disc_a, float& half_b, float& disc_b) {
    const f3 oc = o - mk(s.x, s.y, s.z);
    half_a = dot(oc, da);
    half_b = dot(oc, db);
    const f3 la = madd(da, -half_a, oc);
    const f3 lb = madd(db, -half_b, oc);
    disc_a = s.w - dot(la, la);
    disc_b = s.w - dot(lb, lb);
}
// (the root parts stay two branches: both behind one branch "either discriminant accepted" interleaves the chains in the ISA and
// was measured slower -- docs/EXPERIMENTS.md, "One scene pass for shadow ray and next path ray")
PT_DEV void sphere_post2(float ha, float da, float hb, float db, float t_min, float bound_a, int& id_a, float& closest, int& id, int obj) {
    sphere_post<true>(ha, da, t_min, bound_a, id_a, obj);
    sphere_post<false>(hb, db, t_min, closest, id, obj);
}
PT_DEV void scan_run2(const float4* __restrict__ p, uint32_t tag, uint32_t n, int first_obj, f3 o, f3 da, f3 db, float t_min,
                      float bound_a, int& id_a, float& closest, int& id) {
    if (tag == SHAPE_SPHERE) {
        uint32_t i = 0;
        for (; i + 4u <= n; i += 4u) {
            const float4 s0 = p[i], s1 = p[i + 1], s2 = p[i + 2], s3 = p[i + 3];
            float ha0, ha1, ha2, ha3, da0, da1, da2, da3, hb0, hb1, hb2, hb3, db0, db1, db2, db3;
            sphere_pre2(s0, o, da, db, ha0, da0, hb0, db0); sphere_pre2(s1, o, da, db, ha1, da1, hb1, db1);
            sphere_pre2(s2, o, da, db, ha2, da2, hb2, db2); sphere_pre2(s3, o, da, db, ha3, da3, hb3, db3);
            sphere_post2(ha0, da0, hb0, db0, t_min, bound_a, id_a, closest, id, first_obj + (int)i);
            sphere_post2(ha1, da1, hb1, db1, t_min, bound_a, id_a, closest, id, first_obj + (int)i + 1);
            sphere_post2(ha2, da2, hb2, db2, t_min, bound_a, id_a, closest, id, first_obj + (int)i + 2);
            sphere_post2(ha3, da3, hb3, db3, t_min, bound_a, id_a, closest, id, first_obj + (int)i + 3);
        }
        if (i + 2u <= n) {
            const float4 s0 = p[i], s1 = p[i + 1];
            float ha0, ha1, da0, da1, hb0, hb1, db0, db1;
            sphere_pre2(s0, o, da, db, ha0, da0, hb0, db0); sphere_pre2(s1, o, da, db, ha1, da1, hb1, db1);
            sphere_post2(ha0, da0, hb0, db0, t_min, bound_a, id_a, closest, id, first_obj + (int)i);
            sphere_post2(ha1, da1, hb1, db1, t_min, bound_a, id_a, closest, id, first_obj + (int)i + 1);
            i += 2u;
        }
        for (; i < n; ++i) {
            float ha0, da0, hb0, db0;
            sphere_pre2(p[i], o, da, db, ha0, da0, hb0, db0);
            sphere_post2(ha0, da0, hb0, db0, t_min, bound_a, id_a, closest, id, first_obj + (int)i);
        }
    } else if (tag == kRunTriangle) {
        // one record read, the two existing tests (their s = o - v0 is one common subexpression)
        for (uint32_t i = 0; i < n; ++i) {
            const float4 a0 = p[3 * i], a1 = p[3 * i + 1], a2 = p[3 * i + 2];
            float ca = bound_a;
            triangle_test<false, true>(a0, a1, a2, o, da, t_min, ca, id_a, first_obj + (int)i);
            triangle_test<false, false>(a0, a1, a2, o, db, t_min, closest, id, first_obj + (int)i);
        }
    } else {
        for (uint32_t i = 0; i < n; ++i) {
            const float4 a0 = p[5 * i], a1 = p[5 * i + 1], a2 = p[5 * i + 2], a3 = p[5 * i + 3], a4 = p[5 * i + 4];
            float ca = bound_a;
            tripair_test<true>(a0, a1, a2, a3, a4, o, da, t_min, ca, id_a, first_obj + 2 * (int)i);
            tripair_test<false>(a0, a1, a2, a3, a4, o, db, t_min, closest, id, first_obj + 2 * (int)i);
        }
    }
}
// id_a >= 0: something lies on ray A inside [t_min, t_max_a]; (id_b, t_b): World::hit_scene of ray B, as scan_closest gives it
template <int MODE>
PT_DEV void scan_closest2(const SceneRef& sc, f3 o, f3 da, float t_max_a, f3 db, float t_min, float t_max_b, int& id_a, int& id_b,
                          float& t_b) {
    static_assert(MODE == kModeLds, "the whole scan array in LDS");
    float closest = t_max_b;
    int ia = -1, ib = -1;
    for (uint32_t r = 0; r < sc.n_runs; ++r) {
        Run run = sc.runs[r];
        run.tag = __builtin_amdgcn_readfirstlane(run.tag); run.first_obj = __builtin_amdgcn_readfirstlane(run.first_obj);
        run.count = __builtin_amdgcn_readfirstlane(run.count); run.off4 = __builtin_amdgcn_readfirstlane(run.off4);
        scan_run2(sc.scan + run.off4, run.tag, run.count, (int)run.first_obj, o, da, db, t_min, t_max_a, ia, closest, ib);
    }
    id_a = ia; id_b = ib; t_b = closest;
}
// the same scan with every record read from global memory (no LDS, no barrier: any subset of lanes may call it)
PT_DEV void scan_global(const SceneRef& sc, f3 o, f3 d, float t_min, float t_max, int& id_out, float& t_out) {
    float closest = t_max;
    int id = -1;
    for (uint32_t r = 0; r < sc.n_runs; ++r) {
        const Run run = sc.runs_global[r];
        scan_run<false>(sc.scan_global + run.off4, run.tag, run.count, (int)run.first_obj, o, d, t_min, closest, id);
    }
    id_out = id;
    t_out = closest;
}

// Ray given to lanes that carry no path (or need no shadow ray).  It must FAIL every sphere
// discriminant with a finite negative number: a zero ray gives a = 0, 1/a = inf, disc = NaN, and a
// NaN falls through to the hit branch (reference semantics, Q10) -- one dead lane then drags its
// whole wave through the sqrt/root logic of every sphere (measured on C4: 0.6 transcendental
// instructions per sphere test).  From 3e18 along +x every |oc - (oc.d)d|^2 is ~1.8e37.
PT_DEV f3 parked_origin() { return mk(3e18f, 3e18f, 3e18f); }
PT_DEV f3 parked_dir() { return mk(1.0f, 0.0f, 0.0f); }

// number of set bits of a wave mask below this lane (v_mbcnt: no lane-mask registers to keep)
PT_DEV uint32_t lane_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// n / d and n % d for n < 2^32 with the host's magic = floor(2^32 / d) (d >= 2; 0xFFFFFFFF for d = 1): umulhi is at
// most one below the quotient.  Replaces the compiler's division sequence, whose reciprocals sat in VGPRs for the
// whole kernel.
PT_DEV void divmod_magic(uint32_t n, uint32_t d, uint32_t magic, uint32_t& q, uint32_t& r) {
    q = __umulhi(n, magic);
    r = n - q * d;
    if (r >= d) { q += 1u; r -= d; }
}
// tile row -> image row (TileMap)
PT_DEV uint32_t image_row(const TileMap& t, uint32_t yl) {
    uint32_t q = t.band_rows == 1u ? yl : __umulhi(yl, t.band_magic);
    return q * t.band_stride + t.band_first + (yl - q * t.band_rows);
}

// End of a wave: its statistics go to the launch's totals.  Every wave adding them to the same five global words itself is
// ~30 000 atomics on ONE cache line per launch, serialised in L2 at the very end of the launch, where every microsecond is tail
// (measured: the fifth word, the finished-sample count, alone cost 1.5 % of a C2 launch: profiles/r05/ab_count_finished.txt).
// So the waves of a workgroup add up in LDS first and the LAST of them to end does the global atomics: a quarter of the traffic.
struct WgTotals { uint32_t done, shadow, vertices, samples, dmax; };
PT_DEV void wg_totals_init(WgTotals& t) {                 // by one thread, before the workgroup's first barrier
    t.done = 0u; t.shadow = 0u; t.vertices = 0u; t.samples = 0u; t.dmax = 0u;
}
// called by lane 0 of every wave that ran (spare workgroups that end at once never get here); waves_in_block of them
template <bool MIS, bool PRIMARY = true>     // PRIMARY: a level-0 launch (its vertices also count as primary_vertices)
PT_DEV void wave_totals(WgTotals& t, uint32_t waves_in_block, unsigned long long* stats, uint32_t shadow, uint32_t vertices,
                        uint32_t samples, uint32_t dmax) {
    if (MIS && shadow != 0u) __hip_atomic_fetch_add(&t.shadow, shadow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (vertices != 0u) __hip_atomic_fetch_add(&t.vertices, vertices, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (samples != 0u) __hip_atomic_fetch_add(&t.samples, samples, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (vertices != 0u) __hip_atomic_fetch_max(&t.dmax, dmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    // (acq_rel: the sums of the waves that ended earlier are visible to the one that finds itself last)
    if (__hip_atomic_fetch_add(&t.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) + 1u != waves_in_block) return;
    shadow = __hip_atomic_load(&t.shadow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    vertices = __hip_atomic_load(&t.vertices, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    samples = __hip_atomic_load(&t.samples, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    dmax = __hip_atomic_load(&t.dmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (MIS && shadow != 0u) atomicAdd(&stats[0], (unsigned long long)shadow);
    if (vertices != 0u) atomicAdd(&stats[1], (unsigned long long)vertices);
    if (PRIMARY && vertices != 0u) atomicAdd(&stats[3], (unsigned long long)vertices);
    if (vertices != 0u) atomicMax(&stats[2], (unsigned long long)dmax);
    if (samples != 0u) atomicAdd(&stats[4], (unsigned long long)samples);
}

// ------------------------------------------------------------------ one path vertex
// The per-vertex body of MisStrategy::ray_color / BrdfOnlyStrategy::ray_color (rendering.rs:34-142,
// 214-265), cut at the visibility scan: vertex_begin (hit record, emitter credit, light sample) -> shadow
// scan -> vertex_end (NEE term, BSDF sample, roulette, next ray).
struct PathState {
    f3 o, d, beta, L;
    float pdf_prev, eta_in;
    uint32_t s_local, depth, px, yl;
};
struct Vertex {
    Hit hit;
    Mat m;
    bool alive;              // the path continues past this vertex (so far)
    bool need_shadow;        // a light point was sampled: visibility of light_dir up to distance is needed
    f3 light_dir, ls_emission;
    float distance, ls_pdf;
    uint32_t w_bsdf1, w_bsdf2;   // the vertex's BSDF words of BLK_SURFACE (drawn together with the light words)
    uint32_t w_lobe;             // its lobe word of BLK_CHOICE, when vertex_begin had to draw that block (several lights)
    uint32_t w_rr;               // its roulette word (made of the BLK_SURFACE bits u01() skips)
    int obj, light_obj;          // object hit (>= 0) and light picked: vertex_end can re-read their records (REMAT)
    bool hit_emitter;            // the path ray reached an emitter: vertex_end credits it (it needs the carry state)
    float emit_pdf_shape;        // ... with the light pdf of that point seen from the previous vertex (MIS, depth > 0)
};

// Queue planes (pt_kernels.h): the RAY part of the state -- what the closest-hit scan and the light sample need --
// is planes 0 and 1; the CARRY part -- throughput, radiance so far, the previous sampling pdf, the incoming eta --
// is planes 2 and 3 and is only looked at once the vertex's scans are through (k_paths loads it that late, so those
// eight values do not occupy registers during the scans).
PT_DEV void unpack_ray(PathState& p, float4 q0, float4 q1) {
    p.o = mk(q0.x, q0.y, q0.z); p.d = mk(q0.w, q1.x, q1.y);
    const uint32_t xy = __float_as_uint(q1.z), sd = __float_as_uint(q1.w);
    p.yl = xy >> 16; p.px = xy & 0xFFFFu;
    p.s_local = sd >> 16; p.depth = sd & 0xFFFFu;
}
PT_DEV void unpack_carry(PathState& p, float4 q2, float4 q3) {
    p.beta = mk(q2.x, q2.y, q2.z); p.pdf_prev = q2.w;
    p.L = mk(q3.x, q3.y, q3.z); p.eta_in = q3.w;
}
PT_DEV PathState unpack_state(float4 q0, float4 q1, float4 q2, float4 q3) {
    PathState p;
    unpack_ray(p, q0, q1);
    unpack_carry(p, q2, q3);
    return p;
}
PT_DEV void store_state(const Queue& q, uint32_t j, const PathState& p) {
    q.q[0][j] = make_float4(p.o.x, p.o.y, p.o.z, p.d.x);
    q.q[1][j] = make_float4(p.d.y, p.d.z, __uint_as_float((p.yl << 16) | p.px), __uint_as_float((p.s_local << 16) | p.depth));
    q.q[2][j] = make_float4(p.beta.x, p.beta.y, p.beta.z, p.pdf_prev);
    q.q[3][j] = make_float4(p.L.x, p.L.y, p.L.z, p.eta_in);
}
PT_DEV PathState parked_state() {
    PathState p;
    p.o = parked_origin(); p.d = parked_dir(); p.beta = mk(1.f, 1.f, 1.f); p.L = mk(0.f, 0.f, 0.f);
    p.pdf_prev = 0.0f; p.eta_in = 1.0f;
    p.s_local = 0; p.depth = 0; p.px = 0; p.yl = 0;
    return p;
}

// Camera::get_ray_with_offset for sample `sample` of pixel (px, py) (camera.rs:139-147; jitter draws world.rs:299)
PT_DEV void camera_ray(const CameraF& cam, uint32_t sample, uint32_t px, uint32_t py, f3& o, f3& d) {
    uint32_t dc[4];
    philox4x32_draw(px, py, sample, kDepthCamera, BLK_SURFACE, 0u, dc);
    float ox = u01(dc[0]), oy = u01(dc[1]);                               // world.rs:299 (ox first)
    // (The divisors go through an empty asm: the compiler otherwise hoists their reciprocals out of the path loop of the
    // regenerating kernels into two registers that live -- or are spilled -- for the whole kernel; camera rays are generated once
    // per 64-path chunk, two reciprocals there cost nothing.  Same arithmetic.)
    float wm1 = (float)(cam.width - 1u), hm1 = (float)(cam.height - 1u);
    asm volatile("" : "+v"(wm1), "+v"(hm1));
    float u = pt_div((float)px + ox, wm1);                                   // camera.rs:140
    float v = pt_div((float)(cam.height - 1u - py) + oy, hm1);               // world.rs:299 y flip
    const f3 cam_o = mk(cam.origin[0], cam.origin[1], cam.origin[2]);
    f3 dir = mk(cam.lower_left[0], cam.lower_left[1], cam.lower_left[2]) +
             mk(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]) * u +
             mk(cam.vertical[0], cam.vertical[1], cam.vertical[2]) * v - cam_o;   // camera.rs:143-144
    o = cam_o;
    d = normalize(dir);                                                   // Ray::new, camera.rs:13
}

// World::sample_light_point (world.rs:251-267) from `from`: w_index = the light-index word, w_r1 / w_r2 = the surface words.
// n_lights > 0.
// dir / dist: unit direction and distance from `from` to the point (rendering.rs:58-60), from the sampler itself.
// Material sets a kernel (or a part of one) is compiled for: vertex_begin / vertex_end / sample_light_point take one as
// their second template argument (bool DIFFUSE converts: false = every material, true = Lambertian + emissive only).
//   kMatsAll       every material
//   kMatsDiffuse   Lambertian and emissive only (scene property, decided at pt_scene_upload): no GGX, no OrenNayar code
//   kMatsNoMirror  everything but Mirror (the plain iterations of k_paths_regen_split, which hand Mirror vertices on)
//   kMatsMirror    the object HIT is a Mirror (the batches of k_paths_regen_split: every entry of the special stack is one);
//                  says nothing about the light's material
// (kMatsAll = 0, kMatsDiffuse = 1, kMatsNoMirror = 2, kMatsMirror = 3: pt_kernels.h)
template <int MATS>
PT_DEV void assume_mats(uint32_t tag) {
    if (MATS == kMatsDiffuse) __builtin_assume(tag <= MAT_EMISSIVE);
    if (MATS == kMatsNoMirror) __builtin_assume(tag != MAT_MIRROR);
    if (MATS == kMatsMirror) __builtin_assume(tag == MAT_MIRROR);
}
template <int DIFFUSE>
PT_DEV void sample_light_point(const SceneRef& sc, f3 from, uint32_t w_index, uint32_t w_r1, uint32_t w_r2, f3& point,
                               int& lobj, f3& emission, float& pdf, f3& dir, float& dist) {
    const uint32_t li = __umulhi(w_index, sc.n_lights);                           // random_range(0..n), world.rs:255
    lobj = (int)sc.lights[li];
    const Mat lm = load_mat(sc.mat, lobj);
    if (DIFFUSE != kMatsMirror) assume_mats<DIFFUSE>(lm.tag);
    float pdf_shape;
    shape_sample(sc.shape, sc.mat, lobj, lm.shape_tag, from, false, from, u01(w_r1), u01(w_r2), point, pdf_shape, dir, dist);
    emission = lm.color;                                                          // world.rs:259
    pdf = sc.n_lights == 1u ? pdf_shape : pt_div(pdf_shape, (float)sc.n_lights);  // world.rs:260 (x/1 == x)
}

// (id, t) = closest hit of the path ray, id < 0: miss.  Notes an emitter hit and samples the light point.  Reads only the
// RAY part of p (origin, direction, depth, film position).
// DIFFUSE: the scene has Lambertian and emissive materials only (decided at pt_scene_upload); the GGX and
// OrenNayar code is then compiled out of the kernel (same results; smaller code, no spills at 6 waves/SIMD: C2 +2 %).
// (kx, py) = the pixel's RNG key (main.rs:51); it is the path's film position except in pixel-list renders.
template <bool MIS, int DIFFUSE>
PT_DEV void vertex_begin(const SceneRef& sc, PathState& p, bool active, int id, float t, uint32_t sample, uint32_t kx,
                         uint32_t py, Vertex& v) {
    v.alive = active && id >= 0;
    v.obj = id >= 0 ? id : 0; v.light_obj = 0;
    v.hit_emitter = false; v.emit_pdf_shape = 0.0f;
    v.hit.point = p.o; v.hit.normal = p.d; v.hit.t = 0.0f; v.hit.front_face = false;
    v.m.tag = MAT_LAMBERT; v.m.shape_tag = 0; v.m.emits = 0; v.m.color = mk(0.f, 0.f, 0.f);
    v.m.roughness = 0.f; v.m.metallic = 0.f; v.m.ior = 1.f; v.m.on_a = 1.f; v.m.on_b = 0.f;
    if (v.alive) {
        v.m = load_mat(sc.mat, id);
        assume_mats<DIFFUSE>(v.m.tag);
        v.hit = finish_hit(sc.shape, id, v.m.shape_tag, p.o, p.d, t);
        if (v.m.emits) {
            v.hit_emitter = true;
            if (MIS && p.depth != 0u) {
                // emitter reached by a BSDF-sampled ray: its MIS weight (vertex_end) is against the light pdf of
                // this point seen from the previous vertex = this ray's origin (rendering.rs:107-116)
                f3 sp, sd; float sl;
                shape_sample(sc.shape, sc.mat, id, v.m.shape_tag, p.o, true, v.hit.point, 0.f, 0.f, sp, v.emit_pdf_shape, sd, sl);
            }
            v.alive = false;
        }
    }

    // ---- draws of the vertex; NEE: light pick + surface sample (world.rs:251-267)
    v.need_shadow = false;
    v.light_dir = mk(0.f, 0.f, 0.f); v.ls_emission = mk(0.f, 0.f, 0.f);
    v.distance = 0.0f; v.ls_pdf = 1.0f;
    v.w_bsdf1 = v.w_bsdf2 = v.w_lobe = v.w_rr = 0u;
    if (v.alive) {
        uint32_t ds[4];
        philox4x32_draw(kx, py, sample, p.depth, BLK_SURFACE, 0u, ds);
        v.w_bsdf1 = ds[2]; v.w_bsdf2 = ds[3];
        v.w_rr = (ds[0] << 23) | ((ds[1] & 0x1FFu) << 14) | ((ds[2] & 0x1FFu) << 5);   // roulette word: the bits of the block u01() skips
        if (MIS && sc.n_lights > 0u) {
            uint32_t w_index = 0u;                                                // umulhi(u, 1) = 0: one light needs no draw
            if (sc.n_lights > 1u) {
                uint32_t dc[4];
                philox4x32_draw(kx, py, sample, p.depth, BLK_CHOICE, 0u, dc);
                w_index = dc[0]; v.w_lobe = dc[1];
            }
            f3 lp;                                                                // rendering.rs:58-60: direction and distance
            sample_light_point<DIFFUSE>(sc, v.hit.point, w_index, ds[0], ds[1], lp, v.light_obj, v.ls_emission, v.ls_pdf,
                                        v.light_dir, v.distance);                 // to the point, from the sampler itself
            v.need_shadow = true;
        }
    }
}

// visible: the shadow scan found nothing between the vertex and the light point.  Returns "the path goes on";
// p is then the state at the next vertex.
// REMAT (scene in LDS): the material of the hit object and the light's emission are read again here instead of
// being carried across the visibility scan -- two broadcast LDS reads instead of ~6 live registers, which is what
// keeps the kernel at 80 VGPRs without spills.
// DEFER (k_paths_regen, whose visibility scan runs together with the next closest-hit scan): `visible` is not known yet.  The NEE
// term is evaluated as if visible and, where the original adds it to L, handed to `pd` together with the throughput it is to
// be multiplied with; vertex_finish adds it -- or exactly 0 -- once the scan is through.  Nothing else of the vertex reads
// `visible`, and nothing touches L in between, so a path's arithmetic is unchanged.  A path that ends here with its term
// pending (black throughput, depth limit) keeps the hit point as p.o: its visibility ray starts there.
struct Pending {
    bool on;                 // L = L + beta * (visible ? direct : 0) is still to be done
    f3 beta, direct;
};
PT_DEV void vertex_finish(PathState& p, Pending& pd, bool visible) {
    if (pd.on) {
        const f3 direct = visible ? pd.direct : mk(0.f, 0.f, 0.f);
        p.L = p.L + pd.beta * direct;
        pd.on = false;
    }
}
template <bool MIS, int DIFFUSE, bool REMAT, bool DEFER = false>
PT_DEV bool vertex_end(const SceneRef& sc, PathState& p, const Vertex& vin, bool visible, uint32_t sample, uint32_t kx,
                       uint32_t py, uint32_t min_depth, uint32_t max_depth, Pending* pd = nullptr) {
    const uint32_t n_lights = sc.n_lights;
    Vertex v = vin;
    if (REMAT) {
        asm volatile("" ::: "memory");          // a real re-read, not the values of vertex_begin kept alive
        v.m = load_mat(sc.mat, vin.obj);
        v.ls_emission = load_mat(sc.mat, vin.light_obj).color;
    }
    if (DIFFUSE != kMatsMirror) assume_mats<DIFFUSE>(v.m.tag);
    else if (vin.alive) assume_mats<DIFFUSE>(v.m.tag);         // (a lane without a path re-reads object 0's material)
    if (vin.hit_emitter) {
        if (!MIS || p.depth == 0u) {
            p.L = p.L + p.beta * v.m.color;                                       // rendering.rs:44-45 / :225-227
        } else {
            float w_bsdf = pt_div(p.pdf_prev, p.pdf_prev + vin.emit_pdf_shape);   // :117 (Q2: not / n_lights)
            p.L = p.L + p.beta * v.m.color * w_bsdf;                              // :119-121
        }
    }
    f3 direct = mk(0.f, 0.f, 0.f);
    if (MIS && (DEFER ? vin.need_shadow : visible)) {
        float cos_theta = __builtin_fabsf(dot(v.hit.normal, v.light_dir));    // rendering.rs:68
        f3 bsdf; float pdf_bsdf;
        bsdf_pdf(v.m, p.d, p.eta_in, v.light_dir, v.hit.normal, bsdf, pdf_bsdf);   // :71-72 (stale eta, Q5)
        float w_nee = pt_div(v.ls_pdf, v.ls_pdf + pdf_bsdf);                       // :73
        direct = w_nee * bsdf * v.ls_emission * cos_theta / v.ls_pdf;         // :75-76
    }

    // ---- BSDF sample, throughput, Russian roulette (rendering.rs:83-102)
    bool alive = v.alive;
    if (alive) {
        // BLK_CHOICE: already drawn by vertex_begin when the scene has several lights; otherwise only a Mirror
        // surface (lobe) reads it
        uint32_t w_lobe = v.w_lobe, w_rr = v.w_rr;
        if (!(MIS && n_lights > 1u) && v.m.tag == MAT_MIRROR) {
            uint32_t dc[4];
            philox4x32_draw(kx, py, sample, p.depth, BLK_CHOICE, 0u, dc);
            w_lobe = dc[1];
        }
        float eta_mat = v.m.tag == MAT_MIRROR ? v.m.ior : 1.0f;               // get_eta, material.rs:50 / mirror.rs:317
        float eta_here = v.hit.front_face ? pt_rcp(eta_mat) : eta_mat;         // rendering.rs:20-25
        f3 wo, bsdf; float pdf, cos_theta;
        bsdf_pdf_sample(v.m, p.d, eta_here, v.hit.normal, v.w_bsdf1, v.w_bsdf2, w_lobe, wo, bsdf, pdf, cos_theta);   // :84-85
        f3 next_tp = p.beta * bsdf * cos_theta / pdf;                         // :89
        float rr = rr_prob(p.depth, min_depth, max_depth, next_tp);           // :91-98
        if (u01(w_rr) > rr) {                                                 // :100-102 (drops direct, Q1)
            alive = false;
        } else {
            if (DEFER) { pd->on = true; pd->beta = p.beta; pd->direct = direct; }
            else p.L = p.L + p.beta * direct;
            p.beta = rr == 1.0f ? next_tp : next_tp / rr;                     // :129 (x * (1/1) == x exactly)
            if (is_zero(p.beta) || p.depth >= 65534u) {                       // Q7: nothing downstream contributes
                alive = false;
                if (DEFER) p.o = v.hit.point;
            } else {
                p.pdf_prev = pdf;
                p.o = v.hit.point;
                p.d = v.m.tag == MAT_EMISSIVE ? normalize(wo) : wo;           // Ray::new, :86; every sampler but
                                                                              // Emissive's returns a normalised wo
                p.eta_in = eta_here;                                          // :87
                p.depth += 1u;
            }
        }
    }
    return alive;
}

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
// film position of a path -> its pixel: the RNG key (x, y) and camera pixel.  LIST: looked up in the pixel list.
// A lane without a path may carry stale slot contents as its film position (k_paths reads whole chunks): it must not
// index the list with them.
template <bool LIST>
PT_DEV void pixel_key(const BounceArgs& a, const PathState& p, bool active, uint32_t& kx, uint32_t& py) {
    if (LIST) { const uint2 k = a.pixels[active ? ((p.yl << 16) | p.px) : 0u]; kx = k.x; py = k.y; }
    else { kx = p.px; py = image_row(a.tile, p.yl); }
}
// a continuation launch whose path count is only known on the device: count, chunks and segment size from there
template <bool OVF>
PT_DEV void launch_shape(const BounceArgs& a, uint32_t nw, uint32_t& n_first, uint32_t& seg_cap) {
    n_first = a.n_first; seg_cap = a.seg_cap;
    if (OVF && a.n_first_dev) {
        n_first = __builtin_amdgcn_readfirstlane(*a.n_first_dev);
        seg_cap = ((((n_first + 63u) >> 6) + nw - 1u) / nw) * 64u;
    }
}
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
// Occupancy the variants are compiled for (pt_kernels.h: the host sizes the grid by it): the DIFFUSE variant needs 80 VGPRs
// (6 waves per SIMD), the generic ones 95-96 (5; reached only with PtTuning.level0_form = 2); none spills.
// Finished samples (stats[4]; pt_sync compares the sum with pixels x spp).  The queue-form kernels count the lanes that write their
// radiance to the sample buffer (a ballot at the store).  In the regenerating kernels a lane's ONLY transition from "has a path" to
// "has none" is that store, and paths enter a wave only from its ring, so finished = (entries taken from the ring) - (paths handed
// over at the end): one scalar add per iteration on a number the loop computes anyway.  (Counting at the store itself was measured:
// a per-lane count packed into the depth word cost 1.5 % on C2 -- profiles/r05/ab_count_finished.txt; a ballot per iteration
// costs the split form two more spilled registers.)
constexpr uint32_t kPool = 128;            // ring entries per wave (>= 2 chunks: refilled whenever fewer than 64 are left)
// Workgroup size of k_paths_regen.  Its waves share nothing but the LDS copy of the scene, so a workgroup could be ONE wave --
// a wave that ends would free a slot the next launch (pt_api.cpp, lanes) can take at once, where a four-wave workgroup needs
// four slots of a CU at the same moment.  Measured (round 4, profiles/r04/ab_regen_block_64.txt): one rank's share of C2 at 8
// ranks 0.94 -> 1.00 ms, the whole image unchanged: rejected, 256 stays; the knob remains for measurements.
#ifndef PT_REGEN_BLOCK
#define PT_REGEN_BLOCK 256
#endif
constexpr uint32_t kRegenBlock = PT_REGEN_BLOCK;
#ifndef PT_RESOLVE_UNROLL
#define PT_RESOLVE_UNROLL 4     // k_resolve: samples whose loads are in flight together (32 VGPRs: what is free beside six 80-VGPR waves;
#endif                          // 8 -> 56 VGPRs and C1 1.3 % slower; a raised wave priority: nothing.  profiles/r04/ab_resolve_variants.txt)
// DIFFUSE = the material set the kernel is compiled for (kMatsDiffuse / kMatsNoMirror / kMatsAll); round 3 added the
// middle one: a scene with OrenNayar but no Mirror surface (material.rs:166-296) takes this kernel too by default.
// LIST (pt_render_adaptive's passes): the batch's paths come from a pixel list -- list slot pid % np, sample pid / np (the
// sample-major order of every list render); film slot i = (tile_row << 16) | x of a 65536-wide film, camera pixel and RNG
// key = pixels[i], like pixel_key<true>.
template <bool MIS, int DIFFUSE, bool LIST = false>
__global__ void __launch_bounds__(kRegenBlock, DIFFUSE == kMatsDiffuse ? kRegenWavesDiffuse : kRegenWavesGeneric) k_paths_regen(BounceArgs a) {
    extern __shared__ float4 lds[];
    __shared__ float4 s_pool_d[kRegenBlock / 64][kPool];      // (d.x, d.y, d.z, bits(tile_row << 16 | x))
    __shared__ uint32_t s_pool_s[kRegenBlock / 64][kPool];    // s_local << 16 (depth 0)
    __shared__ WgTotals s_totals;
    // MIS: the pending NEE term of every lane (Pending::beta, ::direct) sits here during the joint scan instead of in six registers
    // (2 KB per wave; a lane reads only what it wrote itself: no barrier)
    __shared__ float4 s_park[MIS ? kRegenBlock / 64 : 1][2][64];
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
    float4* const pool_d = s_pool_d[wib];
    uint32_t* const pool_s = s_pool_s[wib];
    float4* const park0 = &s_park[MIS ? wib : 0u][0][lane];
    float4* const park1 = &s_park[MIS ? wib : 0u][1][lane];
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
        *park1 = make_float4(pd.direct.y, pd.direct.z, 0.0f, 0.0f);
    };
    auto unpark = [&]() {
        asm volatile("" ::: "memory");          // a real read after the scan, not the values kept alive across it
        const float4 k0 = *park0, k1 = *park1;
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
        // ---- keep at least one chunk of camera rays in the ring
        while (!exhausted && pool_cnt < 64u) {
            uint32_t chunk;
            if (st_next < a.regen_static) {            // dealt round-robin, like pass 0 of k_paths
                chunk = st_next; st_next += nw;
            } else {
                // the shared rest: chunk regen_static + ticket * kRegenCounters + c from counter c; a wave starts at the
                // counter of its workgroup and moves on to the next one when that is used up
                for (;;) {
                    uint32_t got = 0;
                    if (lane == 0u) got = atomicAdd(a.chunk_counter + ctr * kRegenCounterStride, 1u);
                    chunk = a.regen_static + __builtin_amdgcn_readfirstlane(got) * kRegenCounters + ctr;
                    if (chunk < n_chunks) break;
                    ctr = ctr + 1u == kRegenCounters ? 0u : ctr + 1u;
                    if (++ctr_dry == kRegenCounters) { exhausted = true; break; }
                }
                if (exhausted) break;
            }
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
                scan_closest2<kModeLds>(sc, p.o, shadow ? sdir : p.d, shadow ? smax : -1.0f, p.d, a.t_min, kInf, sid, id, t);
            else
                scan_closest<kModeLds, false>(sc, p.o, p.d, a.t_min, kInf, id, t);
            // ---- the previous vertex's NEE term, now that its visibility is known; a path that ended there retires
            const bool ended = pd.on && !alive;
            unpark();
            vertex_finish(p, pd, shadow && sid < 0);
            if (ended) retire();
            // ---- the new vertex up to the point where its own visibility is needed
            Vertex v;
            vertex_begin<MIS, DIFFUSE>(sc, p, active, id, t, sample, kx, py, v);
            wave_shadow += (uint32_t)__popcll(__ballot(v.need_shadow));
            alive = vertex_end<MIS, DIFFUSE, true, true>(sc, p, v, false, sample, kx, py, a.min_depth, a.max_depth, &pd);
            sdir = v.light_dir; smax = v.distance - a.t_min;
            park();
            if (active && !alive && !pd.on) retire();
        } else {
            int id; float t;
            scan_closest<kModeLds, false>(sc, p.o, p.d, a.t_min, kInf, id, t);
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
                scan_closest<kModeLds, true>(sc, shadow ? p.o : parked_origin(), shadow ? sdir : parked_dir(), a.t_min, smax, sid, st);
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

// ------------------------------------------------------------------ the regenerating form for scenes with a few Mirror (GGX) objects
// The reference's own scene (World::new(), world.rs:80-211) is 12 Lambertian / emissive triangles and ONE rough-glass
// sphere.  In k_paths_regen paths of every depth share a wave, so nearly every iteration has a lane or two on the glass
// and the whole GGX code (bsdf_pdf + VNDF sample + the lobe's Philox block, ~350-500 instructions) runs at a few percent
// lane utilisation: C1 costs 37.5 us per million vertices against 26.3 for the same geometry with a Lambertian sphere
// (tools/r03/c1_ggx_cost.py).  This form separates the two populations IN TIME inside each wave:
//   * plain iterations are k_paths_regen's, compiled without the Mirror code (kMatsNoMirror).  A lane whose path ray
//     turns out to hit a Mirror object (known after the closest-hit scan) does not shade it: it pushes the path -- the
//     state BEFORE the vertex plus the scan's (id, t) -- onto the wave's SPECIAL stack and takes a new path like a lane
//     whose path has ended.
//   * when 64 Mirror vertices have piled up (or nothing else is left to do) the wave parks its 64 plain paths in LDS (round 4;
//     round 3: in global memory), pops 64 special entries -- whole, into the registers the parked paths left -- and runs ONE
//     vertex for them with every lane on the GGX code (vertex_begin / scan / vertex_end of kMatsAll), then the closest-hit scan
//     of their NEXT vertex, the survivors staying in registers: Mirror again (a path inside the sphere) -> back onto the special
//     stack with its (id, t); anything else -> onto the wave's PLAIN stack, from which the regeneration step of the plain
//     iterations takes entries before it takes camera rays.  Then the plain paths come back into the lanes.
// Both stacks share one 128-entry region per wave in global memory (L2-resident: 10 KB per wave), special growing up, plain
// growing down.  They cannot collide.  Let S, P be the entries of the two stacks.  At the top of an iteration S <= 63 (batches
// run whenever >= 64 specials wait).  A plain iteration finds f <= 64 Mirror vertices; each of the first min(f, P) takes an
// entry OFF the plain stack as it puts one ON the special stack (round 5: S + P unchanged), the others push
// with the plain stack empty, so afterwards S + P <= max(S + P before, 63 + 64).  A batch takes 64 entries off the special
// stack and puts at most 64 back on either: S + P does not grow.  Hence S + P <= 127 < 128 always.  (Round 3-4 form, without
// the replacement: lanes take plain entries before camera rays, so a push finds the plain stack empty.)  No atomics, no other
// wave involved; a violated invariant sets stats[7] and pt_sync fails.
// Same per-vertex functions on the same inputs as every other form (a path's arithmetic does not depend on which lane
// or in which order it is traced), so the film is bit-identical (test_level0_forms_give_the_same_film, the fuzz tests).
constexpr int kWaitVm0 = 0x0F70;                                 // s_waitcnt vmcnt(0) alone (gfx9 encoding: expcnt 7, lgkmcnt 15 = no wait)
constexpr uint32_t kXq = 128;                                    // exchange entries per wave
constexpr uint32_t kXqEntryF4 = 5;                               // stack entry: 4 float4 of path state (layout of Queue) + (bits(id), t, -, -)
constexpr uint32_t kXqF4PerWave = kXq * kXqEntryF4;               // the stacks (round 3 also parked the wave's 64 plain paths here: LDS since round 4, ab_c1_park_in_lds.txt)
constexpr bool kSplitPairPrefetch = true;                          // scan_run's PF in this kernel (registers to spare)
static_assert(kXqF4PerWave == kRegenSplitF4PerWave, "pt_kernels.h sizes the buffer");
// One wave-uniform base pointer (two scalar registers); entry-major, so the planes of an entry are immediate offsets of
// ONE address -- with plane-major arrays the compiler kept a scalar base per plane (24 SGPRs more than the kernel has).
struct XWave {
    float4* b;
    PT_DEV float4* entry(uint32_t e) const { return b + e * kXqEntryF4; }                  // [0..3] state, [4] = (bits(id), t, -, -) of a special entry's pending vertex
};
PT_DEV XWave xwave(float4* base, uint32_t wave_uniform) {
    XWave x;
    x.b = base + (size_t)wave_uniform * kXqF4PerWave;
    return x;
}
PT_DEV void store_entry(float4* e, const PathState& p) {
    e[0] = make_float4(p.o.x, p.o.y, p.o.z, p.d.x);
    e[1] = make_float4(p.d.y, p.d.z, __uint_as_float((p.yl << 16) | p.px), __uint_as_float((p.s_local << 16) | p.depth));
    e[2] = make_float4(p.beta.x, p.beta.y, p.beta.z, p.pdf_prev);
    e[3] = make_float4(p.L.x, p.L.y, p.L.z, p.eta_in);
}
PT_DEV bool is_mirror_obj(const SceneRef& sc, int id) { return (__float_as_uint(sc.mat[2 * id].x) & 0xFFu) == MAT_MIRROR; }

// PLAIN = the material set of the plain iterations: kMatsDiffuse when the scene has no OrenNayar surface either (the
// reference scene: exactly k_paths_regen<MIS, DIFFUSE>'s code there), else kMatsNoMirror.
template <bool MIS, int PLAIN>
__global__ void __launch_bounds__(kBlock, kRegenWavesSplit) k_paths_regen_split(BounceArgs a) {
    extern __shared__ float4 lds[];
    __shared__ float4 s_pool_d[kBlock / 64][kPool];
    __shared__ uint32_t s_pool_s[kBlock / 64][kPool];
    __shared__ float4 s_stage[kBlock / 64][4][64];       // the parking area of each wave's plain paths during a batch of specials (plane-major: conflict-free)
    __shared__ WgTotals s_totals;
    if (threadIdx.x == 0u) wg_totals_init(s_totals);
    if (a.posted != nullptr && blockIdx.x >= a.core_blocks) {       // spare workgroup (see k_paths_regen)
        __shared__ uint32_t s_posted;
        if (threadIdx.x == 0u) s_posted = __hip_atomic_load(a.posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __syncthreads();
        if (s_posted - a.seq >= 2u) return;
    }
    const SceneRef sc = stage_scene<kModeLds>(a.sc, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    float4* const pool_d = s_pool_d[wib];
    uint32_t* const pool_s = s_pool_s[wib];
    float4 (*const park)[64] = s_stage[wib];             // the wave's plain paths while a batch of specials runs
    const uint32_t n_first = a.n_first;
    const uint32_t n_chunks = (n_first + 63u) >> 6;
    const uint32_t W = a.film_w;
    const f3 cam_o = mk(a.cam.origin[0], a.cam.origin[1], a.cam.origin[2]);

    const uint32_t wave = blockIdx.x * (kBlock / 64) + wib, nw = gridDim.x * (kBlock / 64);
    const XWave x = xwave(a.xchg, __builtin_amdgcn_readfirstlane(wave));
    uint32_t st_next = wave;
    uint32_t ctr = blockIdx.x % kRegenCounters, ctr_dry = 0;
    uint32_t pool_head = 0, pool_cnt = 0;
    bool exhausted = false;
    uint32_t sq_cnt = 0, pq_cnt = 0;       // wave-uniform: special entries [0, sq_cnt), plain entries [kXq - pq_cnt, kXq)
    bool overflow = false;                 // wave-uniform: the stacks met (cannot happen, see above; reported instead of corrupting paths)
    uint32_t wave_shadow = 0, wave_vertices = 0;
    uint32_t wave_taken = 0;               // wave-uniform: paths taken from the ring; every one of them ends in this wave (no hand-over)
    uint32_t dmax = 0;
    PathState p = parked_state();
    bool alive = false;

    for (;;) {
        // ---- keep at least one chunk of camera rays in the ring (as k_paths_regen)
        while (!exhausted && pool_cnt < 64u) {
            uint32_t chunk;
            if (st_next < a.regen_static) {
                chunk = st_next; st_next += nw;
            } else {
                for (;;) {
                    uint32_t got = 0;
                    if (lane == 0u) got = atomicAdd(a.chunk_counter + ctr * kRegenCounterStride, 1u);
                    chunk = a.regen_static + __builtin_amdgcn_readfirstlane(got) * kRegenCounters + ctr;
                    if (chunk < n_chunks) break;
                    ctr = ctr + 1u == kRegenCounters ? 0u : ctr + 1u;
                    if (++ctr_dry == kRegenCounters) { exhausted = true; break; }
                }
                if (exhausted) break;
            }
            const uint32_t pid = chunk * 64u + lane;
            const uint32_t valid = n_first - chunk * 64u < 64u ? n_first - chunk * 64u : 64u;
            if (lane < valid) {
                uint32_t s_local, pix, yl, px;
                divmod_magic(pid, a.np, a.np_magic, s_local, pix);
                divmod_magic(pix, W, a.film_w_magic, yl, px);
                f3 o, d;
                camera_ray(a.cam, a.s_base + s_local, px, image_row(a.tile, yl), o, d);
                const uint32_t e = (pool_head + pool_cnt + lane) & (kPool - 1u);
                pool_d[e] = make_float4(d.x, d.y, d.z, __uint_as_float((yl << 16) | px));
                pool_s[e] = s_local << 16;
            }
            pool_cnt += valid;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- lanes without a path: first the ring, then the plain stack (paths that left a Mirror surface).  What waits on the plain
        // stack has its next vertex scanned already and takes the place of the lanes that find a Mirror vertex below; the lanes here
        // take it only when the ring cannot serve them: the end of the batch
        {
            const unsigned long long need = __ballot(!alive);
            const uint32_t r = lane_rank(need);
            const uint32_t n_need = (uint32_t)__popcll(need);
            const uint32_t n_ring = n_need < pool_cnt ? n_need : pool_cnt;
            const uint32_t n_pq = n_need - n_ring < pq_cnt ? n_need - n_ring : pq_cnt;
            const bool from_pq = !alive && r >= n_ring && r - n_ring < n_pq;
            const bool from_ring = !alive && r < n_ring;
            const uint32_t e_pq = kXq - pq_cnt + (r - n_ring), e_ring = (pool_head + r) & (kPool - 1u);
            if (from_pq) {
                const float4* src = x.entry(e_pq);
                p = unpack_state(src[0], src[1], src[2], src[3]);
                // all four loads back HERE: otherwise the compiler waits (vmcnt(0)) at the first use of beta / L in the
                // iteration below, on every path -- and on gfx9 that counter also holds the previous iteration's
                // sample stores, a full HBM write latency per iteration (measured on C2, which never takes this
                // branch: 7.5 instead of 6.2 ms)
                __builtin_amdgcn_s_waitcnt(kWaitVm0);
                alive = true;
            } else if (from_ring) {
                const float4 q = pool_d[e_ring];
                const uint32_t sd = pool_s[e_ring];
                p.o = cam_o; p.d = mk(q.x, q.y, q.z);
                const uint32_t xy = __float_as_uint(q.w);
                p.yl = xy >> 16; p.px = xy & 0xFFFFu;
                p.s_local = sd >> 16; p.depth = 0u;
                p.beta = mk(1.f, 1.f, 1.f); p.L = mk(0.f, 0.f, 0.f);
                p.pdf_prev = 0.0f; p.eta_in = 1.0f;
                alive = true;
            }
            pq_cnt -= n_pq;
            pool_head += n_ring; pool_cnt -= n_ring;
            wave_taken += n_ring;
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t n_alive = (uint32_t)__popcll(__ballot(alive));
        // no plain path although stack and ring were offered: the batch is used up.  Without waiting specials the wave is done.
        if (n_alive == 0u && sq_cnt == 0u) break;

        if (n_alive != 0u) {
            // ---- plain iteration: scan #1 (rendering.rs:41)
            int id; float t;
            scan_closest<kModeLds, false, kSplitPairPrefetch>(sc, p.o, p.d, a.t_min, kInf, id, t);
            // a Mirror vertex is not shaded here: the path waits on the special stack for a batch of its kind
            const bool special = alive && id >= 0 && is_mirror_obj(sc, id);
            const unsigned long long spm = __ballot(special);
            if (spm != 0ull) {
                // Round 5: a lane that hands its path to the special stack takes, in the same breath, a path from the plain stack --
                // one that left the glass in an earlier batch, whose next vertex that batch has scanned already: (id, t) travel with
                // the entry.  The lane goes on with vertex_begin at once instead of idling through the rest of the iteration, and the
                // path is not scanned a second time.  The pops are complete before the pushes are issued (with both stacks nearly
                // full the pushed entries may be the popped ones); lanes + stacks stay <= 127 paths: a push without a pop happens
                // only with the plain stack empty, i.e. at <= 63 + 64 entries.
                const uint32_t rk = lane_rank(spm);
                const uint32_t n_sp = (uint32_t)__popcll(spm);
                const uint32_t n_rep = n_sp < pq_cnt ? n_sp : pq_cnt;
                const bool rep = special && rk < n_rep;
                PathState q = p;
                int qid = -1; float qt = 0.0f;
                if (rep) {
                    const float4* src = x.entry(kXq - pq_cnt + rk);
                    q = unpack_state(src[0], src[1], src[2], src[3]);
                    const float2 it = *reinterpret_cast<const float2*>(src + 4);
                    qid = __float_as_int(it.x); qt = it.y;
                    __builtin_amdgcn_s_waitcnt(kWaitVm0);
                }
                if (special) {
                    float4* dst = x.entry(sq_cnt + rk);
                    store_entry(dst, p);
                    *reinterpret_cast<float2*>(dst + 4) = make_float2(__int_as_float(id), t);     // (8 of the slot's 16 bytes: no padding words to keep in registers)
                    if (rep) {
                        p = q; id = qid; t = qt;
                    } else {
                        alive = false;
                        p.o = parked_origin(); p.d = parked_dir();
                        id = -1;
                    }
                }
                sq_cnt += n_sp;
                pq_cnt -= n_rep;
                overflow = overflow || sq_cnt + pq_cnt > kXq;
            }
            const bool active = alive;
            const uint32_t kx = p.px, py = image_row(a.tile, p.yl);
            const uint32_t sample = a.s_base + p.s_local;
            wave_vertices += (uint32_t)__popcll(__ballot(active));
            Vertex v;
            vertex_begin<MIS, PLAIN>(sc, p, active, id, t, sample, kx, py, v);
            bool visible = false;
            if (MIS) {
                const unsigned long long sm = __ballot(v.need_shadow);
                if (sm != 0ull) {
                    f3 sdir = v.need_shadow ? v.light_dir : parked_dir();
                    f3 sorg = v.need_shadow ? v.hit.point : parked_origin();
                    int sid; float st;
                    scan_closest<kModeLds, true, kSplitPairPrefetch>(sc, sorg, sdir, a.t_min, v.distance - a.t_min, sid, st);
                    visible = v.need_shadow && sid < 0;
                    wave_shadow += (uint32_t)__popcll(sm);
                }
            }
            alive = vertex_end<MIS, PLAIN, true>(sc, p, v, visible, sample, kx, py, a.min_depth, a.max_depth);
            if (active && !alive) {
                a.lsamp[p.s_local * a.np + p.yl * W + p.px] = Rgb{p.L.x, p.L.y, p.L.z};
                dmax = p.depth > dmax ? p.depth : dmax;
                p.o = parked_origin(); p.d = parked_dir();
            }
        }

        // ---- batches of Mirror vertices: whenever a full wave of them waits, or nothing else is left to do
        auto plain_work = [&]() { return __ballot(alive) != 0ull || pool_cnt != 0u || !exhausted || pq_cnt != 0u; };
        if (sq_cnt >= 64u || (sq_cnt != 0u && !plain_work())) {
            // park the plain paths in LDS for the batch (round 4): their 16 registers carry the batch's paths instead -- the
            // popped entry WHOLE (one wait per batch iteration instead of one for the ray part and one for the carry part), and
            // the survivors across the scan of their next vertex
            park[0][lane] = make_float4(p.o.x, p.o.y, p.o.z, p.d.x);
            park[1][lane] = make_float4(p.d.y, p.d.z, __uint_as_float((p.yl << 16) | p.px), __uint_as_float((p.s_local << 16) | p.depth));
            park[2][lane] = make_float4(p.beta.x, p.beta.y, p.beta.z, p.pdf_prev);
            park[3][lane] = make_float4(p.L.x, p.L.y, p.L.z, p.eta_in);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");     // entries pushed above are read by other lanes below
            do {
                const uint32_t n = sq_cnt < 64u ? sq_cnt : 64u;
                const bool qa = lane < n;
                const uint32_t e = sq_cnt - n + (qa ? lane : 0u);     // the top n entries
                PathState q = parked_state();
                int qid = -1; float qt = 0.0f;
                if (qa) {
                    const float4* src = x.entry(e);
                    q = unpack_state(src[0], src[1], src[2], src[3]);
                    const float2 it = *reinterpret_cast<const float2*>(src + 4);
                    qid = __float_as_int(it.x); qt = it.y;
                }
                sq_cnt -= n;
                const uint32_t kx = q.px, py = image_row(a.tile, q.yl);
                const uint32_t sample = a.s_base + q.s_local;
                wave_vertices += n;
                Vertex v;
                vertex_begin<MIS, kMatsAll>(sc, q, qa, qid, qt, sample, kx, py, v);
                bool visible = false;
                if (MIS) {
                    const unsigned long long sm = __ballot(v.need_shadow);
                    if (sm != 0ull) {
                        f3 sdir = v.need_shadow ? v.light_dir : parked_dir();
                        f3 sorg = v.need_shadow ? v.hit.point : parked_origin();
                        int sid; float st;
                        scan_closest<kModeLds, true, kSplitPairPrefetch>(sc, sorg, sdir, a.t_min, v.distance - a.t_min, sid, st);
                        visible = v.need_shadow && sid < 0;
                        wave_shadow += (uint32_t)__popcll(sm);
                    }
                }
                const bool qalive = vertex_end<MIS, kMatsAll, true>(sc, q, v, visible, sample, kx, py, a.min_depth, a.max_depth);
                if (qa && !qalive) {
                    a.lsamp[q.s_local * a.np + q.yl * W + q.px] = Rgb{q.L.x, q.L.y, q.L.z};
                    dmax = q.depth > dmax ? q.depth : dmax;
                }
                // the survivors' next vertex: Mirror again (a path inside the sphere) or not?
                const f3 so = qalive ? q.o : parked_origin(), sd = qalive ? q.d : parked_dir();
                asm volatile("" ::: "memory");
                int id2; float t2;
                scan_closest<kModeLds, false, kSplitPairPrefetch>(sc, so, sd, a.t_min, kInf, id2, t2);
                const bool spec2 = qalive && id2 >= 0 && is_mirror_obj(sc, id2);
                const bool plain2 = qalive && !spec2;
                const unsigned long long m_s = __ballot(spec2), m_p = __ballot(plain2);
                const uint32_t n_p = (uint32_t)__popcll(m_p);
                if (qalive) {
                    const uint32_t dst = spec2 ? sq_cnt + lane_rank(m_s) : kXq - pq_cnt - n_p + lane_rank(m_p);
                    float4* de = x.entry(dst);
                    store_entry(de, q);
                    *reinterpret_cast<float2*>(de + 4) = make_float2(__int_as_float(id2), t2);
                }
                sq_cnt += (uint32_t)__popcll(m_s);
                pq_cnt += n_p;
                overflow = overflow || sq_cnt + pq_cnt > kXq;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            } while (sq_cnt >= 64u || (sq_cnt != 0u && !plain_work()));
            p = unpack_state(park[0][lane], park[1][lane], park[2][lane], park[3][lane]);
        }
    }

    const uint32_t wave_samples = wave_taken;
    for (int off = 32; off > 0; off >>= 1) { const uint32_t w2 = (uint32_t)__shfl_xor((int)dmax, off); dmax = w2 > dmax ? w2 : dmax; }
    if (lane == 0u) {
        wave_totals<MIS>(s_totals, kBlock / 64, a.stats, wave_shadow, wave_vertices, wave_samples, dmax);
        if (overflow) atomicMax(&a.stats[7], 1ull);      // pt_sync turns it into an error
    }
}

// ------------------------------------------------------------------ the path kernel, BVH form
// Same organisation as k_paths (one launch per batch, wave-private queue segments compacted in place, tail
// hand-off), but a BVH traversal diverges: rays of one wave need between a handful and a few hundred steps,
// and a wave that traces 64 rays side by side idles most lanes most of the time (measured on C4: 17 % of the
// VALU lane-cycles did work).  So every pass over a segment is cut into stages, and the two traversal stages
// hand a NEW ray to a lane as soon as its ray is done (traverse_segment):
//     stage 1  extend   closest hit of every path ray of the segment          -> aux[slot].xy = (id, t)
//     stage 2  connect  hit record + light sample of every path (vertex_begin) -> shadow ray of the slot
//     stage 3  occlude  any-hit traversal of the shadow rays                   -> aux[slot].z
//     stage 4  shade    vertex_begin again (cheaper than storing it) + vertex_end, in-place compaction
// Pass 0 first writes the camera rays (or the overflow queue's paths) into the segment.

// Rays of a segment: plane0[slot] = (o, d.x), plane1[slot] = (d.y, d.z, t_max, has_ray) when TMAX_IN_RAY (a slot
// with has_ray == 0 is skipped; t_max itself may be anything, also negative or NaN -- the scan's semantics
// decide), else plane1[slot] = (d.y, d.z, -, -) and t_max = inf.  ANY: out[slot].z = 1 if anything is hit, else 0 (visibility).  Otherwise
// out[slot].xy = (id, t) of the closest hit.  Semantics of one ray: bvh_scan.
template <bool TMAX_IN_RAY, bool ANY>
PT_DEV void traverse_segment(const SceneRef& sc, const float4* __restrict__ plane0, const float4* __restrict__ plane1,
                             float4* __restrict__ out, uint32_t n, float t_min, uint32_t refill_below, uint32_t leaf_batch) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t* stk = sc.stack + threadIdx.x;
    uint32_t next = 0;                         // wave-uniform: first slot not handed out yet
    bool has = false;                          // this lane is tracing a ray
    uint32_t slot = 0, node = 0xFFFFFFFFu, sp = 1;
    // slab planes as one FMA each: t = plane * inv + b with bp = -(o + pad) * inv for the lower plane of a box and
    // bm = -(o - pad) * inv for the upper one (the rounding of b moves a plane by <= ulp(|o|), far inside pad)
    // ... with the plane on the builder's 16-bit grid, plane = grid_min + q * cell: t = q * (cell * inv) + b, b now from
    // (grid_min - (o +- pad)) * inv.  The folded form rounds differently from "decode, then slab", by ~1e-7 of the
    // scene extent: far inside pad as well.
    f3 o = parked_origin(), d = parked_dir(), inv = mk(0.f, 0.f, 0.f), bp = inv, bm = inv;
    const f3 gmin = mk(sc.bvh.grid_min[0], sc.bvh.grid_min[1], sc.bvh.grid_min[2]);
    const f3 gcell = mk(sc.bvh.grid_cell[0], sc.bvh.grid_cell[1], sc.bvh.grid_cell[2]);
    float closest = 0.0f;
    int id = -1;
    uint32_t pend = 0xFFFFFFFFu;                // a leaf this lane has put aside (none: the sentinel)
    for (;;) {
        // ---- hand the next slots to the idle lanes, in lane order
        const unsigned long long idle = __ballot(!has);
        if (next < n && idle != 0ull) {
            uint32_t cand = next + (uint32_t)__popcll(idle & lt);
            if (!has && cand < n) {
                const float4 r0 = plane0[cand], r1 = plane1[cand];
                const float t_max = TMAX_IN_RAY ? r1.z : kInf;
                if (!TMAX_IN_RAY || r1.w != 0.0f) {
                    slot = cand;
                    o = mk(r0.x, r0.y, r0.z); d = mk(r0.w, r1.x, r1.y);
                    const float a = dot(d, d), inv_a = __builtin_amdgcn_rcpf(a);      // only to recognise zero / NaN rays
                    closest = t_max;
                    id = -1;
                    const float o1 = __builtin_fabsf(o.x) + __builtin_fabsf(o.y) + __builtin_fabsf(o.z);
                    const bool regular = o1 + __builtin_fabsf(d.x) + __builtin_fabsf(d.y) + __builtin_fabsf(d.z) + a + inv_a < kInf;
                    if (regular) {
                        const float pad = kBvhPad * (o1 + sc.bvh.scene_abs);
                        // 1/d clamped to +-1e25: a zero (or denormal) component then acts like +-infinity without the
                        // inf - inf = NaN an FMA would make of it (one NaN plane and min/max collapse the slab interval)
                        inv = mk(__builtin_fminf(__builtin_fmaxf(__builtin_amdgcn_rcpf(d.x), -1e25f), 1e25f),
                                 __builtin_fminf(__builtin_fmaxf(__builtin_amdgcn_rcpf(d.y), -1e25f), 1e25f),
                                 __builtin_fminf(__builtin_fmaxf(__builtin_amdgcn_rcpf(d.z), -1e25f), 1e25f));
                        bp = mk((gmin.x - (o.x + pad)) * inv.x, (gmin.y - (o.y + pad)) * inv.y, (gmin.z - (o.z + pad)) * inv.z);
                        bm = mk((gmin.x - (o.x - pad)) * inv.x, (gmin.y - (o.y - pad)) * inv.y, (gmin.z - (o.z - pad)) * inv.z);
                        inv = inv * gcell;                                    // from here on: per grid step
                        stk[0] = 0xFFFFFFFFu;
                        sp = 1;
                        node = sc.bvh.root;
                    } else {
                        scan_global(sc, o, d, t_min, t_max, id, closest);      // the linear scan's NaN behaviour (rare)
                        node = 0xFFFFFFFFu;
                    }
                    has = true;
                }
            }
            const uint32_t given = (uint32_t)__popcll(idle);
            next = n - next < given ? n : next + given;
        }
        if (__ballot(has) == 0ull) {
            if (next >= n) break;
            continue;
        }
        const uint32_t low_water = next < n ? refill_below : 1u;
        do {
            if (has && (int)node >= 0) {                 // internal node: one 64-byte visit tests its (up to) four child boxes
                const uint4* nd = sc.bvh.nodes + 4u * node;
                const uint4 qa = nd[0], qb = nd[1], qc = nd[2], qd = nd[3];
                // child c = three words (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16); entry distance of the
                // padded box inside [t_min, closest], or "no hit"
                auto slab = [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t code, float& tn) -> bool {
                    const float ax0 = __builtin_fmaf((float)(w0 & 0xFFFFu), inv.x, bp.x), ax1 = __builtin_fmaf((float)(w1 >> 16), inv.x, bm.x);
                    const float ay0 = __builtin_fmaf((float)(w0 >> 16), inv.y, bp.y), ay1 = __builtin_fmaf((float)(w2 & 0xFFFFu), inv.y, bm.y);
                    const float az0 = __builtin_fmaf((float)(w1 & 0xFFFFu), inv.z, bp.z), az1 = __builtin_fmaf((float)(w2 >> 16), inv.z, bm.z);
                    tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax0, ax1), __builtin_fminf(ay0, ay1)),
                                         __builtin_fmaxf(__builtin_fminf(az0, az1), t_min));
                    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax0, ax1), __builtin_fmaxf(ay0, ay1)),
                                                     __builtin_fminf(__builtin_fmaxf(az0, az1), closest));
                    return tn <= tf && code != 0xFFFFFFFFu;          // unused child slots carry the sentinel code
                };
                float t0, t1, t2, t3;
                const bool h0 = slab(qa.x, qa.y, qa.z, qd.x, t0), h1 = slab(qa.w, qb.x, qb.y, qd.y, t1);
                const bool h2 = slab(qb.z, qb.w, qc.x, qd.z, t2), h3 = slab(qc.y, qc.z, qc.w, qd.w, t3);
                // Nearest child first, the others onto the stack far to near: a five-comparator network on (key, code) pairs,
                // key = bits of the entry distance (t_min > 0: positive floats order like integers; with an unusual t_min <= 0
                // the order is merely not by distance), misses sort last.  Branch-free: the three far codes are STORED
                // unconditionally at the running stack top (a store above the top is harmless: the stack has three spare
                // rows for it) and only the top moves conditionally -- as divergent branches this part cost more than the
                // slab tests.
                uint32_t k0 = h0 ? __float_as_uint(t0) : 0xFFFFFFFFu, k1 = h1 ? __float_as_uint(t1) : 0xFFFFFFFFu;
                uint32_t k2 = h2 ? __float_as_uint(t2) : 0xFFFFFFFFu, k3 = h3 ? __float_as_uint(t3) : 0xFFFFFFFFu;
                uint32_t c_near = qd.x, c1 = qd.y, c2 = qd.z, c3 = qd.w;
                auto cx = [](uint32_t& kx, uint32_t& cxv, uint32_t& ky, uint32_t& cyv) {
                    const bool sw = ky < kx;
                    const uint32_t ka = sw ? ky : kx, kb = sw ? kx : ky, ca = sw ? cyv : cxv, cb = sw ? cxv : cyv;
                    kx = ka; ky = kb; cxv = ca; cyv = cb;
                };
                cx(k0, c_near, k1, c1); cx(k2, c2, k3, c3); cx(k0, c_near, k2, c2); cx(k1, c1, k3, c3); cx(k1, c1, k2, c2);   // ascending: k0 nearest
                stk[sp * kBlock] = c3; sp += k3 != 0xFFFFFFFFu ? 1u : 0u;
                stk[sp * kBlock] = c2; sp += k2 != 0xFFFFFFFFu ? 1u : 0u;
                stk[sp * kBlock] = c1; sp += k1 != 0xFFFFFFFFu ? 1u : 0u;
                if (k0 != 0xFFFFFFFFu) {
                    node = c_near;
                } else {
                    --sp;
                    node = stk[sp * kBlock];
                }
            }
            // A lane that reaches a leaf puts it aside (one per lane) and goes on with its stack: it keeps working on inner
            // nodes while the wave collects enough leaves for a dense batch of primitive tests.  (The tests run later than
            // in stack order, so `closest` may shrink later: a few more visits, never another answer.)
            if (has && pend == 0xFFFFFFFFu && (int)node < 0 && node != 0xFFFFFFFFu) {
                pend = node;
                --sp;
                node = stk[sp * kBlock];
            }
            const bool at_leaf = has && pend != 0xFFFFFFFFu;
            const uint32_t leaf = pend;
            const unsigned long long leafs = __ballot(at_leaf);
            if (leafs != 0ull && ((uint32_t)__popcll(leafs) >= leaf_batch || __ballot(has && (int)node >= 0) == 0ull)) {
                if (at_leaf) {
                    const uint32_t first = leaf & 0x0FFFFFFFu, cnt = ((leaf >> 28) & 7u) + 1u;
                    // all ids (one aligned 16-byte load) and lead records (one 64-byte line) requested before the
                    // first test: one memory latency per leaf
                    const uint4 idv = *reinterpret_cast<const uint4*>(sc.bvh.ids + first);
                    const uint32_t w[kBvhMaxLeaf] = {idv.x, idv.y, idv.z, idv.w};
                    float4 r0[kBvhMaxLeaf];
#pragma unroll
                    for (uint32_t i = 0; i < kBvhMaxLeaf; ++i) r0[i] = sc.bvh.lead[first + (i < cnt ? i : 0u)];
#pragma unroll
                    for (uint32_t i = 0; i < kBvhMaxLeaf; ++i) {
                        if (i < cnt) {
                            if ((int)w[i] >= 0) {
                                sphere_test<true>(r0[i], o, d, t_min, closest, id, (int)w[i]);
                            } else {
                                const float4* rec = sc.bvh.rec + 3u * (first + i);
                                const float4 r1 = rec[1], r2 = rec[2];
                                triangle_test<true>(r0[i], r1, r2, o, d, t_min, closest, id, (int)(w[i] & 0x7FFFFFFFu));
                            }
                        }
                    }
                    pend = 0xFFFFFFFFu;
                    if (ANY && id >= 0) node = 0xFFFFFFFFu;
                }
            }
            if (has && node == 0xFFFFFFFFu && pend == 0xFFFFFFFFu) {   // this ray is done
                if (ANY) out[slot].z = id >= 0 ? 1.0f : 0.0f;
                else *reinterpret_cast<float2*>(&out[slot]) = make_float2(__int_as_float(id), closest);
                has = false;
            }
        } while ((uint32_t)__popcll(__ballot(has)) >= low_water);
    }
}

#ifndef PT_BVH_WAVES
#define PT_BVH_WAVES 5      // measured on C4: 4 -> 74.0 ms, 5 -> 70.2 ms, 6 (spills) -> 72.8 ms
#endif
template <bool MIS, bool OVF, bool DIFFUSE, bool LIST>
__global__ void __launch_bounds__(kBlock, PT_BVH_WAVES) k_paths_bvh(BounceArgs a) {
    extern __shared__ float4 lds[];
    __shared__ WgTotals s_totals;
    if (threadIdx.x == 0u) wg_totals_init(s_totals);
    __syncthreads();                                             // (the traversal form has no barrier of its own before a wave can end)
    const SceneRef sc = stage_scene<kModeBvh>(a.sc, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t nw = gridDim.x * (kBlock / 64);
    uint32_t n_first, seg_cap;
    launch_shape<OVF>(a, nw, n_first, seg_cap);
    const uint32_t seg_base = wave * seg_cap;
    const uint32_t n_chunks = (n_first + 63u) >> 6;
    const uint32_t W = a.film_w;
    const Queue q = {{a.q.q[0] + seg_base, a.q.q[1] + seg_base, a.q.q[2] + seg_base, a.q.q[3] + seg_base}};
    float4* const aux = a.aux + seg_base;
    float4* const sr0 = a.sray0 + seg_base;
    float4* const sr1 = a.sray1 + seg_base;
    uint32_t wave_shadow = 0, wave_vertices = 0, wave_depth = 0, wave_samples = 0;

    // ---- the wave's share of the batch -> its segment (chunk k of the batch belongs to wave k % nw)
    uint32_t n_in = 0;
    for (uint32_t it = 0, n_iter = (n_chunks + nw - 1u) / nw; it < n_iter; ++it) {
        const uint32_t chunk = it * nw + wave;
        const uint32_t pid = chunk * 64u + lane;
        const bool active = chunk < n_chunks && pid < n_first;
        if (active) {
            PathState p = parked_state();
            if (OVF) {
                p = unpack_state(a.ovf_in.q[0][pid], a.ovf_in.q[1][pid], a.ovf_in.q[2][pid], a.ovf_in.q[3][pid]);
            } else {
                uint32_t pix;
                divmod_magic(pid, a.np, a.np_magic, p.s_local, pix);
                divmod_magic(pix, W, a.film_w_magic, p.yl, p.px);
                uint32_t kx, py;
                pixel_key<LIST>(a, p, active, kx, py);
                camera_ray(a.cam, a.s_base + p.s_local, kx, py, p.o, p.d);
            }
            store_state(q, it * 64u + lane, p);     // dense: only the last chunk of the batch can be partial
        }
        n_in += (uint32_t)__popcll(__ballot(active));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");

    for (uint32_t pass = 0; n_in != 0u; ++pass) {
        const uint32_t n_iter = (n_in + 63u) >> 6;
        // ---- stage 1: closest hits (rendering.rs:41)
        traverse_segment<false, false>(sc, q.q[0], q.q[1], aux, n_in, a.t_min, a.bvh_refill, a.bvh_leaf);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (MIS) {
            // ---- stage 2: light samples -> shadow rays (world.rs:251-267, rendering.rs:58-62)
            for (uint32_t it = 0; it < n_iter; ++it) {
                const uint32_t s = it * 64u + lane;
                const bool active = s < n_in;
                PathState p = parked_state();
                float4 h = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
                if (active) { unpack_ray(p, q.q[0][s], q.q[1][s]); h = aux[s]; }
                Vertex v;
                uint32_t kx, py;
                pixel_key<LIST>(a, p, active, kx, py);
                vertex_begin<true, DIFFUSE>(sc, p, active, __float_as_int(h.x), h.y, a.s_base + p.s_local, kx, py, v);
                if (active) {
                    sr0[s] = make_float4(v.hit.point.x, v.hit.point.y, v.hit.point.z, v.light_dir.x);
                    sr1[s] = make_float4(v.light_dir.y, v.light_dir.z, v.distance - a.t_min, v.need_shadow ? 1.0f : 0.0f);
                }
                wave_shadow += (uint32_t)__popcll(__ballot(v.need_shadow));
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            // ---- stage 3: visibility (rendering.rs:62-65)
            traverse_segment<true, true>(sc, sr0, sr1, aux, n_in, a.t_min, a.bvh_refill, a.bvh_leaf);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
        // ---- stage 4: shade and compact in place
        uint32_t out_n = 0;
        for (uint32_t it = 0; it < n_iter; ++it) {
            const uint32_t s = it * 64u + lane;
            const bool active = s < n_in;
            PathState p = parked_state();
            float4 h = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
            if (active) { p = unpack_state(q.q[0][s], q.q[1][s], q.q[2][s], q.q[3][s]); h = aux[s]; }
            uint32_t kx, py;
            pixel_key<LIST>(a, p, active, kx, py);
            const uint32_t sample = a.s_base + p.s_local;
            wave_vertices += (uint32_t)__popcll(__ballot(active));
            if (!OVF) {
                wave_depth = pass;
            } else if (__ballot(active && p.depth > wave_depth) != 0ull) {
                uint32_t m = active ? p.depth : 0u;
                for (int off = 32; off > 0; off >>= 1) { const uint32_t w2 = (uint32_t)__shfl_xor((int)m, off); m = w2 > m ? w2 : m; }
                wave_depth = __builtin_amdgcn_readfirstlane(m);
            }
            Vertex v;
            vertex_begin<MIS, DIFFUSE>(sc, p, active, __float_as_int(h.x), h.y, sample, kx, py, v);
            const bool visible = MIS && v.need_shadow && h.z == 0.0f;
            const bool alive = vertex_end<MIS, DIFFUSE, false>(sc, p, v, visible, sample, kx, py, a.min_depth, a.max_depth);
            if (active && !alive) a.lsamp[p.s_local * a.np + p.yl * W + p.px] = Rgb{p.L.x, p.L.y, p.L.z};
            wave_samples += (uint32_t)__popcll(__ballot(active && !alive));
            const unsigned long long mask = __ballot(alive);
            if (alive) store_state(q, out_n + lane_rank(mask), p);
            out_n += (uint32_t)__popcll(mask);
        }
        n_in = out_n;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (n_in < a.export_below) break;
    }

    if (n_in != 0u) {                          // tail hand-off, as in k_paths
        uint32_t base = 0;
        if (lane == 0u) base = atomicAdd(a.ovf_out_count, n_in);
        base = __shfl(base, 0);
        for (uint32_t j = lane; j < n_in; j += 64u) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k) { const float4 t = a.q.q[k][seg_base + j]; a.ovf_out.q[k][base + j] = t; }
        }
    }
    if (lane == 0u) wave_totals<MIS, !OVF>(s_totals, kBlock / 64, a.stats, wave_shadow, wave_vertices, wave_samples, wave_depth);
}

[[maybe_unused]] static int scene_mode(const SceneView& sc, uint32_t accel) {
    return accel ? kModeBvh : (sc.n_objs <= kSmallObjs ? kModeLds : kModeTiled);
}
[[maybe_unused]] static size_t scene_lds_bytes(const SceneView& sc, int mode) {
    if (mode == kModeBvh) return (size_t)(kBvhStack + 3u) * kBlock * sizeof(uint32_t);   // + 3 rows: the traversal stores a visit's (up to) three far children before it knows how many there are
    return (mode == kModeLds ? (sc.blob_f4 ? sc.blob_f4 : 1u) : kTileF4) * sizeof(float4);
}
// the launchers return the instance code (pt_kernels.h) of the kernel they enqueue
constexpr bool kExactMath = PT_MATH_EXACT != 0;
template <int MODE, bool DIFFUSE, bool LIST>
[[maybe_unused]] static uint32_t launch_paths_mode(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st) {
    const bool mis = a.integrator == 0;
    const bool ovf = a.src_mode != 0u;     // continuation launch
    const dim3 g(grid), b(kBlock);
    if (mis && !ovf) hipLaunchKernelGGL((k_paths<MODE, true, false, DIFFUSE, LIST>), g, b, lds, st, a);
    else if (mis) hipLaunchKernelGGL((k_paths<MODE, true, true, DIFFUSE, LIST>), g, b, lds, st, a);
    else if (!ovf) hipLaunchKernelGGL((k_paths<MODE, false, false, DIFFUSE, LIST>), g, b, lds, st, a);
    else hipLaunchKernelGGL((k_paths<MODE, false, true, DIFFUSE, LIST>), g, b, lds, st, a);
    return instance_code(kInstPaths, MODE, mis, ovf, DIFFUSE, LIST, kExactMath);
}
#if PT_TU_BVH
template <bool DIFFUSE, bool LIST>
static uint32_t launch_paths_bvh_t(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st) {
    const bool mis = a.integrator == 0;
    const bool ovf = a.src_mode != 0u;
    const dim3 g(grid), b(kBlock);
    if (mis && !ovf) hipLaunchKernelGGL((k_paths_bvh<true, false, DIFFUSE, LIST>), g, b, lds, st, a);
    else if (mis) hipLaunchKernelGGL((k_paths_bvh<true, true, DIFFUSE, LIST>), g, b, lds, st, a);
    else if (!ovf) hipLaunchKernelGGL((k_paths_bvh<false, false, DIFFUSE, LIST>), g, b, lds, st, a);
    else hipLaunchKernelGGL((k_paths_bvh<false, true, DIFFUSE, LIST>), g, b, lds, st, a);
    return instance_code(kInstBvh, 0, mis, ovf, DIFFUSE, LIST, kExactMath);
}
#endif

}  // namespace PTK_IMPL
namespace ptk {
using namespace PTK_IMPL;
#if PT_TU_BVH
uint32_t PT_LAUNCH(launch_paths_bvh)(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st, bool diffuse, bool list) {
    if (list) return launch_paths_bvh_t<false, true>(a, grid, lds, st);        // pixel lists: the generic kernels only
    if (diffuse) return launch_paths_bvh_t<true, false>(a, grid, lds, st);
    return launch_paths_bvh_t<false, false>(a, grid, lds, st);
}
#endif
#if PT_TU_SPLIT
// k_paths_regen_split for the scene's material set (the plain iterations': no OrenNayar either / no Mirror)
typedef void (*RegenSplitKernel)(BounceArgs);
static RegenSplitKernel regen_split_kernel(const BounceArgs& a, uint32_t* code = nullptr) {
    const bool mis = a.integrator == 0;
    const int plain = a.sc.no_oren_nayar ? kMatsDiffuse : kMatsNoMirror;
    if (code) *code = instance_code(kInstRegenSplit, 0, mis, false, plain, false, kExactMath);
    if (a.sc.no_oren_nayar) return mis ? k_paths_regen_split<true, kMatsDiffuse> : k_paths_regen_split<false, kMatsDiffuse>;
    return mis ? k_paths_regen_split<true, kMatsNoMirror> : k_paths_regen_split<false, kMatsNoMirror>;
}
int PT_LAUNCH(regen_split_blocks_per_cu)(const BounceArgs& a, size_t lds) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, regen_split_kernel(a), (int)kBlock, lds) != hipSuccess) return -1;
    return n;
}
uint32_t PT_LAUNCH(launch_regen_split)(const BounceArgs& b, uint32_t blocks, size_t lds, hipStream_t st) {
    uint32_t code = 0;
    hipLaunchKernelGGL(regen_split_kernel(b, &code), dim3(blocks), dim3(kBlock), lds, st, b);
    return code;
}
#endif
#if PT_TU_MAIN
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
#endif
}  // namespace ptk
#if PT_TU_MAIN
namespace PTK_IMPL {

// ------------------------------------------------------------------ film resolve
// World::render_pixel's tail (world.rs:311-332).  One thread per tile pixel; the
// nb samples of the batch are added in sample order into an f64 sum, so the film
// does not depend on how paths were scheduled.
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
#if !PT_MATH_EXACT
namespace PTK_IMPL {
// ------------------------------------------------------------------ multi-GPU film exchange (pt_multi.cpp)
// A device's tile -> one 16-byte record per pixel (12 B linear RGB + 4 B RGBA8), so that both film planes travel in
// ONE gather; rows beyond the tile (tiles are padded to the largest one) are left untouched.
__global__ void __launch_bounds__(kBlock) k_film_pack(const float* __restrict__ lin, const uint8_t* __restrict__ rgba,
                                                      uint32_t np, uint4* __restrict__ packed) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= np) return;
    uint4 v;
    v.x = __float_as_uint(lin[3 * (size_t)p]); v.y = __float_as_uint(lin[3 * (size_t)p + 1]); v.z = __float_as_uint(lin[3 * (size_t)p + 2]);
    v.w = rgba ? *reinterpret_cast<const uint32_t*>(rgba + 4 * (size_t)p) : 0u;
    packed[p] = v;
}
// The gathered tiles (device g's padded tile at recv + g * max_rows * W) -> the frame in image order.  Image row y lies
// in band y / band_rows, which device (band % n_dev) rendered as its tile row (band / n_dev) * band_rows + y % band_rows.
__global__ void __launch_bounds__(kBlock) k_film_unpack(const uint4* __restrict__ recv, uint32_t W, uint32_t H, uint32_t band_rows,
                                                        uint32_t n_dev, uint32_t max_rows, float* __restrict__ lin,
                                                        uint8_t* __restrict__ rgba) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= W * H) return;
    const uint32_t y = p / W, x = p - y * W;
    const uint32_t band = y / band_rows, g = band % n_dev;
    const uint32_t k = (band / n_dev) * band_rows + (y - band * band_rows);
    const uint4 v = recv[((size_t)g * max_rows + k) * W + x];
    lin[3 * (size_t)p] = __uint_as_float(v.x); lin[3 * (size_t)p + 1] = __uint_as_float(v.y); lin[3 * (size_t)p + 2] = __uint_as_float(v.z);
    if (rgba) *reinterpret_cast<uint32_t*>(rgba + 4 * (size_t)p) = v.w;
}

// ------------------------------------------------------------------ adaptive sampling (pt_render_adaptive, rule: pt_adaptive.h)
// k_resolve for one sample batch of an adaptive pass: list slot i -> image pixel pix, whose f64 sums (R, G, B and the
// luminance sums S1, S2) take the batch's samples in sample order.  A pixel's sums are thus exactly the ones k_resolve forms
// for it in a uniform render of as many samples, and its mean, gamma and RGBA8 are the same expressions (world.rs:311-332).
__global__ void __launch_bounds__(kBlock) k_resolve_adaptive(AdaptiveResolveArgs a) {
    if (blockIdx.x == 0u && a.zero_words)
        for (uint32_t k = threadIdx.x; k < a.n_zero; k += kBlock) a.zero_words[k] = 0u;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    uint32_t pix = i;
    if (a.pixels) { const uint2 xy = a.pixels[i]; pix = xy.y * a.width + xy.x; }
    double* const sp = a.f.sums + 5 * (size_t)pix;
    double r = 0.0, g = 0.0, b = 0.0, s1 = 0.0, s2 = 0.0;
    if (a.load) { r = sp[0]; g = sp[1]; b = sp[2]; s1 = sp[3]; s2 = sp[4]; }
    auto add = [&](const Rgb& v) {
        r += (double)v.r; g += (double)v.g; b += (double)v.b;                     // world.rs:311
        const double L = ptad::luminance(v.r, v.g, v.b);
        s1 += L; s2 += L * L;
    };
    uint32_t s = 0;
    for (; s + 4u <= a.nb; s += 4u) {              // four samples' loads in flight before the ordered additions (as k_resolve)
        Rgb v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = a.lsamp[(size_t)(s + k) * a.n + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) add(v[k]);
    }
    for (; s < a.nb; ++s) add(a.lsamp[(size_t)s * a.n + i]);
    sp[0] = r; sp[1] = g; sp[2] = b; sp[3] = s1; sp[4] = s2;
    if (!a.finalize) return;
    const double dn = (double)a.n_total;
    const double c[3] = {r / dn, g / dn, b / dn};                                 // world.rs:315
    uint32_t q8 = 0xFF000000u;                                                    // alpha 255, world.rs:331
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double gm = __builtin_sqrt(c[k]);                                   // gamma 2.0, world.rs:322-324
        const double cl = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);                 // clamp keeps NaN
        const double q = cl * 255.0;
        q8 |= (uint32_t)((q != q) ? (uint8_t)0 : (uint8_t)q) << (8 * k);          // `as u8`: truncation, NaN -> 0
        a.f.out_linear[3 * (size_t)pix + k] = (float)c[k];
    }
    *reinterpret_cast<uint32_t*>(a.f.out_rgba + 4 * (size_t)pix) = q8;
    double rel;
    const bool conv = ptad::check(s1, s2, a.n_total, a.f.rel_tol, a.f.abs_floor, &rel);
    a.f.count[pix] = a.n_total;
    a.f.rel_err[pix] = (float)rel;
    a.f.conv[pix] = conv ? 1u : 0u;
}

// The list's pixels that failed their last check, compacted in list order.  Workgroup b owns the kSelectTile slots from
// b * kSelectTile; k_adaptive_count leaves its survivor count in block_counts[b], and k_adaptive_select adds up the counts
// of the workgroups before it (its output offset), then writes its survivors by wave ballot + prefix popcount.
constexpr uint32_t kSelectRounds = kSelectTile / kBlock;
PT_DEV uint2 select_pixel(const uint2* pixels, uint32_t width, uint32_t i) {
    return pixels ? pixels[i] : make_uint2(i % width, i / width);
}
PT_DEV bool select_keep(const uint2* pixels, uint32_t n, uint32_t width, const uint32_t* conv, uint32_t i, uint2& xy) {
    if (i >= n) return false;
    xy = select_pixel(pixels, width, i);
    return conv[xy.y * width + xy.x] == 0u;
}
__global__ void __launch_bounds__(kBlock) k_adaptive_count(const uint2* __restrict__ pixels, uint32_t n, uint32_t width,
                                                           const uint32_t* __restrict__ conv, uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    uint32_t cnt = 0;                              // wave-uniform
    for (uint32_t r = 0; r < kSelectRounds; ++r) {
        uint2 xy;
        const bool keep = select_keep(pixels, n, width, conv, blockIdx.x * kSelectTile + r * kBlock + threadIdx.x, xy);
        cnt += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0u) s_wave[wib] = cnt;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_wave[w];
        block_counts[blockIdx.x] = t;
    }
}
__global__ void __launch_bounds__(kBlock) k_adaptive_select(const uint2* __restrict__ pixels, uint32_t n, uint32_t width,
                                                            const uint32_t* __restrict__ conv, const uint32_t* __restrict__ block_counts,
                                                            uint2* __restrict__ out, uint32_t* __restrict__ out_n) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    // output offset of this workgroup: survivors of the workgroups before it
    uint32_t part = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += kBlock) part += block_counts[k];
    for (int off = 32; off > 0; off >>= 1) part += (uint32_t)__shfl_xor((int)part, off);
    if (lane == 0u) s_wave[wib] = part;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) base += s_wave[w];
    for (uint32_t r = 0; r < kSelectRounds; ++r) {
        __syncthreads();                           // (everybody has read s_wave)
        uint2 xy;
        const bool keep = select_keep(pixels, n, width, conv, blockIdx.x * kSelectTile + r * kBlock + threadIdx.x, xy);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0u) s_wave[wib] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kBlock / 64; ++w) { before += w < wib ? s_wave[w] : 0u; total += s_wave[w]; }
        if (keep) out[base + before + lane_rank(mask)] = xy;
        base += total;
    }
    if (blockIdx.x + 1u == gridDim.x && threadIdx.x == 0u) *out_n = base;
}
}  // namespace PTK_IMPL
namespace ptk {   // the film kernels have no division or sqrt in f32: one copy serves both modes
void launch_resolve(const ResolveArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(PTK_IMPL::k_resolve, dim3((a.np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_resolve_adaptive(const AdaptiveResolveArgs& a, hipStream_t st) {
    if (a.n) hipLaunchKernelGGL(PTK_IMPL::k_resolve_adaptive, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_adaptive_select(const uint2* pixels, uint32_t n, uint32_t width, const uint32_t* conv, uint32_t* block_counts,
                            uint2* out, uint32_t* out_n, hipStream_t st) {
    if (n == 0u) { (void)hipMemsetAsync(out_n, 0, sizeof(uint32_t), st); return; }
    const dim3 g((n + kSelectTile - 1) / kSelectTile), b(kBlock);
    hipLaunchKernelGGL(PTK_IMPL::k_adaptive_count, g, b, 0, st, pixels, n, width, conv, block_counts);
    hipLaunchKernelGGL(PTK_IMPL::k_adaptive_select, g, b, 0, st, pixels, n, width, conv, (const uint32_t*)block_counts, out, out_n);
}
void launch_film_pack(const float* lin, const uint8_t* rgba, uint32_t np, void* packed, hipStream_t st) {
    if (np) hipLaunchKernelGGL(PTK_IMPL::k_film_pack, dim3((np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, lin, rgba, np, (uint4*)packed);
}
void launch_film_unpack(const void* recv, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_dev, uint32_t max_rows, float* lin,
                        uint8_t* rgba, hipStream_t st) {
    if (W * H) hipLaunchKernelGGL(PTK_IMPL::k_film_unpack, dim3((W * H + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint4*)recv, W, H,
                                  band_rows, n_dev, max_rows, lin, rgba);
}
}  // namespace ptk
#endif
#endif      // PT_TU_MAIN
namespace PTK_IMPL {

// ------------------------------------------------------------------ debug: hit_scene on arbitrary rays
// HitRecord of the winning object (shape.rs:84-88 / 194-197 + base.rs:19-33): rec[8] = (t, point3, normal3, front_face)
PT_DEV void store_hit_record(const SceneRef& sc, int id, f3 o, f3 d, float t, float* rec) {
    Hit h;
    h.t = 0.0f; h.point = mk(0.f, 0.f, 0.f); h.normal = mk(0.f, 0.f, 0.f); h.front_face = false;
    if (id >= 0) h = finish_hit(sc.shape, id, load_mat(sc.mat, id).shape_tag, o, d, t);
    rec[0] = h.t; rec[1] = h.point.x; rec[2] = h.point.y; rec[3] = h.point.z;
    rec[4] = h.normal.x; rec[5] = h.normal.y; rec[6] = h.normal.z; rec[7] = h.front_face ? 1.0f : 0.0f;
}
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
#if PT_TU_BVH
// the same through the BVH: every wave packs a contiguous slice of the rays into segment form and runs
// traverse_segment (the routine of k_paths_bvh) over it
__global__ void __launch_bounds__(kBlock) k_debug_hit_bvh(SceneView scv, const float* __restrict__ rays6, uint32_t n,
                                                          float t_min, float t_max, float4* p0, float4* p1, float4* res,
                                                          int32_t* out_id, float* out_t, float* out_rec) {
    extern __shared__ float4 lds[];
    const SceneRef sc = stage_scene<kModeBvh>(scv, lds);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t nw = gridDim.x * (kBlock / 64);
    const uint32_t slice = (n + nw - 1u) / nw;
    const uint32_t base = wave * slice;
    if (base >= n) return;
    const uint32_t cnt = n - base < slice ? n - base : slice;
    for (uint32_t k = lane; k < cnt; k += 64u) {
        const size_t i = base + k;
        const f3 o = mk(rays6[6 * i], rays6[6 * i + 1], rays6[6 * i + 2]);
        const f3 d = normalize(mk(rays6[6 * i + 3], rays6[6 * i + 4], rays6[6 * i + 5]));
        p0[i] = make_float4(o.x, o.y, o.z, d.x);
        p1[i] = make_float4(d.y, d.z, t_max, 1.0f);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    traverse_segment<true, false>(sc, p0 + base, p1 + base, res + base, cnt, t_min, kRefillBelow, kLeafBatch);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    for (uint32_t k = lane; k < cnt; k += 64u) {
        const float4 r = res[base + k];
        const int id = __float_as_int(r.x);
        out_id[base + k] = id;
        out_t[base + k] = id >= 0 ? r.y : 0.0f;
        if (out_rec) {
            const float4 q0 = p0[base + k], q1 = p1[base + k];
            store_hit_record(sc, id, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), r.y, out_rec + 8 * (size_t)(base + k));
        }
    }
}
#endif      // PT_TU_BVH
#if PT_TU_MAIN
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
#endif      // PT_TU_MAIN
}  // namespace PTK_IMPL
namespace ptk {
using namespace PTK_IMPL;
#if PT_TU_BVH
void PT_LAUNCH(launch_debug_hit_bvh)(const SceneView& sc, uint32_t grid, size_t lds, const float* rays6, uint32_t n, float t_min, float t_max,
                                     float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st) {
    // scratch: 3 planes of n float4 (two ray planes + result)
    hipLaunchKernelGGL(k_debug_hit_bvh, dim3(grid), dim3(kBlock), lds, st, sc, rays6, n, t_min, t_max, scratch,
                       scratch + n, scratch + 2 * (size_t)n, out_id, out_t, out_rec);
}
#endif
#if PT_TU_MAIN
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
#endif      // PT_TU_MAIN

}  // namespace ptk

#if PT_TU_MAIN
// ------------------------------------------------------------------ first-hit feature buffers (pt_render_features_device)
// k_feature_rays: the camera rays of samples s_base .. s_base + nb - 1 of every image pixel (camera_ray: the key, jitter draws
// and arithmetic of the path kernels), ray i = s_local * np + p in the rays6 form k_debug_hit reads.  k_feature_resolve maps
// the hits of one batch to records (albedo rgb, emitter | normal xyz, depth) and adds them to the pixel's f32 sums in sample
// order; the sums of earlier batches wait in `out` (load), and the last batch divides by n_samples.
namespace PTK_IMPL {
__global__ void __launch_bounds__(kBlock) k_feature_rays(CameraF cam, uint32_t s_base, uint32_t nb, float* __restrict__ rays6) {
    const uint32_t np = cam.width * cam.height;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nb * np) return;
    const uint32_t s = i / np, p = i - s * np;
    const uint32_t y = p / cam.width, x = p - y * cam.width;
    f3 o, d;
    camera_ray(cam, s_base + s, x, y, o, d);
    float* r = rays6 + 6 * (size_t)i;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}
__global__ void __launch_bounds__(kBlock) k_feature_resolve(FeatureResolveArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.np) return;
    float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
    if (a.load) { f0 = a.out[2 * (size_t)p]; f1 = a.out[2 * (size_t)p + 1]; }
    for (uint32_t s = 0; s < a.nb; ++s) {
        const size_t i = (size_t)s * a.np + p;
        const int id = a.ids[i];
        float4 g0 = make_float4(1.f, 1.f, 1.f, 0.f), g1 = make_float4(0.f, 0.f, 0.f, 0.f);   // a miss
        if (id >= 0) {
            const Mat m = load_mat(a.mat, id);
            const float* rec = a.rec + 8 * i;
            if (m.tag == MAT_EMISSIVE) g0.w = 1.0f;
            else g0 = make_float4(fminf(fmaxf(m.color.x, 0.f), 1.f), fminf(fmaxf(m.color.y, 0.f), 1.f), fminf(fmaxf(m.color.z, 0.f), 1.f), 0.f);
            g1 = make_float4(rec[4], rec[5], rec[6], rec[0]);                         // face-forwarded normal, t
        }
        f0.x += g0.x; f0.y += g0.y; f0.z += g0.z; f0.w += g0.w;
        f1.x += g1.x; f1.y += g1.y; f1.z += g1.z; f1.w += g1.w;
    }
    if (a.finalize) {
        const float n = (float)a.n_samples;
        f0 = make_float4(pt_div(f0.x, n), pt_div(f0.y, n), pt_div(f0.z, n), pt_div(f0.w, n));
        f1 = make_float4(pt_div(f1.x, n), pt_div(f1.y, n), pt_div(f1.z, n), pt_div(f1.w, n));
    }
    a.out[2 * (size_t)p] = f0; a.out[2 * (size_t)p + 1] = f1;
}
}  // namespace PTK_IMPL
namespace ptk {
void PT_LAUNCH(launch_feature_rays)(const CameraF& cam, uint32_t s_base, uint32_t nb, float* rays6, hipStream_t st) {
    const uint32_t n = nb * cam.width * cam.height;
    if (n) hipLaunchKernelGGL(PTK_IMPL::k_feature_rays, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, cam, s_base, nb, rays6);
}
void PT_LAUNCH(launch_feature_resolve)(const FeatureResolveArgs& a, hipStream_t st) {
    if (a.np) hipLaunchKernelGGL(PTK_IMPL::k_feature_resolve, dim3((a.np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
}  // namespace ptk

#if !PT_MATH_EXACT
// ------------------------------------------------------------------ edge-avoiding a-trous denoiser (pt_denoise_device)
// The rule is stated in include/pathtrace_amd.h (PtDenoise) and DESIGN.md 5b.  One thread per pixel, one launch per step.
// State plane: float4 (u.rgb, var) per pixel, u = colour / max(albedo, 1e-3); the features: (albedo rgb, emitter),
// (normal xyz, depth).  Every tap is three 16-byte loads; at 1024^2 the 48 MB of the three planes stay in the Infinity Cache.
// The sums are formed as u_p + sum w (u_q - u_p) / sum w (the rule's sum w u_q / sum w): a flat region stays exactly flat.
namespace PTK_IMPL {
constexpr uint32_t kDnBx = 32, kDnBy = 8;      // a wave covers 32 x 2 pixels: its 5 x 5 taps touch few cache lines
PT_DEV float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
PT_DEV float dn_albedo(float a) { return fmaxf(a, 1e-3f); }
// c' = u * a, and the RGBA8 word of c' through k_resolve's gamma / clamp / `as u8` (world.rs:322-331)
PT_DEV void dn_store(const DenoiseArgs& a, size_t p, float ur, float ug, float ub, float4 f0) {
    const float c[3] = {ur * dn_albedo(f0.x), ug * dn_albedo(f0.y), ub * dn_albedo(f0.z)};
    uint32_t q8 = 0xFF000000u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.out_linear[3 * p + k] = c[k];
        const double gm = __builtin_sqrt((double)c[k]);
        const double cl = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);
        const double q = cl * 255.0;
        q8 |= (uint32_t)((q != q) ? (uint8_t)0 : (uint8_t)q) << (8 * k);
    }
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * p) = q8;
}
// demodulated colour of pixel q straight from the film
PT_DEV float3 dn_demod(const DenoiseArgs& a, size_t q) {
    const float4 f0 = a.feat[2 * q];
    return make_float3(a.linear[3 * q] / dn_albedo(f0.x), a.linear[3 * q + 1] / dn_albedo(f0.y), a.linear[3 * q + 2] / dn_albedo(f0.z));
}
// the 3 x 3 population variance of L(u) around pixel (x, y), taps outside the image skipped: k_denoise_temporal's variance
// of a pixel with fewer than 4 frames of history.  The statements are k_denoise_init's, in its order, so the value is the
// same bits (tests/test_gpu_temporal.py); k_denoise_init keeps its own text because calling this function there changes
// the instructions the compiler schedules for that kernel.
PT_DEV float dn_spatial_var(const DenoiseArgs& a, uint32_t x, uint32_t y) {
    float Ls[9];
    uint32_t cnt = 0;
    float sum = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx, qy = (int)y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) continue;
            const float3 uq = dn_demod(a, (size_t)qy * a.width + qx);
            Ls[cnt] = dn_lum(uq.x, uq.y, uq.z);
            sum += Ls[cnt];
            ++cnt;
        }
    const float mu = sum / (float)cnt;
    float var = 0.0f;
    for (uint32_t k = 0; k < cnt; ++k) var += (Ls[k] - mu) * (Ls[k] - mu);
    var /= (float)cnt;
    return var;
}
// first launch: u and the 3 x 3 population variance of L(u) (taps outside the image skipped); finalize: iterations = 0
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_init(DenoiseArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float3 u = dn_demod(a, p);
    float Ls[9];
    uint32_t cnt = 0;
    float sum = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx, qy = (int)y + dy;
            if (qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) continue;
            const float3 uq = dn_demod(a, (size_t)qy * a.width + qx);
            Ls[cnt] = dn_lum(uq.x, uq.y, uq.z);
            sum += Ls[cnt];
            ++cnt;
        }
    const float mu = sum / (float)cnt;
    float var = 0.0f;
    for (uint32_t k = 0; k < cnt; ++k) var += (Ls[k] - mu) * (Ls[k] - mu);
    var /= (float)cnt;
    if (a.finalize) dn_store(a, p, u.x, u.y, u.z, a.feat[2 * p]);
    else a.dst[p] = make_float4(u.x, u.y, u.z, var);
}
// one a-trous step of size h: the 3 x 3 Gaussian of var (renormalised over the in-image taps) gives g_p, then the 5 x 5
// B3-spline taps at (dx, dy) h with the edge-stopping weights; finalize: remodulate and write both film planes
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_step(DenoiseArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const int W = (int)a.width, H = (int)a.height, h = (int)a.step;
    const size_t p = (size_t)y * a.width + x;
    const float4 sp = a.src[p], f0p = a.feat[2 * p], f1p = a.feat[2 * p + 1];
    float4 res = sp;
    if (!(f0p.w > 0.0f)) {                     // an emitter pixel takes no other tap: it keeps (u, var)
        float gs = 0.0f, gw = 0.0f;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = (int)x + dx, qy = (int)y + dy;
                if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                gs += k * a.src[(size_t)qy * W + qx].w;
                gw += k;
            }
        const float g = __builtin_sqrtf(gs / gw);
        const float Lp = dn_lum(sp.x, sp.y, sp.z);
        const float inv_l = 1.0f / (a.sigma_l * g + 1e-10f);
        const float inv_d = 1.0f / (a.sigma_d * (float)h * fmaxf(f1p.w, 1e-3f) + 1e-10f);
        constexpr float kB3[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const float kc = kB3[2] * kB3[2];
        float wsum = kc, ar = 0.0f, ag = 0.0f, ab = 0.0f, av = kc * kc * sp.w;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int qy = (int)y + (j - 2) * h;
            if (qy < 0 || qy >= H) continue;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (i == 2 && j == 2) continue;
                const int qx = (int)x + (i - 2) * h;
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                const float4 sq = a.src[q], f0q = a.feat[2 * q], f1q = a.feat[2 * q + 1];
                const float nd = f1p.x * f1q.x + f1p.y * f1q.y + f1p.z * f1q.z;
                if (!(nd > 0.0f) || f0q.w > 0.0f) continue;
                const float el = fabsf(Lp - dn_lum(sq.x, sq.y, sq.z)) * inv_l;
                const float ed = fabsf(f1p.w - f1q.w) * inv_d;
                // k * nd^sigma_n * exp(-el - ed), as one exp2
                const float w = kB3[j] * kB3[i] * exp2f(a.sigma_n * log2f(nd) - (el + ed) * 1.44269504f);
                wsum += w;
                ar += w * (sq.x - sp.x); ag += w * (sq.y - sp.y); ab += w * (sq.z - sp.z);
                av += w * w * sq.w;
            }
        }
        const float inv = 1.0f / wsum;
        res = make_float4(sp.x + ar * inv, sp.y + ag * inv, sp.z + ab * inv, av * inv * inv);
    }
    if (a.finalize) dn_store(a, p, res.x, res.y, res.z, f0p);
    else a.dst[p] = res;
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_denoise(const DenoiseArgs& a, bool init, hipStream_t st) {
    const dim3 g((a.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    if (init) hipLaunchKernelGGL(PTK_IMPL::k_denoise_init, g, b, 0, st, a);
    else hipLaunchKernelGGL(PTK_IMPL::k_denoise_step, g, b, 0, st, a);
}
}  // namespace ptk

// ------------------------------------------------------------------ temporal accumulation (pt_denoise_temporal_device)
// The rule is stated in include/pathtrace_amd.h (PtTemporal) and DESIGN.md 5c.  One thread per pixel, in place of k_denoise_init.
// The reprojection runs in f64: an f32 solve puts x' about 1e-4 pixel off at 1024^2, and a bilinear tap of that weight moves
// a dim pixel next to a bright one by far more than the accumulation's own rounding.  Everything after it is f32.
namespace PTK_IMPL {
PT_DEV double tm_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PT_DEV void tm_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// pixel (x, y) at depth d seen from the frame's camera -> (x', y') in the history's image and d_exp; false: no reprojection
PT_DEV bool tm_reproject(const TemporalArgs& a, uint32_t x, uint32_t y, float d, double& xr, double& yr, double& dexp) {
    const double* o = a.cur; const double* l = a.cur + 3; const double* hz = a.cur + 6; const double* vt = a.cur + 9;
    const double* o2 = a.prev; const double* l2 = a.prev + 3; const double* hz2 = a.prev + 6; const double* vt2 = a.prev + 9;
    const double W1 = (double)(a.dn.width - 1u), H1 = (double)(a.dn.height - 1u);
    const double s = ((double)x + 0.5) / W1, t = ((double)(a.dn.height - 1u - y) + 0.5) / H1;      // camera.rs:139-147, world.rs:299
    double D[3], P[3], c[3], r[3], bc[3], rc[3], br[3];
    for (int k = 0; k < 3; ++k) D[k] = l[k] + s * hz[k] + t * vt[k] - o[k];
    const double inv_len = 1.0 / __builtin_sqrt(tm_dot(D, D));
    for (int k = 0; k < 3; ++k) {
        P[k] = o[k] + (double)d * (D[k] * inv_len);
        c[k] = o2[k] - P[k];                 // -(P - o')
        r[k] = o2[k] - l2[k];
    }
    // s' hz' + t' vt' + lambda c = r by Cramer's rule
    tm_cross(vt2, c, bc);
    const double det = tm_dot(hz2, bc);
    if (!(det != 0.0) || !__builtin_isfinite(det)) return false;
    tm_cross(r, c, rc);
    tm_cross(vt2, r, br);
    const double inv = 1.0 / det;
    const double s2 = tm_dot(r, bc) * inv, t2 = tm_dot(hz2, rc) * inv, lam = tm_dot(hz2, br) * inv;
    if (!(lam > 0.0) || !__builtin_isfinite(s2) || !__builtin_isfinite(t2) || !__builtin_isfinite(lam)) return false;
    xr = s2 * W1 - 0.5;
    yr = (double)a.dn.height - 0.5 - t2 * H1;
    dexp = __builtin_sqrt(tm_dot(c, c));
    return true;
}
__global__ void __launch_bounds__(kDnBx * kDnBy) k_denoise_temporal(TemporalArgs a) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.dn.width || y >= a.dn.height) return;
    const int W = (int)a.dn.width, H = (int)a.dn.height;
    const size_t p = (size_t)y * a.dn.width + x;
    const float4 f0p = a.dn.feat[2 * p], f1p = a.dn.feat[2 * p + 1];
    const float3 uc = dn_demod(a.dn, p);
    const float Lc = dn_lum(uc.x, uc.y, uc.z);
    // the valid-weighted history of the 2 x 2 bilinear taps around (x', y')
    float S = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hm1 = 0.0f, hm2 = 0.0f, hn = 0.0f;
    if (a.hist_src && f1p.w > 0.0f) {
        double xr = x, yr = y, dexp = f1p.w;
        const bool ok = a.same_camera || tm_reproject(a, x, y, f1p.w, xr, yr, dexp);
        if (ok && xr > -1.0 && xr < (double)W && yr > -1.0 && yr < (double)H) {      // else no tap lies inside the image
            const int x0 = (int)__builtin_floor(xr), y0 = (int)__builtin_floor(yr);
            const float fx = (float)(xr - x0), fy = (float)(yr - y0);
            const float de = (float)dexp, dmax = a.depth_tol * de;
            const bool em = f0p.w > 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int qx = x0 + i, qy = y0 + j;
                    const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                    if (!(w > 0.0f) || qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                    const size_t q = (size_t)qy * W + qx;
                    const float4 h2 = a.hist_src[3 * q + 2];
                    if (!(h2.w > 0.0f) || !(fabsf(h2.w - de) <= dmax)) continue;
                    if (!(f1p.x * h2.x + f1p.y * h2.y + f1p.z * h2.z >= a.normal_tol)) continue;
                    const float4 h1 = a.hist_src[3 * q + 1];
                    if (em != (h1.z > 0.0f)) continue;
                    const float4 h0 = a.hist_src[3 * q];
                    S += w;
                    hr += w * h0.x; hg += w * h0.y; hb += w * h0.z; hm1 += w * h0.w;
                    hm2 += w * h1.x; hn += w * h1.y;
                }
        }
    }
    float3 u = uc;
    float m1 = Lc, m2 = Lc * Lc, n = 1.0f;            // a fresh pixel
    if (S >= 1e-2f) {
        const float inv = 1.0f / S;
        const float ur = hr * inv, ug = hg * inv, ub = hb * inv, um1 = hm1 * inv, um2 = hm2 * inv;
        n = hn * inv + 1.0f;
        const float al = fmaxf(a.alpha, 1.0f / n);
        u = make_float3(ur + al * (uc.x - ur), ug + al * (uc.y - ug), ub + al * (uc.z - ub));
        m1 = um1 + al * (Lc - um1);
        m2 = um2 + al * (Lc * Lc - um2);
    }
    const float var = n >= 4.0f ? fmaxf(0.0f, m2 - m1 * m1) : dn_spatial_var(a.dn, x, y);
    a.hist_dst[3 * p] = make_float4(u.x, u.y, u.z, m1);
    a.hist_dst[3 * p + 1] = make_float4(m2, n, f0p.w, 0.0f);
    a.hist_dst[3 * p + 2] = f1p;
    if (a.dn.finalize) dn_store(a.dn, p, u.x, u.y, u.z, f0p);
    else a.dn.dst[p] = make_float4(u.x, u.y, u.z, var);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_denoise_temporal(const TemporalArgs& a, hipStream_t st) {
    const dim3 g((a.dn.width + PTK_IMPL::kDnBx - 1) / PTK_IMPL::kDnBx, (a.dn.height + PTK_IMPL::kDnBy - 1) / PTK_IMPL::kDnBy),
        b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_denoise_temporal, g, b, 0, st, a);
}
}  // namespace ptk
#endif      // !PT_MATH_EXACT
#endif      // PT_TU_MAIN
