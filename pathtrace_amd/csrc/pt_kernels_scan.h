// pt_kernels_scan.h -- device code every kernel unit shares: the primitive tests, the scene as a kernel sees it (SceneRef,
// stage_scene), World::hit_scene as a linear scan (scan_closest, scan_closest2, scan_global) and a few wave / index helpers.
#pragma once
#include "pt_kernels_unit.h"

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
    uint32_t n_spheres;     // SceneView::spheres_only: the scan array is spheres 0 .. n_spheres - 1 and nothing else; 0: walk the runs
    uint32_t lambert_surfaces;   // SceneView::lambert_surfaces: a path that goes on past a vertex stands on a Lambertian surface there
    BvhView bvh;
    uint32_t* stack;        // kModeBvh: LDS traversal stack, entry e of thread t at stack[e * kBlock + t]
};
template <int MODE>
PT_DEV SceneRef stage_scene(const SceneView& sc, float4* lds) {
    SceneRef r;
    r.n_runs = sc.n_runs; r.n_lights = sc.n_lights;
    r.n_spheres = sc.spheres_only ? sc.n_objs : 0u;
    r.lambert_surfaces = sc.lambert_surfaces;
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

// World::hit_scene (world.rs:270-290): linear scan in object order with a
// shrinking t_max.  kModeLds: the whole scan array already sits in LDS.  kModeTiled:
// every run is streamed through one LDS tile; the loop is block-uniform (all
// threads of the workgroup call this together, active or not).
// SPHERES (kModeLds; the caller has seen sc.n_spheres != 0): the scan array is ONE run of spheres at offset 0, objects 0 .. n - 1
// (SceneView::spheres_only, decided at upload).  The run's sphere code is entered directly with those constants: no loop over runs,
// no run record out of LDS, no dispatch on its tag -- the same tests on the same records in the same order, so the same bits.
template <int MODE, bool ANY = false, bool PF = false, bool SPHERES = false>
PT_DEV void scan_closest(const SceneRef& sc, f3 o, f3 d, float t_min, float t_max, int& id_out, float& t_out) {
    constexpr bool SMALL = MODE == kModeLds;
    float closest = t_max;
    int id = -1;
    if constexpr (SPHERES) {
        static_assert(SMALL, "the whole scan array in LDS");
        scan_run<false, ANY, PF>(sc.scan, SHAPE_SPHERE, sc.n_spheres, 0, o, d, t_min, closest, id);
    } else
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
// SPHERES: as scan_closest's -- scan_run2's sphere code on sc.scan[0 .. n_spheres), objects numbered from 0, groups of four, then a
// pair, then singles, each group behind a scalar branch on the count.  (Not a switch on the count into unrolled bodies: sixteen of
// them are 136 joint tests of code for the sake of immediate offsets, and the count's branches are scalar and few.)
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
template <int MODE, bool SPHERES = false>
PT_DEV void scan_closest2(const SceneRef& sc, f3 o, f3 da, float t_max_a, f3 db, float t_min, float t_max_b, int& id_a, int& id_b,
                          float& t_b) {
    static_assert(MODE == kModeLds, "the whole scan array in LDS");
    float closest = t_max_b;
    int ia = -1, ib = -1;
    if constexpr (SPHERES) scan_run2(sc.scan, SHAPE_SPHERE, sc.n_spheres, 0, o, da, db, t_min, t_max_a, ia, closest, ib);
    else
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

// HitRecord of the winning object (shape.rs:84-88 / 194-197 + base.rs:19-33): rec[8] = (t, point3, normal3, front_face)
PT_DEV void store_hit_record(const SceneRef& sc, int id, f3 o, f3 d, float t, float* rec) {
    Hit h;
    h.t = 0.0f; h.point = mk(0.f, 0.f, 0.f); h.normal = mk(0.f, 0.f, 0.f); h.front_face = false;
    if (id >= 0) h = finish_hit(sc.shape, id, load_mat(sc.mat, id).shape_tag, o, d, t);
    rec[0] = h.t; rec[1] = h.point.x; rec[2] = h.point.y; rec[3] = h.point.z;
    rec[4] = h.normal.x; rec[5] = h.normal.y; rec[6] = h.normal.z; rec[7] = h.front_face ? 1.0f : 0.0f;
}

}  // namespace PTK_IMPL
