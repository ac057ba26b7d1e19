// pt_kernels_vertex.h -- device code the path kernels of every unit share: one path vertex (vertex_begin / vertex_end /
// vertex_finish and the state they work on), the camera ray, the material sets, a wave's statistics.
#pragma once
#include "pt_kernels_scan.h"

namespace PTK_IMPL {

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
// A scene's ONLY light (sc.n_lights == 1; ONE below).  Which object it is, its shape tag, its first shape record and its emission
// are the same in every lane at every vertex of a launch: a kernel reads them once (load_one_light, after stage_scene) into scalar
// registers, and sample_light_point / vertex_begin / vertex_end take them from here where they otherwise read lights[], the light's
// material (twice: REMAT) and its shape record through per-lane addresses and branch on the tag lane by lane.  The samplers get the
// same numbers in the same order; only where an operand comes from differs.  An object that emits IS the light (the light list is the
// objects whose material emits: pt_host.cpp), so the look-ahead pdf of an emitter hit takes the same record.
struct OneLight {
    int obj;
    uint32_t shape_tag;
    float4 r0;               // sphere: (centre, radius); triangle: (v0, normal.x) -- its other records are read where they are needed
    f3 emission;
};
PT_DEV float wave_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
PT_DEV OneLight load_one_light(const SceneRef& sc) {
    const int obj = (int)sc.lights[0];
    const Mat lm = load_mat(sc.mat, obj);
    const float4 r0 = sc.shape[3 * obj];
    OneLight ol;
    ol.obj = __builtin_amdgcn_readfirstlane(obj);
    ol.shape_tag = (uint32_t)__builtin_amdgcn_readfirstlane((int)lm.shape_tag);
    ol.r0 = make_float4(wave_uniform(r0.x), wave_uniform(r0.y), wave_uniform(r0.z), wave_uniform(r0.w));
    ol.emission = mk(wave_uniform(lm.color.x), wave_uniform(lm.color.y), wave_uniform(lm.color.z));
    return ol;
}
// shape_sample for that light: the tag is wave-uniform, so the sampler is chosen by a scalar branch
PT_DEV void one_light_sample(const SceneRef& sc, const OneLight& ol, f3 from, bool with_target, f3 target, float r1, float r2, f3& point,
                             float& pdf_omega, f3& dir, float& dist) {
    if (ol.shape_tag == SHAPE_SPHERE) {
        sphere_sample(ol.r0, from, with_target, target, r1, r2, point, pdf_omega, dir, dist);
    } else {
        const float4 q1 = sc.shape[3 * ol.obj + 1], q2 = sc.shape[3 * ol.obj + 2];      // (one address for all lanes: broadcast reads)
        triangle_sample(mk(ol.r0.x, ol.r0.y, ol.r0.z), mk(q1.x, q1.y, q1.z), mk(q2.x, q2.y, q2.z), mk(ol.r0.w, q1.w, q2.w),
                        sc.mat[2 * ol.obj + 1].w, from, with_target, target, r1, r2, point, pdf_omega, dir, dist);
    }
}
template <int DIFFUSE, bool ONE = false>
PT_DEV void sample_light_point(const SceneRef& sc, f3 from, uint32_t w_index, uint32_t w_r1, uint32_t w_r2, f3& point,
                               int& lobj, f3& emission, float& pdf, f3& dir, float& dist, const OneLight* ol = nullptr) {
    if constexpr (ONE) {
        lobj = ol->obj;
        one_light_sample(sc, *ol, from, false, from, u01(w_r1), u01(w_r2), point, pdf, dir, dist);
        emission = ol->emission;                                                  // world.rs:259; pdf: world.rs:260 (x/1 == x)
        return;
    }
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
// ONE: the scene has exactly one light and `ol` holds it (OneLight above).
// SPHERES: every object is a sphere (SceneView::spheres_only): the hit record is finished by the sphere code, no shape tag is looked at.
template <bool MIS, int DIFFUSE, bool ONE = false, bool SPHERES = false>
PT_DEV void vertex_begin(const SceneRef& sc, PathState& p, bool active, int id, float t, uint32_t sample, uint32_t kx,
                         uint32_t py, Vertex& v, const OneLight* ol = nullptr) {
    v.alive = active && id >= 0;
    v.obj = id >= 0 ? id : 0; v.light_obj = 0;
    v.hit_emitter = false; v.emit_pdf_shape = 0.0f;
    v.hit.point = p.o; v.hit.normal = p.d; v.hit.t = 0.0f; v.hit.front_face = false;
    v.m.tag = MAT_LAMBERT; v.m.shape_tag = 0; v.m.emits = 0; v.m.color = mk(0.f, 0.f, 0.f);
    v.m.roughness = 0.f; v.m.metallic = 0.f; v.m.ior = 1.f; v.m.on_a = 1.f; v.m.on_b = 0.f;
    if (v.alive) {
        v.m = load_mat(sc.mat, id);
        assume_mats<DIFFUSE>(v.m.tag);
        if constexpr (SPHERES) v.hit = finish_hit(sc.shape, id, SHAPE_SPHERE, p.o, p.d, t);
        else v.hit = finish_hit(sc.shape, id, v.m.shape_tag, p.o, p.d, t);
        if (v.m.emits) {
            v.hit_emitter = true;
            if (MIS && p.depth != 0u) {
                // emitter reached by a BSDF-sampled ray: its MIS weight (vertex_end) is against the light pdf of
                // this point seen from the previous vertex = this ray's origin (rendering.rs:107-116)
                f3 sp, sd; float sl;
                if constexpr (ONE) one_light_sample(sc, *ol, p.o, true, v.hit.point, 0.f, 0.f, sp, v.emit_pdf_shape, sd, sl);
                else shape_sample(sc.shape, sc.mat, id, v.m.shape_tag, p.o, true, v.hit.point, 0.f, 0.f, sp, v.emit_pdf_shape, sd, sl);
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
        if (MIS && (ONE || sc.n_lights > 0u)) {
            uint32_t w_index = 0u;                                                // umulhi(u, 1) = 0: one light needs no draw
            if (!ONE && sc.n_lights > 1u) {
                uint32_t dc[4];
                philox4x32_draw(kx, py, sample, p.depth, BLK_CHOICE, 0u, dc);
                w_index = dc[0]; v.w_lobe = dc[1];
            }
            f3 lp;                                                                // rendering.rs:58-60: direction and distance
            sample_light_point<DIFFUSE, ONE>(sc, v.hit.point, w_index, ds[0], ds[1], lp, v.light_obj, v.ls_emission, v.ls_pdf,
                                             v.light_dir, v.distance, ol);        // to the point, from the sampler itself
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
// ONE: the light's emission is ol.emission; nothing of the light is read again.
// LAMBERT (SceneView::lambert_surfaces, decided at upload; REMAT only): every object is Lambertian or an Emissive that emits.  A hit
// on one that emits ends the path in vertex_begin, so a lane with need_shadow or alive set stands on a Lambertian surface: the re-read
// fetches the object's colour and nothing else (an emitter's colour for its credit: the same three words), bsdf_pdf and
// bsdf_pdf_sample are entered with the tag a constant, the sampled direction is the cosine sampler's as it is (normalised there), and
// eta_here is 1: pt_rcp(1) is exactly 1 in both arithmetic modes, Lambert's bsdf_pdf reads no eta, and p.eta_in, 1 when the path
// started, is never written.  What remains has the operands and the order it had.
template <bool MIS, int DIFFUSE, bool REMAT, bool DEFER = false, bool ONE = false, bool LAMBERT = false>
PT_DEV bool vertex_end(const SceneRef& sc, PathState& p, const Vertex& vin, bool visible, uint32_t sample, uint32_t kx,
                       uint32_t py, uint32_t min_depth, uint32_t max_depth, Pending* pd = nullptr, const OneLight* ol = nullptr) {
    const uint32_t n_lights = ONE ? 1u : sc.n_lights;
    Vertex v = vin;
    if (REMAT) {
        asm volatile("" ::: "memory");          // a real re-read, not the values of vertex_begin kept alive
        if constexpr (LAMBERT) {
            const float4 m0 = sc.mat[2 * vin.obj];
            v.m.tag = MAT_LAMBERT; v.m.color = mk(m0.y, m0.z, m0.w);
        } else {
            v.m = load_mat(sc.mat, vin.obj);
        }
        if constexpr (!ONE) v.ls_emission = load_mat(sc.mat, vin.light_obj).color;
    }
    if constexpr (ONE) v.ls_emission = ol->emission;
    static_assert(!LAMBERT || (REMAT && DIFFUSE == kMatsDiffuse), "a Lambert-surfaced scene is a diffuse one, its material re-read here");
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
        if constexpr (LAMBERT) eta_here = 1.0f;                                // pt_rcp(1) == 1 exactly, fast and exact arithmetic
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
                if constexpr (!LAMBERT) p.eta_in = eta_here;                  // :87 (LAMBERT: it is 1 and stays 1)
                p.depth += 1u;
            }
        }
    }
    return alive;
}

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
// the regenerating kernels' per-wave ring of camera rays in LDS (k_paths_regen, k_paths_regen_split)
constexpr uint32_t kPool = 128;            // ring entries per wave (>= 2 chunks: refilled whenever fewer than 64 are left)
// k_paths_regen<.., DENSE0>: a wave's LDS.  A ring entry is a path AFTER its first vertex, 19 words: origin, direction,
// throughput, sampling pdf, its pending NEE term, that term's visibility ray (direction, range), film position, sample | depth;
// four 16-byte planes and three word planes.  At most one chunk's survivors are in the ring at a time (64 entries).  Behind them
// the six parked floats of every lane.  6400 B per wave: with a scene of <= 78 float4 six workgroups still fit a CU's 160 KB.
struct alignas(16) DenseWave {
    float4 e4[4][64];
    uint32_t e1[3][64];
    float4 park0[64];
    float2 park1[64];
};

}  // namespace PTK_IMPL
