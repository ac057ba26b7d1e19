// pt_kernels_bvh.hip -- the BVH form (PtRenderParams.accel = 1): traverse_segment, k_paths_bvh, k_debug_hit_bvh.  A translation
// unit of its own for its compiler options (pt_kernels_unit.h).
#include "pt_kernels_scan.h"
#include "pt_kernels_vertex.h"

namespace PTK_IMPL {

// hit_scene by BVH traversal (traverse_segment below).  Every primitive whose test the linear scan would have
// accepted is still tested: a subtree is skipped only if the ray misses its box, enlarged by `pad` on every
// side, inside [t_min, closest].  pad = 2^-15 (|o|_1 + scene extent) is ~100x the rounding error of the
// primitive tests (their error scales with the distance between ray origin and primitive), so a hit that exists
// only through rounding (a grazing ray) is inside the padded box as well.  Rays with a non-finite coordinate or
// a zero direction (the reference lets NaN through its sphere test, Q10) take the linear scan, from global
// memory (scan_global).  A visibility query only uses "is there a hit": the lane stops at its first accepted
// primitive.
constexpr float kBvhPad = 1.0f / 32768.0f;

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
}  // namespace PTK_IMPL
namespace ptk {
using namespace PTK_IMPL;
uint32_t PT_LAUNCH(launch_paths_bvh)(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st, bool diffuse, bool list) {
    if (list) return launch_paths_bvh_t<false, true>(a, grid, lds, st);        // pixel lists: the generic kernels only
    if (diffuse) return launch_paths_bvh_t<true, false>(a, grid, lds, st);
    return launch_paths_bvh_t<false, false>(a, grid, lds, st);
}
void PT_LAUNCH(launch_debug_hit_bvh)(const SceneView& sc, uint32_t grid, size_t lds, const float* rays6, uint32_t n, float t_min, float t_max,
                                     float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st) {
    // scratch: 3 planes of n float4 (two ray planes + result)
    hipLaunchKernelGGL(k_debug_hit_bvh, dim3(grid), dim3(kBlock), lds, st, sc, rays6, n, t_min, t_max, scratch,
                       scratch + n, scratch + 2 * (size_t)n, out_id, out_t, out_rec);
}
}  // namespace ptk
