// pt_kernels_split.hip -- k_paths_regen_split: the regenerating level-0 kernel (k_paths_regen, pt_kernels_main.hip) for scenes
// with a few Mirror objects.  A translation unit of its own for its compiler options (pt_kernels_unit.h).
#include "pt_kernels_scan.h"
#include "pt_kernels_vertex.h"

namespace PTK_IMPL {

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

}  // namespace PTK_IMPL
namespace ptk {
using namespace PTK_IMPL;
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
}  // namespace ptk
