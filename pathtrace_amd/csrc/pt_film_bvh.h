// pt_film_bvh.h -- part of the film unit (its options, and compiled once: none of this depends on the arithmetic mode):
// included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_bvh.h"

// ------------------------------------------------------------------ device-side BVH refit (pt_scene_refit)
// The rule is ptbvh::refit (pt_bvh.h / pt_bvh.cpp) and DESIGN.md 5e; these kernels reproduce its arrays bit for bit.  That is a
// requirement: the grid comes from the HOST's boxes and the quantisation clamps to it, so a device box one ulp outside the
// host's would be quantised to a box that no longer encloses it.  Hence f64 + - * / sqrt floor ceil (correctly rounded on the
// device as on the host), no contraction, the host's compare-and-step outward rounding, and fmaf for the decode as there.
// None of it depends on the arithmetic mode.
namespace PTK_IMPL {
// ptbvh's down() / up(): the f32 at or below / at or above v
PT_DEV float refit_down(double v) {
    float f = (float)v;
    if ((double)f > v) {                       // step to the next f32 below (nextafterf(f, -inf))
        const uint32_t b = __float_as_uint(f);
        f = f > 0.0f ? __uint_as_float(b - 1u) : f == 0.0f ? __uint_as_float(0x80000001u) : __uint_as_float(b + 1u);
    }
    return f;
}
PT_DEV float refit_up(double v) {
    float f = (float)v;
    if ((double)f < v) {                       // nextafterf(f, +inf)
        const uint32_t b = __float_as_uint(f);
        f = f < 0.0f ? __uint_as_float(b - 1u) : f == 0.0f ? __uint_as_float(0x00000001u) : __uint_as_float(b + 1u);
    }
    return f;
}
// ptbvh::primitive_box for a finite primitive (the host drops the tree before any launch when an object is not finite)
PT_DEV void refit_primitive_box(const float4& r0, const float4& r1, const float4& r2, bool tri, float lo[3], float hi[3]) {
#pragma clang fp contract(off)
    if (!tri) {
        const float r2f = r0.w * r0.w;
        const double r = __builtin_sqrt((double)r2f) * (1.0 + 1e-7);
        const double c[3] = {r0.x, r0.y, r0.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = refit_down(c[k] - r); hi[k] = refit_up(c[k] + r); }
    } else {
        const double v0[3] = {r0.x, r0.y, r0.z}, e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = v0[k], b = v0[k] + e1[k], c = v0[k] + e2[k];
            const double mn_bc = c < b ? c : b, mx_bc = b < c ? c : b;      // std::min / std::max
            lo[k] = refit_down(mn_bc < a ? mn_bc : a);
            hi[k] = refit_up(a < mx_bc ? mx_bc : a);
        }
    }
}
// Box::grow
PT_DEV void refit_grow(float lo[3], float hi[3], const float4& blo, const float4& bhi) {
    lo[0] = blo.x < lo[0] ? blo.x : lo[0]; lo[1] = blo.y < lo[1] ? blo.y : lo[1]; lo[2] = blo.z < lo[2] ? blo.z : lo[2];
    hi[0] = hi[0] < bhi.x ? bhi.x : hi[0]; hi[1] = hi[1] < bhi.y ? bhi.y : hi[1]; hi[2] = hi[2] < bhi.z ? bhi.z : hi[2];
}
// quantise()'s q_lo / q_hi: the grid plane at or below / at or above v, by the decode the traversal evaluates
PT_DEV uint32_t refit_q_lo(float v, float gmin, float cell) {
#pragma clang fp contract(off)
    long long q = (long long)__builtin_floor(((double)v - (double)gmin) / (double)cell);
    q = q < 0 ? 0 : q > 65535 ? 65535 : q;
    while (q > 0 && __builtin_fmaf((float)(uint32_t)q, cell, gmin) > v) --q;
    return (uint32_t)q;
}
PT_DEV uint32_t refit_q_hi(float v, float gmin, float cell) {
#pragma clang fp contract(off)
    long long q = (long long)__builtin_ceil(((double)v - (double)gmin) / (double)cell);
    q = q < 0 ? 0 : q > 65535 ? 65535 : q;
    while (q < 65535 && __builtin_fmaf((float)(uint32_t)q, cell, gmin) < v) ++q;
    return (uint32_t)q;
}

// One thread per leaf slot: the slot's scan records (make_leaf's) and the primitive's f32 box.  Padding slots keep their zeros.
__global__ void __launch_bounds__(kBlock) k_bvh_refit_leaves(BvhRefitArgs a) {
    if (blockIdx.x == 0u && threadIdx.x < 3u) a.cost[threadIdx.x] = 0ull;      // the level launches add to them
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= a.n_slots) return;
    const uint32_t w = a.ids[slot];
    if (w == ptbvh::kDone) return;
    const uint32_t o = w & ~ptbvh::kTriangleBit;
    const bool tri = (w & ptbvh::kTriangleBit) != 0u;
    const float4 r0 = a.shape[3 * (size_t)o], r1 = a.shape[3 * (size_t)o + 1], r2 = a.shape[3 * (size_t)o + 2];
    float4 rec[3];
    if (tri) {
        ptbvh::triangle_scan_record(r0, r1, r2, rec);
    } else {
        rec[0] = make_float4(r0.x, r0.y, r0.z, r0.w * r0.w);                   // (c, r^2)
        rec[1] = make_float4(0.f, 0.f, 0.f, 0.f); rec[2] = rec[1];
    }
    a.rec[3 * (size_t)slot] = rec[0]; a.rec[3 * (size_t)slot + 1] = rec[1]; a.rec[3 * (size_t)slot + 2] = rec[2];
    a.lead[slot] = rec[0];
    float lo[3], hi[3];
    refit_primitive_box(r0, r1, r2, tri, lo, hi);
    a.slot_box[2 * (size_t)slot] = make_float4(lo[0], lo[1], lo[2], 0.f);
    a.slot_box[2 * (size_t)slot + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

// The nodes order[first, first + count) -- one height --, four lanes per node, one per child slot.  A lane forms its child's
// f32 box (a leaf: the union of its slots' boxes; a node: that node's stored union, written by an earlier launch), the four
// lanes' union is stored for the parent, each lane quantises its box, and the twelve box words are regrouped across the
// four lanes into the node's three 16-byte stores.  The cost terms are summed over the wave before one 64-bit atomic add
// per sum and wave: integer sums, so the result does not depend on the order.
__global__ void __launch_bounds__(kBlock) k_bvh_refit_level(BvhRefitArgs a, uint32_t first, uint32_t count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x, pos = t >> 2, c = t & 3u;
    const uint32_t lane = threadIdx.x & 63u;
    const bool node_ok = pos < count;
    uint32_t k = 0u, code = ptbvh::kDone;
    uint4 codes = make_uint4(ptbvh::kDone, ptbvh::kDone, ptbvh::kDone, ptbvh::kDone);
    if (node_ok) {
        k = a.order[first + pos];
        codes = a.nodes[4 * (size_t)k + 3];
        code = c == 0u ? codes.x : c == 1u ? codes.y : c == 2u ? codes.z : codes.w;
    }
    const bool used = code != ptbvh::kDone;    // the builder fills the child slots from 0 and gives the rest the sentinel
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    if (used) {
        if (code & ptbvh::kLeafBit) {
            const uint32_t s0 = code & 0x0FFFFFFFu, cnt = ((code >> 28) & 7u) + 1u;
            for (uint32_t i = s0; i < s0 + cnt && i < a.n_slots; ++i) refit_grow(lo, hi, a.slot_box[2 * (size_t)i], a.slot_box[2 * (size_t)i + 1]);
        } else {
            refit_grow(lo, hi, a.node_box[2 * (size_t)code], a.node_box[2 * (size_t)code + 1]);
        }
    }
    // the node's own union (an unused slot's box is empty: it changes nothing)
    float ulo[3], uhi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        ulo[d] = fminf(lo[d], __shfl_xor(lo[d], 1)); ulo[d] = fminf(ulo[d], __shfl_xor(ulo[d], 2));
        uhi[d] = fmaxf(hi[d], __shfl_xor(hi[d], 1)); uhi[d] = fmaxf(uhi[d], __shfl_xor(uhi[d], 2));
    }
    if (node_ok && c == 0u) {
        a.node_box[2 * (size_t)k] = make_float4(ulo[0], ulo[1], ulo[2], 0.f);
        a.node_box[2 * (size_t)k + 1] = make_float4(uhi[0], uhi[1], uhi[2], 0.f);
    }
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u;        // unused slot: zero words
    unsigned long long sxy = 0ull, syz = 0ull, szx = 0ull;
    if (used) {
        const uint32_t lx = refit_q_lo(lo[0], a.grid_min[0], a.grid_cell[0]), ly = refit_q_lo(lo[1], a.grid_min[1], a.grid_cell[1]),
                       lz = refit_q_lo(lo[2], a.grid_min[2], a.grid_cell[2]);
        const uint32_t hx = refit_q_hi(hi[0], a.grid_min[0], a.grid_cell[0]), hy = refit_q_hi(hi[1], a.grid_min[1], a.grid_cell[1]),
                       hz = refit_q_hi(hi[2], a.grid_min[2], a.grid_cell[2]);
        w0 = lx | (ly << 16); w1 = lz | (hx << 16); w2 = hy | (hz << 16);
        const unsigned long long dx = hx - lx, dy = hy - ly, dz = hz - lz;
        sxy = dx * dy; syz = dy * dz; szx = dz * dx;
    }
    // word j of the node (j < 12) = word j % 3 of child j / 3; lane c < 3 stores uint4 c = words 4c .. 4c + 3, which lie in
    // children c and c + 1: (w0 w1 w2 | w0'), (w1 w2 | w0' w1'), (w2 | w0' w1' w2')
    const uint32_t base = lane & ~3u, src_a = base + (c < 3u ? c : 0u), src_b = base + (c < 3u ? c + 1u : 0u);
    const uint32_t a0 = __shfl(w0, src_a), a1 = __shfl(w1, src_a), a2 = __shfl(w2, src_a);
    const uint32_t b0 = __shfl(w0, src_b), b1 = __shfl(w1, src_b), b2 = __shfl(w2, src_b);
    if (node_ok && c < 3u) {
        const uint4 v = c == 0u ? make_uint4(a0, a1, a2, b0) : c == 1u ? make_uint4(a1, a2, b0, b1) : make_uint4(a2, b0, b1, b2);
        a.nodes[4 * (size_t)k + c] = v;
    }
    if (node_ok && c == 3u) a.nodes[4 * (size_t)k + 3] = codes;                 // the code word, carried over
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sxy += __shfl_xor(sxy, off); syz += __shfl_xor(syz, off); szx += __shfl_xor(szx, off);
    }
    if (lane == 0u && (sxy | syz | szx) != 0ull) {
        atomicAdd(a.cost, sxy); atomicAdd(a.cost + 1, syz); atomicAdd(a.cost + 2, szx);
    }
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_bvh_refit_leaves(const BvhRefitArgs& a, hipStream_t st) {
    if (a.n_slots) hipLaunchKernelGGL(PTK_IMPL::k_bvh_refit_leaves, dim3((a.n_slots + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
void launch_bvh_refit_level(const BvhRefitArgs& a, uint32_t first, uint32_t count, hipStream_t st) {
    if (count) hipLaunchKernelGGL(PTK_IMPL::k_bvh_refit_level, dim3((uint32_t)(((uint64_t)count * 4u + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, first, count);
}
}  // namespace ptk

// ------------------------------------------------------------------ device-side BVH build (pt_scene_rebuild)
// The rule is ptbvh::build_morton (pt_bvh.h) and DESIGN.md 5f.  The topology is a function of the object count and comes from
// the host once; what these kernels decide is the order of the objects: (Morton key, index) ascending.  The key is the host's
// expression on the host's boxes (refit_primitive_box) and the host's grid, in correctly rounded f64; the order is total, so a
// correct sort reproduces the host's leaf_ids bit for bit.
namespace PTK_IMPL {
static_assert(kBlock == 256 && kSortDigits == kBlock, "one thread per digit");
constexpr uint32_t kSortRounds = kSortTile / kBlock;
constexpr uint32_t kSortWaves = kBlock / 64;
constexpr uint32_t kScanBlock = 1024;      // k_bvh_sort_scan: one workgroup, four words per thread and step

// digit of a pass: the pair as one 64-bit key, .x the low word (shift is a multiple of 8: a digit lies in one word)
PT_DEV uint32_t sort_digit(const uint2& kv, uint32_t shift) {
    return ((shift < 32u ? kv.x >> shift : kv.y >> (shift - 32u))) & (kSortDigits - 1u);
}

__global__ void __launch_bounds__(kBlock) k_bvh_morton(BvhBuildArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 r0 = a.shape[3 * (size_t)i], r1 = a.shape[3 * (size_t)i + 1], r2 = a.shape[3 * (size_t)i + 2];
    float lo[3], hi[3];
    refit_primitive_box(r0, r1, r2, a.tags[i] != 0u, lo, hi);
    const float gmin[3] = {a.grid_min[0], a.grid_min[1], a.grid_min[2]}, cell[3] = {a.grid_cell[0], a.grid_cell[1], a.grid_cell[2]};
    a.pairs[0][i] = make_uint2(ptbvh::morton_key(lo, hi, gmin, cell), i);
}

// One pass of the sort, part 1: how many keys of tile blockIdx.x carry each value of the pass's digit -> hist[digit * tiles + tile]
__global__ void __launch_bounds__(kBlock) k_bvh_sort_hist(const uint2* __restrict__ in, uint32_t* __restrict__ hist, uint32_t n, uint32_t tiles, uint32_t shift) {
    __shared__ uint32_t h[kSortDigits];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortTile;
    for (uint32_t r = 0; r < kSortRounds; ++r) {
        const uint32_t i = base + r * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&h[sort_digit(in[i], shift)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// Part 2: the exclusive prefix sum over hist as one array (digit-major: all tiles of digit 0, then of digit 1, ...), in place:
// afterwards hist[digit * tiles + tile] is where that tile's first key with that digit goes.  One workgroup walks the array
// with a running carry; `total` = 256 * tiles is a multiple of 4 and the array is 16-byte aligned.
__global__ void __launch_bounds__(kScanBlock) k_bvh_sort_scan(uint32_t* hist, uint32_t total) {
    __shared__ uint32_t wsum[kScanBlock / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < total; base += 4u * kScanBlock) {
        const uint32_t i = base + 4u * threadIdx.x;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < total) v = *reinterpret_cast<const uint4*>(hist + i);
        const uint32_t s = v.x + v.y + v.z + v.w;
        uint32_t x = s;                                          // inclusive scan over the wave
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63u) wsum[wave] = x;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kScanBlock / 64; ++w) { const uint32_t t = wsum[w]; before += w < wave ? t : 0u; all += t; }
        if (i < total) {
            const uint32_t e = carry + before + x - s;
            *reinterpret_cast<uint4*>(hist + i) = make_uint4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
        }
        carry += all;
        __syncthreads();
    }
}

// Part 3: every key of the tile to its place.  The tile is taken in rounds of one key per thread, in index order.  Within a
// round a key's rank among the keys with the same digit is: the lanes below it in its wave with that digit (the lanes that
// agree on all eight digit bits, by eight ballots) + the counts of that digit in the waves before (through LDS); base[digit]
// then moves on by the round's count.  Input order is kept among equal digits: the pass is stable.
__global__ void __launch_bounds__(kBlock) k_bvh_sort_scatter(const uint2* __restrict__ in, uint2* __restrict__ out, const uint32_t* __restrict__ hist, uint32_t n,
                                                             uint32_t tiles, uint32_t shift) {
    __shared__ uint32_t base[kSortDigits];
    __shared__ uint32_t wcnt[kSortWaves][kSortDigits];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    base[tid] = hist[(size_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) wcnt[w][tid] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * kSortTile;
    for (uint32_t r = 0; r < kSortRounds; ++r) {
        if (first + r * kBlock >= n) break;                      // (the same for every thread of the workgroup)
        const uint32_t i = first + r * kBlock + tid;
        const bool valid = i < n;
        const uint2 kv = valid ? in[i] : make_uint2(0u, 0u);
        const uint32_t d = sort_digit(kv, shift);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = ((d >> b) & 1u) != 0u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)), cnt = (uint32_t)__popcll(same);
        if (valid && rank == 0u) wcnt[wave][d] = cnt;            // one lane per digit present in the wave
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
#pragma unroll
            for (uint32_t w = 0; w < kSortWaves; ++w) pos += w < wave ? wcnt[w][d] : 0u;
            if (pos < n) out[pos] = kv;
        }
        __syncthreads();
        uint32_t add = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; ++w) { add += wcnt[w][tid]; wcnt[w][tid] = 0u; }
        base[tid] += add;
        __syncthreads();
    }
}

// One thread per leaf slot: the object of sorted position p (pairs == nullptr: object p) with its triangle bit; the padding
// slots behind the last object get the sentinel and zero records, as build() leaves them.
__global__ void __launch_bounds__(kBlock) k_bvh_write_ids(BvhBuildArgs a, const uint2* pairs) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.n_slots) return;
    uint32_t w = ptbvh::kDone;
    if (p < a.n) {
        const uint32_t o = pairs ? pairs[p].y : p;
        if (o < a.n) w = o | (a.tags[o] != 0u ? ptbvh::kTriangleBit : 0u);
    }
    a.ids[p] = w;
    if (w == ptbvh::kDone) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        a.rec[3 * (size_t)p] = z; a.rec[3 * (size_t)p + 1] = z; a.rec[3 * (size_t)p + 2] = z;
        a.lead[p] = z;
    }
}

// The child codes of the cached topology into the code words of the node array
__global__ void __launch_bounds__(kBlock) k_bvh_codes(uint4* nodes, const uint4* __restrict__ codes, uint32_t n_nodes) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k < n_nodes) nodes[4 * (size_t)k + 3] = codes[k];
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_bvh_morton(const BvhBuildArgs& a, hipStream_t st) {
    if (a.n) hipLaunchKernelGGL(PTK_IMPL::k_bvh_morton, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
// `passes` stable passes over the digits from bit 0 upward, from pairs[src]; returns the buffer that holds the result
static uint32_t bvh_sort_passes(const BvhBuildArgs& a, uint32_t src, uint32_t passes, hipStream_t st) {
    const uint32_t tiles = bvh_sort_tiles(a.n);
    for (uint32_t pass = 0; pass < passes; ++pass, src ^= 1u) {
        const uint2* in = a.pairs[src];
        uint2* out = a.pairs[src ^ 1u];
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_sort_hist, dim3(tiles), dim3(kBlock), 0, st, in, a.hist, a.n, tiles, 8u * pass);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_sort_scan, dim3(1), dim3(PTK_IMPL::kScanBlock), 0, st, a.hist, kSortDigits * tiles);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_sort_scatter, dim3(tiles), dim3(kBlock), 0, st, in, out, (const uint32_t*)a.hist, a.n, tiles, 8u * pass);
    }
    return src;
}
void launch_bvh_sort(const BvhBuildArgs& a, hipStream_t st) {
    if (a.n) bvh_sort_passes(a, 0u, 4u, st);                     // the 32-bit key; an even number of passes: the result is in pairs[0]
}
void launch_bvh_write_ids(const BvhBuildArgs& a, bool sorted, hipStream_t st) {
    if (a.n_slots) hipLaunchKernelGGL(PTK_IMPL::k_bvh_write_ids, dim3((a.n_slots + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a, sorted ? (const uint2*)a.pairs[0] : (const uint2*)nullptr);
}
void launch_bvh_codes(uint4* nodes, const uint4* codes, uint32_t n_nodes, hipStream_t st) {
    if (n_nodes) hipLaunchKernelGGL(PTK_IMPL::k_bvh_codes, dim3((n_nodes + kBlock - 1) / kBlock), dim3(kBlock), 0, st, nodes, codes, n_nodes);
}
}  // namespace ptk

// ------------------------------------------------------------------ device-side BVH build, median order (pt_scene_rebuild_ordered)
// The rule is ptbvh::build_median (pt_bvh.h) and DESIGN.md 5i.  Every step orders its positions by (cell on the step's axis,
// object index), a total order: whatever sorts correctly reproduces the host's leaf_ids bit for bit.  Steps above T positions
// go through the radix sort, level by level; a step of at most T positions and everything beneath it is one workgroup's work.
namespace PTK_IMPL {
constexpr uint32_t kMedianT = ptbvh::kMedianTile;
constexpr uint32_t kMedianBlock = 1024;
constexpr uint32_t kMedianPer = kMedianT / kMedianBlock;     // positions per thread
constexpr uint32_t kMedianMaxSteps = 512;                    // a tile has at most T / 4 leaves, so fewer steps than that
static_assert(kMedianT % kMedianBlock == 0 && kMedianT / 4 <= kMedianMaxSteps && kMedianT < 65536, "tile steps are 16-bit offsets");
struct MedianCell { float c[3]; };

__global__ void __launch_bounds__(kBlock) k_bvh_cells(BvhBuildArgs a, uint2* __restrict__ cells) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const float4 r0 = a.shape[3 * (size_t)i], r1 = a.shape[3 * (size_t)i + 1], r2 = a.shape[3 * (size_t)i + 2];
    float lo[3], hi[3];
    refit_primitive_box(r0, r1, r2, a.tags[i] != 0u, lo, hi);
    const float gmin[3] = {a.grid_min[0], a.grid_min[1], a.grid_min[2]}, cell[3] = {a.grid_cell[0], a.grid_cell[1], a.grid_cell[2]};
    const uint32_t g0 = ptbvh::grid_coord(lo, hi, gmin, cell, 0), g1 = ptbvh::grid_coord(lo, hi, gmin, cell, 1), g2 = ptbvh::grid_coord(lo, hi, gmin, cell, 2);
    cells[i] = make_uint2(g0 | (g1 << 16), g2);
    a.pairs[0][i] = make_uint2(i, 0u);
}

// the group of position p: the last one that starts at or before it (the first group starts at 0)
PT_DEV uint32_t median_group(const uint32_t* __restrict__ gs, uint32_t groups, uint32_t p) {
    uint32_t lo = 0u, hi = groups;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((gs[mid] & 0x7FFFFFFFu) <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// the rule's axis from the six bound words of a step
PT_DEV uint32_t median_axis(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t mx, uint32_t my, uint32_t mz, const MedianCell& cell) {
#pragma clang fp contract(off)
    // n* = 65535 - minimum: maximum - minimum = m + n - 65535
    const double wx = (double)(mx + nx - 65535u) * (double)cell.c[0], wy = (double)(my + ny - 65535u) * (double)cell.c[1],
                 wz = (double)(mz + nz - 65535u) * (double)cell.c[2];
    uint32_t axis = 0u;
    double widest = wx;
    if (wy > widest) { widest = wy; axis = 1u; }
    if (wz > widest) axis = 2u;
    return axis;
}

__global__ void __launch_bounds__(kBlock) k_bvh_median_bounds(const uint2* __restrict__ pairs, const uint2* __restrict__ cells, const uint32_t* __restrict__ gs,
                                                              uint32_t groups, uint32_t* bounds, uint32_t n, uint32_t mask) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = p < n;
    const uint32_t grp = median_group(gs, groups, valid ? p : n - 1u);
    const bool step = (gs[grp] >> 31) != 0u;
    uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};                     // 0 changes no maximum
    if (valid && step) {
        const uint32_t o = pairs[p].x & mask;
        if (o < n) {
            const uint2 c = cells[o];
            const uint32_t g0 = c.x & 0xFFFFu, g1 = c.x >> 16, g2 = c.y & 0xFFFFu;
            v[0] = 65535u - g0; v[1] = 65535u - g1; v[2] = 65535u - g2; v[3] = g0; v[4] = g1; v[5] = g2;
        }
    }
    const uint32_t grp0 = __builtin_amdgcn_readfirstlane(grp);
    if (__ballot(grp != grp0) == 0ull) {                         // one group in the wave: six atomics for all of it
#pragma unroll
        for (int k = 0; k < 6; ++k)
            for (int off = 32; off > 0; off >>= 1) { const uint32_t w = (uint32_t)__shfl_xor((int)v[k], off); v[k] = w > v[k] ? w : v[k]; }
        if ((threadIdx.x & 63u) == 0u && step)
            for (int k = 0; k < 6; ++k) atomicMax(&bounds[6 * (size_t)grp + k], v[k]);
    } else if (valid && step) {
        for (int k = 0; k < 6; ++k) atomicMax(&bounds[6 * (size_t)grp + k], v[k]);
    }
}

__global__ void __launch_bounds__(kBlock) k_bvh_median_keys(uint2* pairs, const uint2* __restrict__ cells, const uint32_t* __restrict__ gs, uint32_t groups,
                                                            const uint32_t* __restrict__ bounds, MedianCell cell, uint32_t n, uint32_t index_bits, uint32_t mask) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t o = pairs[p].x & mask;
    const uint32_t grp = median_group(gs, groups, p);
    const uint32_t start = gs[grp];
    uint32_t v = p - (start & 0x7FFFFFFFu);                      // no step: the position stays (a group has at most 65536)
    if ((start >> 31) != 0u) {
        const uint32_t* b = bounds + 6 * (size_t)grp;
        const uint32_t axis = median_axis(b[0], b[1], b[2], b[3], b[4], b[5], cell);
        const uint2 c = cells[o < n ? o : 0u];
        v = axis == 0u ? c.x & 0xFFFFu : axis == 1u ? c.x >> 16 : c.y & 0xFFFFu;
    }
    const unsigned long long key = ((unsigned long long)grp << (16u + index_bits)) | ((unsigned long long)(v & 0xFFFFu) << index_bits) | o;
    pairs[p] = make_uint2((uint32_t)key, (uint32_t)(key >> 32));
}

__global__ void __launch_bounds__(kBlock) k_bvh_median_unpack(const uint2* __restrict__ in, uint2* __restrict__ out, uint32_t n, uint32_t mask) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) out[p] = make_uint2(0u, in[p].x & mask);
}

// One workgroup per tile.  The tile's objects (cells and index) stand in LDS in position order; level by level every step of
// the tile takes its bounds (LDS atomics), its axis, and then every position its rank among the keys (cell << 32 | index) of
// its step -- the keys differ, so the ranks are the new positions.  Positions no step of a level covers stay.
__global__ void __launch_bounds__(kMedianBlock) k_bvh_median_tile(const uint2* __restrict__ in, uint2* __restrict__ out, const uint2* __restrict__ cells,
                                                                  const uint4* __restrict__ tiles, const uint2* __restrict__ tile_steps, MedianCell cell,
                                                                  uint32_t n, uint32_t mask) {
    __shared__ uint32_t e_g01[kMedianT], e_g2[kMedianT], e_obj[kMedianT];
    __shared__ unsigned long long key[kMedianT];
    __shared__ uint2 steps[kMedianMaxSteps];
    __shared__ uint32_t bnd[6 * kMedianMaxSteps];
    __shared__ uint32_t axis_of[kMedianMaxSteps];
    const uint32_t tid = threadIdx.x;
    const uint4 tl = tiles[blockIdx.x];
    const uint32_t p0 = tl.x;
    if (tl.y > n || tl.y <= p0) return;                          // (uniform; the plan never says so)
    const uint32_t size = tl.y - p0 < kMedianT ? tl.y - p0 : kMedianT;
    const uint32_t n_steps = tl.w < kMedianMaxSteps ? tl.w : kMedianMaxSteps;
    for (uint32_t s = tid; s < n_steps; s += kMedianBlock) steps[s] = tile_steps[tl.z + s];
    for (uint32_t p = tid; p < size; p += kMedianBlock) {
        uint32_t o = in[p0 + p].x & mask;
        o = o < n ? o : 0u;
        const uint2 c = cells[o];
        e_g01[p] = c.x; e_g2[p] = c.y & 0xFFFFu; e_obj[p] = o;
    }
    __syncthreads();
    for (uint32_t s0 = 0u; s0 < n_steps;) {
        const uint32_t level = steps[s0].x >> 16;
        uint32_t s1 = s0 + 1u;
        while (s1 < n_steps && (steps[s1].x >> 16) == level) ++s1;
        const uint32_t cnt = s1 - s0;
        for (uint32_t k = tid; k < 6u * cnt; k += kMedianBlock) bnd[k] = 0u;
        __syncthreads();
        // the step of each of this thread's positions: the last one of the level that starts at or before it, if it reaches it
        uint32_t mine[kMedianPer];
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e) {
            const uint32_t p = tid + e * kMedianBlock;
            mine[e] = 0xFFFFFFFFu;
            if (p < size && (steps[s0].x & 0xFFFFu) <= p) {
                uint32_t lo = s0, hi = s1;
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((steps[mid].x & 0xFFFFu) <= p) lo = mid; else hi = mid;
                }
                if (p < steps[lo].y && steps[lo].y <= size) {
                    mine[e] = lo - s0;
                    const uint32_t g01 = e_g01[p], g0 = g01 & 0xFFFFu, g1 = g01 >> 16, g2 = e_g2[p];
                    uint32_t* b = bnd + 6u * mine[e];
                    atomicMax(b, 65535u - g0); atomicMax(b + 1, 65535u - g1); atomicMax(b + 2, 65535u - g2);
                    atomicMax(b + 3, g0); atomicMax(b + 4, g1); atomicMax(b + 5, g2);
                }
            }
        }
        __syncthreads();
        for (uint32_t k = tid; k < cnt; k += kMedianBlock) {
            const uint32_t* b = bnd + 6u * k;
            axis_of[k] = median_axis(b[0], b[1], b[2], b[3], b[4], b[5], cell);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e) {
            const uint32_t p = tid + e * kMedianBlock;
            if (mine[e] != 0xFFFFFFFFu) {
                const uint32_t axis = axis_of[mine[e]], g01 = e_g01[p];
                const uint32_t v = axis == 0u ? g01 & 0xFFFFu : axis == 1u ? g01 >> 16 : e_g2[p];
                key[p] = ((unsigned long long)v << 32) | e_obj[p];
            }
        }
        __syncthreads();
        uint32_t to[kMedianPer], m_g01[kMedianPer], m_g2[kMedianPer], m_obj[kMedianPer];
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e) {
            const uint32_t p = tid + e * kMedianBlock;
            to[e] = 0xFFFFFFFFu; m_g01[e] = 0u; m_g2[e] = 0u; m_obj[e] = 0u;
            if (mine[e] != 0xFFFFFFFFu) {
                const uint2 st = steps[s0 + mine[e]];
                const uint32_t first = st.x & 0xFFFFu, last = st.y;
                const unsigned long long mk = key[p];
                uint32_t rank = 0u;
                for (uint32_t j = first; j < last; ++j) rank += key[j] < mk ? 1u : 0u;
                to[e] = first + rank;                            // < last: the position's own key is not below itself
                m_g01[e] = e_g01[p]; m_g2[e] = e_g2[p]; m_obj[e] = e_obj[p];
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t e = 0; e < kMedianPer; ++e)
            if (to[e] < size) { e_g01[to[e]] = m_g01[e]; e_g2[to[e]] = m_g2[e]; e_obj[to[e]] = m_obj[e]; }
        __syncthreads();
        s0 = s1;
    }
    for (uint32_t p = tid; p < size; p += kMedianBlock) out[p0 + p] = make_uint2(0u, e_obj[p]);
}
}  // namespace PTK_IMPL
namespace ptk {
uint32_t launch_bvh_median(const BvhMedianArgs& a, const BvhMedianLevel* levels, uint32_t n_levels, hipStream_t st) {
    const BvhBuildArgs& b = a.b;
    if (!b.n) return 0u;
    const dim3 grid((b.n + kBlock - 1) / kBlock), block(kBlock);
    const uint32_t mask = a.index_bits >= 32u ? 0xFFFFFFFFu : (1u << a.index_bits) - 1u;
    const PTK_IMPL::MedianCell cell = {{b.grid_cell[0], b.grid_cell[1], b.grid_cell[2]}};
    hipLaunchKernelGGL(PTK_IMPL::k_bvh_cells, grid, block, 0, st, b, a.cells);
    uint32_t cur = 0u;
    for (uint32_t l = 0; l < n_levels; ++l) {
        const BvhMedianLevel& lv = levels[l];
        const uint32_t* gs = a.group_start + lv.first;
        (void)hipMemsetAsync(a.bounds, 0, 6 * (size_t)lv.groups * sizeof(uint32_t), st);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_bounds, grid, block, 0, st, (const uint2*)b.pairs[cur], (const uint2*)a.cells, gs, lv.groups, a.bounds, b.n, mask);
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_keys, grid, block, 0, st, b.pairs[cur], (const uint2*)a.cells, gs, lv.groups, (const uint32_t*)a.bounds, cell, b.n,
                           a.index_bits, mask);
        cur = bvh_sort_passes(b, cur, (a.index_bits + 16u + lv.bits + 7u) / 8u, st);
    }
    hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_unpack, grid, block, 0, st, (const uint2*)b.pairs[cur], b.pairs[cur ^ 1u], b.n, mask);
    if (a.n_tiles)
        hipLaunchKernelGGL(PTK_IMPL::k_bvh_median_tile, dim3(a.n_tiles), dim3(PTK_IMPL::kMedianBlock), 0, st, (const uint2*)b.pairs[cur], b.pairs[cur ^ 1u],
                           (const uint2*)a.cells, a.tiles, a.tile_steps, cell, b.n, mask);
    return cur ^ 1u;
}
}  // namespace ptk
