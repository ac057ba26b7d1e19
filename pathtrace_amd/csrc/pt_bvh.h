// pt_bvh.h -- optional acceleration structure for World::hit_scene (the reference
// itself is linear-scan only, world.rs:281).  A 4-wide BVH over the objects' f32 bounding boxes (a binned-SAH
// binary tree, collapsed), built on the host at first use.  It only decides WHICH primitives a ray is tested against; the
// primitive tests are the ones of the linear scan, and the winner is chosen by the rule the scan
// implies (smallest t; among equal t the highest object index), so the answer does not depend on
// the traversal order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace ptbvh {

// Child code of a node: bit 31 clear = index of an internal node; bit 31 set = leaf with
// ((code >> 28) & 7) + 1 primitives starting at slot (code & 0x0FFFFFFF) of the leaf arrays.
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kDone = 0xFFFFFFFFu;      // stack sentinel / root of an empty scene (no leaf code: a leaf holds <= 4 primitives)
constexpr uint32_t kMaxLeaf = 4;             // primitives per leaf
constexpr uint32_t kWidth = 4;               // children per internal node
#ifndef PT_BVH_STACK
#define PT_BVH_STACK 24
#endif
constexpr uint32_t kStackDepth = PT_BVH_STACK;         // traversal stack entries per lane (LDS); the builder keeps the tree's stack need within it (<= 16 M objects)
constexpr uint32_t kTriangleBit = 0x80000000u;   // in leaf_ids: the primitive is a triangle

// Internal node as the builder and the checker see it: up to kWidth children, each with the f32 box of its subtree.
// Unused child slots carry the code kDone (the traversal never enters them).
struct WideNode {
    float lo[kWidth][3], hi[kWidth][3];
    uint32_t code[kWidth];
    uint32_t n;                       // children in use (2 .. kWidth), slots [0, n)
};

struct Built {
    std::vector<WideNode> wide;
    // What the device traverses: the same nodes with the child boxes on a 16-bit grid over the scene's bounds, 64 bytes
    // (one cache line, four 16-byte loads) per visit.  Round 2's binary nodes took two dependent 32-byte visits for what
    // one visit decides here; the traversal is bound by the latency of those dependent fetches.
    //   child c = three words  w0 = lo.x | lo.y << 16, w1 = lo.z | hi.x << 16, w2 = hi.y | hi.z << 16
    //   qnodes[4k]   = (c0.w0, c0.w1, c0.w2, c1.w0)    qnodes[4k+1] = (c1.w1, c1.w2, c2.w0, c2.w1)
    //   qnodes[4k+2] = (c2.w2, c3.w0, c3.w1, c3.w2)    qnodes[4k+3] = (code0, code1, code2, code3)
    // coordinate = grid_min[axis] + q * grid_cell[axis], evaluated as fmaf((float)q, cell, min); lower planes are
    // rounded down and upper planes up until that f32 expression encloses the f32 box, so a quantised box contains
    // the exact one (it only prunes less).
    std::vector<uint4> qnodes;
    float grid_min[3] = {0.f, 0.f, 0.f}, grid_cell[3] = {0.f, 0.f, 0.f};
    // Leaf slots.  Every leaf starts at a slot index that is a multiple of 4 (unused slots: id kDone), so the <= 4 ids of
    // a leaf are one aligned 16-byte load and its <= 4 lead records one 64-byte line.
    std::vector<float4> leaf_rec;     // 3 float4 per leaf slot: sphere (c, r^2), -, - ; triangle: triangle_scan_record (the scan records)
    std::vector<float4> leaf_lead;    // 1 float4 per leaf slot = leaf_rec[3 * slot]: all a sphere test reads (a triangle reads the other two from leaf_rec)
    std::vector<uint32_t> leaf_ids;   // object index of the leaf slot (| kTriangleBit)
    uint32_t leaf_prims = 0;          // slots that hold a primitive (= number of objects)
    uint32_t root = kDone;            // child code of the root
    uint32_t depth = 0;               // deepest leaf of the BINARY tree the nodes were collapsed from (root = 0)
    // Stack entries a traversal can need: 1 (sentinel) + the largest sum over a root-to-leaf path of (children - 1): a
    // visit pushes every hit child but the one it descends into.  The collapse keeps it <= kStackDepth (it merges a
    // binary node's grandchildren into the node only where the remaining budget still covers the subtrees below).
    uint32_t stack_need = 1;
    float scene_abs = 0.0f;           // sum over axes of the largest |coordinate| of any box: scale of the traversal padding
    // Objects with a NaN/inf coordinate or radius.  The linear scan's answer for such an object depends on the
    // scan order (a NaN t is "accepted" and then lets every later hit through, world.rs:281-287), which no
    // traversal order reproduces: callers refuse accel = 1 for such scenes.
    uint32_t non_finite = 0;
    // For ptbvh::refit and the device-side refit (pt_scene_refit), which keep the topology.  Height of a wide node: 0 = all its
    // children are leaves, otherwise 1 + the largest height of a child node.  A node's boxes depend only on nodes of lower
    // height, so the nodes of one height can be refitted together once the lower heights are done.
    std::vector<uint32_t> node_height;    // per wide node
    std::vector<uint32_t> height_order;   // the node indices ordered by height, ties by index
    std::vector<uint32_t> height_first;   // height h = positions [height_first[h], height_first[h + 1]) of height_order (last entry: the node count)
    // Cost of the tree as the device traverses it: over every used child slot of every node the half-area of the quantised
    // child box, as three exact integer sums in grid units, d = q_hi - q_lo per axis: sum dx dy, sum dy dz, sum dz dx.
    // cost = s[0] cell.x cell.y + s[1] cell.y cell.z + s[2] cell.z cell.x.
    uint64_t cost[3] = {0, 0, 0};
};
// the cost in scene units from the three sums and the grid they were counted in
inline double cost_value(const uint64_t s[3], const float cell[3]) {
    return (double)s[0] * ((double)cell[0] * cell[1]) + (double)s[1] * ((double)cell[1] * cell[2]) + (double)s[2] * ((double)cell[2] * cell[0]);
}

// The f32 box of one primitive from its gather records, rounded outward: a sphere as the ball of radius sqrt(fl(r * r)) (what
// the scan tests against) widened by 1e-7, a triangle as the min / max of its corners v0, v0 + e1, v0 + e2.  Returns false, and
// a box that covers everything, when a coordinate is NaN or inf (Built::non_finite counts those objects).
bool primitive_box(const float4& r0, const float4& r1, const float4& r2, bool triangle, float lo[3], float hi[3]);
// What the scene's boxes decide besides the tree: the quantisation grid (over the bounds of all boxes; left zero when the
// tree has no node, has_nodes = false), scene_abs and the count of non-finite objects -- one pass over the objects.
struct Bounds {
    float grid_min[3] = {0.f, 0.f, 0.f}, grid_cell[3] = {0.f, 0.f, 0.f};
    float scene_abs = 0.0f;
    uint32_t non_finite = 0;
};
Bounds scene_bounds(const float4* shape, const uint32_t* shape_tag, uint32_t n, bool has_nodes);

// Scan record of a triangle (what the primitive test reads; pt_kernels_scan.h triangle_test): the f32 specification of
// TriangleShape::hit (shape.rs:161-192) works on the triangle's plane and two barycentric gradients instead of
// re-deriving them per ray from the edges as Moeller-Trumbore does -- same real-number u, v, t:
//     n  = e1 x e2                 t = -(s.n) / (d.n),  s = o - v0      (a = e1.(d x e2) = -(d.n), t = f e2.(s x e1) = f s.n)
//     N1 = (e2 x n) / (n.n)        u = (s + t d) . N1                    (N1.e1 = 1, N1.e2 = 0, N1.n = 0)
//     N2 = (n x e1) / (n.n)        v = (s + t d) . N2                    (N2.e2 = 1, N2.e1 = 0, N2.n = 0)
// computed in f64 from the f32 edges and rounded to f32 (the oracle's float instantiation does the same, bit for bit).
// Packing, 3 float4, in the order the test reads them -- one aligned 16-byte read per stage (round 5; rounds 3-4 packed v0 first
// and the compiler read the normal as two 8-byte halves of two float4): (n.x, n.y, n.z, N1.x) (v0.x, v0.y, v0.z, N1.y)
// (N1.z, N2.x, N2.y, N2.z).
__host__ __device__ inline void triangle_scan_record(const float4& v0, const float4& e1f, const float4& e2f, float4 out[3]) {
    const double e1[3] = {e1f.x, e1f.y, e1f.z}, e2[3] = {e2f.x, e2f.y, e2f.z};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double a[3] = {e2[1] * n[2] - e2[2] * n[1], e2[2] * n[0] - e2[0] * n[2], e2[0] * n[1] - e2[1] * n[0]};   // e2 x n
    const double b[3] = {n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]};   // n x e1
    out[0] = make_float4((float)n[0], (float)n[1], (float)n[2], (float)(a[0] / nn));
    out[1] = make_float4(v0.x, v0.y, v0.z, (float)(a[1] / nn));
    out[2] = make_float4((float)(a[2] / nn), (float)(b[0] / nn), (float)(b[1] / nn), (float)(b[2] / nn));
}

// shape: 3 float4 per object in the gather form of pt_device.h (sphere: (c, r), (1/r,..), -; triangle: v0, e1, e2);
// scan_w: for spheres the r^2 the scan record carries.  Throws nothing; n may be 0.
Built build(const float4* shape, const uint32_t* shape_tag, uint32_t n);

// The tree of build() carried to a new pose of the same objects (same n, same shape tags): topology, child codes and
// leaf_ids stay.  Recomputed: leaf_rec and leaf_lead from the new records as build() writes them; every wide node's child
// boxes bottom-up (a leaf child: the union of its primitives' boxes; a node child: the union of that node's child boxes);
// grid_min / grid_cell by build()'s rule over the new boxes; qnodes, cost, scene_abs and non_finite.  Refitting to the pose
// the tree was built from returns build()'s arrays bit for bit.  The tree stays CORRECT however far the objects moved (every
// box encloses what is beneath it); only its quality -- cost -- degrades.  This function is the specification of the
// device-side refit (k_bvh_refit_leaves, k_bvh_refit_level).
void refit(Built& t, const float4* shape, const uint32_t* shape_tag, uint32_t n);

// ---- the Morton build (pt_scene_rebuild): a tree whose TOPOLOGY is a pure function of the object count, so
// that a build is "order the objects along a Morton curve, write leaf_ids, refit".
//
// Leaves: L = ceil(n / 4); leaf j is the slots [4j, 4j + 4) and holds the sorted positions 4j .. min(4j + 4, n) - 1 (padding
// slots: kDone).  n = 0: no slot, root = kDone; L = 1: root = that leaf's code, no node -- what build() makes of such scenes.
// Nodes: a node over the leaf range [b, e), m = e - b >= 2, with stack budget B (the root: kStackDepth - 1) has `a` children,
// a = the largest of 4, 3, 2 with a <= m and (a - 1) + ceil(log2(ceil(m / a))) <= B (what is left covers an all-binary subtree
// over the largest child); child i is the range [b + floor(i m / a), b + floor((i + 1) m / a)): one leaf = that leaf's code,
// more = a node with budget B - (a - 1).  Unused child slots carry kDone, a node is numbered before the nodes beneath it.
struct Topology {
    bool ok = true;                       // false: no arity fits at the root (L > 2^(kStackDepth - 1)); nothing else is filled in
    std::vector<uint32_t> codes;          // kWidth child codes per node
    std::vector<uint32_t> node_height, height_order, height_first;   // as in Built
    uint32_t root = kDone;
    uint32_t n_slots = 0;                 // 4 L
    uint32_t stack_need = 1;
    uint32_t depth = 0;                   // deepest leaf in binary levels: a node of 2 children counts 1 level, of 3 or 4 counts 2
};
Topology morton_topology(uint32_t n);

// The grid coordinate of a box on axis k: the cell of its centre, g = floor((((double)lo[k] + (double)hi[k]) * 0.5 -
// (double)grid_min[k]) / (double)grid_cell[k]) in f64 without contraction, clamped to [0, 65535].
__host__ __device__ inline uint32_t grid_coord(const float lo[3], const float hi[3], const float grid_min[3], const float grid_cell[3], int k) {
#pragma clang fp contract(off)
    double g = __builtin_floor((((double)lo[k] + (double)hi[k]) * 0.5 - (double)grid_min[k]) / (double)grid_cell[k]);
    g = !(g >= 0.0) ? 0.0 : g > 65535.0 ? 65535.0 : g;
    return (uint32_t)g;
}
// The 30-bit Morton key of a box on the grid: per axis k, c_k = grid_coord >> 6 (10 bits); bit 3 j + k of the key is bit j of
// c_k.  k_bvh_morton evaluates the same expression on the device.
__host__ __device__ inline uint32_t morton_key(const float lo[3], const float hi[3], const float grid_min[3], const float grid_cell[3]) {
    uint32_t key = 0u;
    for (int k = 0; k < 3; ++k) {
        const uint32_t c = grid_coord(lo, hi, grid_min, grid_cell, k) >> 6;
        for (int j = 0; j < 10; ++j) key |= ((c >> j) & 1u) << (3 * j + k);
    }
    return key;
}

// The tree of the pose: boxes by primitive_box, grid by scene_bounds(.., has_nodes = L > 1), keys by morton_key (all 0 when
// there is no node, hence no grid), objects ordered ascending by (key, object index), leaf_ids from that order, the topology of
// morton_topology(n), and everything else -- leaf records, child boxes, qnodes, cost, scene_abs, non_finite -- by refit().
// keys / order (optional): the key of every object and the sorted object indices.  Returns false, and an empty tree, when
// morton_topology(n) has no plan.  With a non-finite object the tree is formed all the same (non_finite > 0; callers refuse it).
bool build_morton(Built& out, const float4* shape, const uint32_t* shape_tag, uint32_t n, std::vector<uint32_t>* keys = nullptr,
                  std::vector<uint32_t>* order = nullptr);

// ---- the median build (pt_scene_rebuild_ordered, PT_BVH_ORDER_MEDIAN): the Morton build with another order.  The
// topology, the leaves and the refit are those above; the objects reach their positions by a recursive median split along the
// nodes' child boundaries instead of a sort along a curve, so that a node's children are boxes side by side.
//
// The split plan is a pure function of n.  A node over the leaf range [b, e) has the child leaf boundaries c_0 = b < .. < c_a = e.
// split(c_lo .. c_hi) over more than one child is one step: its positions are [P, Q) = [min(4 c_lo, n), min(4 c_hi, n)), its cut
// is the boundary c_mid, mid = lo + ceil((hi - lo) / 2), at position min(4 c_mid, n); then split(c_lo .. c_mid) and
// split(c_mid .. c_hi) one level down.  A split over a single child that is a node runs that node's split (at the level it has
// reached); a single leaf ends the recursion.
// A step: per axis the minimum and maximum of grid_coord over the objects now at [P, Q); the axis is the k with the largest
// (double)(gmax_k - gmin_k) * (double)grid_cell[k], ties to the lowest k; [P, Q) is reordered ascending by (g_axis, object
// index).  Steps run parent before child, from the index order (position p = object p).
constexpr uint32_t kMedianTile = 2048;       // T: a step over at most T positions, and every step beneath it, is one workgroup's work in LDS
constexpr uint32_t kMedianChunk = 65536;     // positions of a level that no step above T covers are cut into groups of at most this many
struct MedianStep { uint32_t level, P, Q, cut; };
struct MedianPlan {
    bool ok = true;                          // false: morton_topology(n) has no plan
    std::vector<MedianStep> steps;           // ascending by (level, P)
    // What the device walks (pt_kernels.h, launch_bvh_median).  Steps over more than T positions run level by level over the whole
    // array: a level's positions fall into groups in position order, a step or a stretch of at most kMedianChunk positions
    // that no step of the level covers.  group_start holds, level after level, the groups' first positions (bit 31: a step) and
    // one closing entry n.  The highest steps of at most T positions are the tiles: (P, Q, first, count) with the tile's own
    // step and every step beneath it at tile_steps[first, first + count) as (P - tile P | local level << 16, Q - tile P),
    // ascending by (level, P).
    struct Level { uint32_t first, groups, bits; };   // group_start[first, first + groups]; bits to number the groups
    std::vector<Level> levels;
    std::vector<uint32_t> group_start;
    std::vector<uint4> tiles;
    std::vector<uint2> tile_steps;
    uint32_t index_bits = 0;                 // bits to hold an object index < n
    uint32_t max_groups = 0;
};
MedianPlan median_plan(uint32_t n);

// build_morton with the order of the rule above.  g (optional): grid_coord of every object, 3 per object (all 0 without a
// node); order (optional): the object at every position.
bool build_median(Built& out, const float4* shape, const uint32_t* shape_tag, uint32_t n, std::vector<uint32_t>* g = nullptr,
                  std::vector<uint32_t>* order = nullptr);

}  // namespace ptbvh
