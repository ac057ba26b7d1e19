// pt_bvh.cpp -- host-side BVH builder (see pt_bvh.h).  A binary tree first -- binned SAH near the root, object-median
// splits wherever SAH could make the tree deeper than the traversal stack --, then collapsed into nodes of up to four
// children wherever the stack budget allows.
#include "pt_bvh.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace ptbvh {
namespace {

struct Box {
    float lo[3], hi[3];
    void reset() { for (int k = 0; k < 3; ++k) { lo[k] = std::numeric_limits<float>::infinity(); hi[k] = -lo[k]; } }
    void grow(const Box& b) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]); } }
    double half_area() const {
        double e[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};
        if (e[0] < 0 || e[1] < 0 || e[2] < 0) return 0.0;
        return e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
    }
};

float down(double v) { float f = (float)v; return (double)f > v ? std::nextafterf(f, -std::numeric_limits<float>::infinity()) : f; }
float up(double v) { float f = (float)v; return (double)f < v ? std::nextafterf(f, std::numeric_limits<float>::infinity()) : f; }

// Leaf records of object o as the scan reads them: sphere (c, r^2), -, - ; triangle: triangle_scan_record
void leaf_records(const float4* shape, bool tri, uint32_t o, float4 out[3]) {
    float4 r0 = shape[3 * (size_t)o], r1 = shape[3 * (size_t)o + 1], r2 = shape[3 * (size_t)o + 2];
    if (!tri) { r0.w = r0.w * r0.w; r1 = make_float4(0, 0, 0, 0); r2 = r1; }   // (c, r^2): the scan record of a sphere
    else { float4 t[3]; triangle_scan_record(r0, r1, r2, t); r0 = t[0]; r1 = t[1]; r2 = t[2]; }
    out[0] = r0; out[1] = r1; out[2] = r2;
}

struct Prim {
    Box box;
    float cen[3];
    uint32_t obj;
};

// primitives a leaf is filled to (<= kMaxLeaf, what the traversal unrolls for); measurement knob
#ifndef PT_BVH_LEAF_TARGET
#define PT_BVH_LEAF_TARGET 4
#endif
constexpr uint32_t kLeafTarget = PT_BVH_LEAF_TARGET;
static_assert(kLeafTarget >= 1 && kLeafTarget <= kMaxLeaf, "leaf size");
// levels an object-median subtree of m primitives needs below its root
uint32_t median_levels(uint64_t m) {
    uint32_t l = 0;
    while (m > kLeafTarget) { m = (m + 1) / 2; ++l; }
    return l;
}

constexpr uint32_t kMaxDepth = kStackDepth - 2;   // deepest leaf the traversal stack (sentinel + one push per level) can take
constexpr int kBins = 16;

// node of the binary tree (temporary): child = leaf code, or index into Builder::bin
struct BinNode {
    Box box[2];
    uint32_t child[2];
    uint32_t height;          // levels of internal nodes below and including this one on its deepest path (a node of two leaves: 1)
};

struct Builder {
    std::vector<Prim> prims;
    std::vector<BinNode> bin;
    const float4* shape;
    const uint32_t* tag;
    Built out;

    uint32_t make_leaf(uint32_t first, uint32_t count, uint32_t depth) {
        while (out.leaf_ids.size() % 4u != 0u) {                 // leaves start at multiples of 4 slots
            out.leaf_ids.push_back(kDone);
            out.leaf_lead.push_back(make_float4(0, 0, 0, 0));
            for (int k = 0; k < 3; ++k) out.leaf_rec.push_back(make_float4(0, 0, 0, 0));
        }
        const uint32_t slot = (uint32_t)out.leaf_ids.size();
        // object order inside a leaf (not needed for correctness, keeps the tests in scan order)
        std::sort(prims.begin() + first, prims.begin() + first + count, [](const Prim& a, const Prim& b) { return a.obj < b.obj; });
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t o = prims[first + i].obj;
            const bool tri = tag[o] != 0;
            out.leaf_ids.push_back(o | (tri ? kTriangleBit : 0u));
            float4 r[3];
            leaf_records(shape, tri, o, r);
            out.leaf_rec.push_back(r[0]); out.leaf_rec.push_back(r[1]); out.leaf_rec.push_back(r[2]);
            out.leaf_lead.push_back(r[0]);
            out.leaf_prims++;
        }
        out.depth = std::max(out.depth, depth);
        return kLeafBit | ((count - 1u) << 28) | slot;
    }

    // returns the child code of the subtree over prims[first, first+count)
    uint32_t build(uint32_t first, uint32_t count, uint32_t depth, Box* box_out) {
        Box box; box.reset();
        Box cb; cb.reset();
        for (uint32_t i = first; i < first + count; ++i) {
            box.grow(prims[i].box);
            for (int k = 0; k < 3; ++k) { cb.lo[k] = std::min(cb.lo[k], prims[i].cen[k]); cb.hi[k] = std::max(cb.hi[k], prims[i].cen[k]); }
        }
        *box_out = box;
        if (count <= kLeafTarget) return make_leaf(first, count, depth);

        uint32_t mid = 0;
        bool split = false;
        if (depth + 1u + median_levels(count - 1u) <= kMaxDepth) {   // SAH may be arbitrarily unbalanced: only while that is safe
            double best = std::numeric_limits<double>::infinity();
            int best_axis = -1, best_bin = -1;
            for (int ax = 0; ax < 3; ++ax) {
                const double lo = cb.lo[ax], ext = (double)cb.hi[ax] - lo;
                if (!(ext > 0.0)) continue;
                Box bb[kBins]; uint32_t bn[kBins];
                for (int b = 0; b < kBins; ++b) { bb[b].reset(); bn[b] = 0; }
                for (uint32_t i = first; i < first + count; ++i) {
                    int b = (int)(((double)prims[i].cen[ax] - lo) / ext * kBins);
                    b = std::min(std::max(b, 0), kBins - 1);
                    bb[b].grow(prims[i].box); bn[b]++;
                }
                double right_area[kBins]; uint32_t right_n[kBins];
                Box acc; acc.reset(); uint32_t n = 0;
                for (int b = kBins - 1; b > 0; --b) { acc.grow(bb[b]); n += bn[b]; right_area[b] = acc.half_area(); right_n[b] = n; }
                acc.reset(); n = 0;
                for (int b = 0; b + 1 < kBins; ++b) {
                    acc.grow(bb[b]); n += bn[b];
                    if (n == 0 || right_n[b + 1] == 0) continue;
                    const double cost = acc.half_area() * n + right_area[b + 1] * right_n[b + 1];
                    if (cost < best) { best = cost; best_axis = ax; best_bin = b; }
                }
            }
            if (best_axis >= 0) {
                const double lo = cb.lo[best_axis], ext = (double)cb.hi[best_axis] - lo;
                auto it = std::partition(prims.begin() + first, prims.begin() + first + count, [&](const Prim& p) {
                    int b = (int)(((double)p.cen[best_axis] - lo) / ext * kBins);
                    b = std::min(std::max(b, 0), kBins - 1);
                    return b <= best_bin;
                });
                mid = (uint32_t)(it - prims.begin());
                split = mid > first && mid < first + count;
            }
        }
        if (!split) {   // object median along the widest centroid axis (or any axis when all centroids coincide)
            int ax = 0;
            double e = -1.0;
            for (int k = 0; k < 3; ++k) { const double x = (double)cb.hi[k] - cb.lo[k]; if (x > e) { e = x; ax = k; } }
            mid = first + (count + 1u) / 2u;
            std::nth_element(prims.begin() + first, prims.begin() + mid, prims.begin() + first + count,
                             [ax](const Prim& a, const Prim& b) { return a.cen[ax] < b.cen[ax] || (a.cen[ax] == b.cen[ax] && a.obj < b.obj); });
        }
        const uint32_t node = (uint32_t)bin.size();
        bin.emplace_back();
        Box b0, b1;
        const uint32_t c0 = build(first, mid - first, depth + 1, &b0);
        const uint32_t c1 = build(mid, first + count - mid, depth + 1, &b1);
        BinNode& bn = bin[node];
        bn.box[0] = b0; bn.box[1] = b1;
        bn.child[0] = c0; bn.child[1] = c1;
        bn.height = 1u + std::max(height_of(c0), height_of(c1));
        return node;
    }
    uint32_t height_of(uint32_t code) const { return (code & kLeafBit) ? 0u : bin[code].height; }

    // Binary subtree `b` -> wide node; returns its index.  budget = stack entries the traversal may use below this
    // node's parent (need of the subtree <= budget).  A binary subtree of height h needs h entries as it is (one push per
    // level); pulling a grandchild pair up into the node costs one more entry for EVERY path through the node, so it is
    // done (largest box first) only while every child's binary height still fits what is left.
    uint32_t collapse(uint32_t b, uint32_t budget, uint32_t* need_out) {
        struct Item { Box box; uint32_t code; };
        Item it[kWidth];
        uint32_t c = 2;
        it[0] = {bin[b].box[0], bin[b].child[0]};
        it[1] = {bin[b].box[1], bin[b].child[1]};
        while (c < kWidth) {
            int best = -1;
            double best_area = -1.0;
            for (uint32_t k = 0; k < c; ++k) {
                if (it[k].code & kLeafBit) continue;
                // after opening child k the node has c + 1 children: every child subtree must fit budget - c
                bool ok = true;
                for (uint32_t j = 0; j < c && ok; ++j)
                    if (j != k) ok = height_of(it[j].code) + c <= budget;
                const BinNode& g = bin[it[k].code];
                ok = ok && height_of(g.child[0]) + c <= budget && height_of(g.child[1]) + c <= budget;
                if (!ok) continue;
                const double a = it[k].box.half_area();
                if (a > best_area) { best_area = a; best = (int)k; }
            }
            if (best < 0) break;
            const BinNode& g = bin[it[best].code];
            it[best] = {g.box[0], g.child[0]};
            it[c++] = {g.box[1], g.child[1]};
        }
        const uint32_t w = (uint32_t)out.wide.size();
        out.wide.emplace_back();
        uint32_t need_below = 0;
        for (uint32_t k = 0; k < kWidth; ++k) {
            uint32_t code = kDone;
            Box bx; bx.reset();
            if (k < c) {
                bx = it[k].box;
                code = it[k].code;
                if (!(code & kLeafBit)) {
                    uint32_t nd = 0;
                    code = collapse(code, budget - (c - 1u), &nd);
                    need_below = std::max(need_below, nd);
                }
            }
            WideNode& wn = out.wide[w];
            for (int a = 0; a < 3; ++a) { wn.lo[k][a] = bx.lo[a]; wn.hi[k][a] = bx.hi[a]; }
            wn.code[k] = code;
        }
        out.wide[w].n = c;
        *need_out = (c - 1u) + need_below;
        return w;
    }
};

// The grid over the bounds lo .. hi of all boxes (see pt_bvh.h)
void grid_over(const double lo[3], const double hi[3], float grid_min[3], float grid_cell[3]) {
    for (int a = 0; a < 3; ++a) {
        grid_min[a] = down(lo[a]);
        const double ext = std::max(hi[a] - (double)grid_min[a], 1e-30);
        grid_cell[a] = up(ext / 65535.0 * (1.0 + 1e-6));          // 65535 cells reach past the upper bound
    }
}

// Child boxes -> 16-bit grid coordinates over the bounds of all child boxes (see pt_bvh.h), and the cost sums of the result.
void quantise(Built& t) {
    const size_t n_nodes = t.wide.size();
    t.qnodes.assign(4 * n_nodes, make_uint4(0, 0, 0, 0));
    t.cost[0] = t.cost[1] = t.cost[2] = 0;
    if (n_nodes == 0) return;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (const WideNode& w : t.wide)
        for (uint32_t c = 0; c < w.n; ++c)
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)w.lo[c][a]); hi[a] = std::max(hi[a], (double)w.hi[c][a]); }
    grid_over(lo, hi, t.grid_min, t.grid_cell);
    auto decode = [&](int a, uint32_t q) { return std::fmaf((float)q, t.grid_cell[a], t.grid_min[a]); };
    auto q_lo = [&](int a, float v) {
        long q = (long)std::floor(((double)v - t.grid_min[a]) / t.grid_cell[a]);
        q = std::min(std::max(q, 0L), 65535L);
        while (q > 0 && decode(a, (uint32_t)q) > v) --q;
        return (uint32_t)q;
    };
    auto q_hi = [&](int a, float v) {
        long q = (long)std::ceil(((double)v - t.grid_min[a]) / t.grid_cell[a]);
        q = std::min(std::max(q, 0L), 65535L);
        while (q < 65535 && decode(a, (uint32_t)q) < v) ++q;
        return (uint32_t)q;
    };
    for (size_t k = 0; k < n_nodes; ++k) {
        const WideNode& w = t.wide[k];
        uint32_t v[kWidth][3];
        for (uint32_t c = 0; c < kWidth; ++c) {
            if (c >= w.n) { v[c][0] = v[c][1] = v[c][2] = 0u; continue; }      // unused slot: its code (kDone) keeps the traversal out
            const uint32_t lx = q_lo(0, w.lo[c][0]), ly = q_lo(1, w.lo[c][1]), lz = q_lo(2, w.lo[c][2]);
            const uint32_t hx = q_hi(0, w.hi[c][0]), hy = q_hi(1, w.hi[c][1]), hz = q_hi(2, w.hi[c][2]);
            v[c][0] = lx | (ly << 16); v[c][1] = lz | (hx << 16); v[c][2] = hy | (hz << 16);
            const uint64_t dx = hx - lx, dy = hy - ly, dz = hz - lz;          // (uint32 differences: hi >= lo for a box that is not inverted)
            t.cost[0] += dx * dy; t.cost[1] += dy * dz; t.cost[2] += dz * dx;
        }
        t.qnodes[4 * k] = make_uint4(v[0][0], v[0][1], v[0][2], v[1][0]);
        t.qnodes[4 * k + 1] = make_uint4(v[1][1], v[1][2], v[2][0], v[2][1]);
        t.qnodes[4 * k + 2] = make_uint4(v[2][2], v[3][0], v[3][1], v[3][2]);
        t.qnodes[4 * k + 3] = make_uint4(w.code[0], w.code[1], w.code[2], w.code[3]);
    }
}

// Heights of the wide nodes and their order by height (pt_bvh.h).  collapse() numbers a node before the nodes beneath it, so
// one pass from the last node to the first sees every child node before its parent.
void order_by_height(Built& t) {
    const size_t n_nodes = t.wide.size();
    t.node_height.assign(n_nodes, 0u);
    uint32_t top = 0;
    for (size_t k = n_nodes; k-- > 0;) {
        uint32_t h = 0;
        for (uint32_t c = 0; c < t.wide[k].n; ++c) {
            const uint32_t code = t.wide[k].code[c];
            if (!(code & kLeafBit)) h = std::max(h, 1u + t.node_height[code]);
        }
        t.node_height[k] = h;
        top = std::max(top, h);
    }
    t.height_first.assign(n_nodes ? top + 2u : 1u, 0u);
    for (size_t k = 0; k < n_nodes; ++k) t.height_first[t.node_height[k] + 1u]++;
    for (size_t h = 1; h < t.height_first.size(); ++h) t.height_first[h] += t.height_first[h - 1];
    t.height_order.assign(n_nodes, 0u);
    std::vector<uint32_t> at(t.height_first.begin(), t.height_first.end());
    for (size_t k = 0; k < n_nodes; ++k) t.height_order[at[t.node_height[k]]++] = (uint32_t)k;
}

// largest |coordinate| per axis over the finite boxes -> scene_abs
struct AbsMax {
    double a[3] = {0, 0, 0};
    void add(const float lo[3], const float hi[3]) {
        for (int k = 0; k < 3; ++k) a[k] = std::max(a[k], std::max(std::fabs((double)lo[k]), std::fabs((double)hi[k])));
    }
    float scene_abs() const { return up(a[0] + a[1] + a[2]); }
};

}  // namespace

Built build(const float4* shape, const uint32_t* shape_tag, uint32_t n) {
    Builder b;
    b.shape = shape; b.tag = shape_tag;
    b.prims.resize(n);
    AbsMax amax;
    for (uint32_t i = 0; i < n; ++i) {
        Prim& p = b.prims[i];
        p.obj = i;
        const bool finite = primitive_box(shape[3 * (size_t)i], shape[3 * (size_t)i + 1], shape[3 * (size_t)i + 2], shape_tag[i] != 0, p.box.lo, p.box.hi);
        if (!finite) b.out.non_finite++;
        else amax.add(p.box.lo, p.box.hi);
        for (int k = 0; k < 3; ++k) p.cen[k] = finite ? (float)(0.5 * ((double)p.box.lo[k] + p.box.hi[k])) : 0.f;
    }
    b.bin.reserve(n);
    b.out.leaf_ids.reserve(n);
    b.out.leaf_rec.reserve(3 * (size_t)n);
    if (n != 0) {
        Box root;
        uint32_t r = b.build(0, n, 0, &root);
        if (!(r & kLeafBit)) {
            // the binary tree is at most kMaxDepth deep: as it stands it fits the budget, and the collapse never breaks that
            uint32_t need = 0;
            r = b.collapse(r, kStackDepth - 2u, &need);
            b.out.stack_need = 1u + need;
        }
        b.out.root = r;
    }
    b.out.scene_abs = amax.scene_abs();
    while (b.out.leaf_ids.size() % 4u != 0u) {                   // the last leaf's 16-byte id load stays in bounds
        b.out.leaf_ids.push_back(kDone);
        b.out.leaf_lead.push_back(make_float4(0, 0, 0, 0));
        for (int k = 0; k < 3; ++k) b.out.leaf_rec.push_back(make_float4(0, 0, 0, 0));
    }
    quantise(b.out);
    order_by_height(b.out);
    return std::move(b.out);
}

bool primitive_box(const float4& r0, const float4& r1, const float4& r2, bool triangle, float lo[3], float hi[3]) {
    if (!triangle) {
        // the scan tests against r2 = fl(r*r); bound the sphere of radius sqrt(r2), rounded outward
        const float r2f = r0.w * r0.w;
        const double r = std::sqrt((double)r2f) * (1.0 + 1e-7);
        const double c[3] = {r0.x, r0.y, r0.z};
        for (int k = 0; k < 3; ++k) { lo[k] = down(c[k] - r); hi[k] = up(c[k] + r); }
    } else {
        const double v0[3] = {r0.x, r0.y, r0.z}, e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
        for (int k = 0; k < 3; ++k) {
            const double a = v0[k], bq = v0[k] + e1[k], c = v0[k] + e2[k];
            lo[k] = down(std::min(a, std::min(bq, c)));
            hi[k] = up(std::max(a, std::max(bq, c)));
        }
    }
    bool finite = true;
    for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(lo[k]) && std::isfinite(hi[k]);
    // a non-finite box would poison every ancestor: make it cover everything (the caller refuses the scene anyway)
    if (!finite)
        for (int k = 0; k < 3; ++k) { lo[k] = -std::numeric_limits<float>::max(); hi[k] = std::numeric_limits<float>::max(); }
    return finite;
}

Bounds scene_bounds(const float4* shape, const uint32_t* shape_tag, uint32_t n, bool has_nodes) {
    Bounds out;
    AbsMax amax;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t i = 0; i < n; ++i) {
        float bl[3], bh[3];
        if (!primitive_box(shape[3 * (size_t)i], shape[3 * (size_t)i + 1], shape[3 * (size_t)i + 2], shape_tag[i] != 0, bl, bh)) out.non_finite++;
        else amax.add(bl, bh);
        // every primitive lies beneath some child box, and a box is the union of what is beneath it: the bounds of all child
        // boxes (quantise) are the bounds of all primitive boxes
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (double)bl[a]); hi[a] = std::max(hi[a], (double)bh[a]); }
    }
    out.scene_abs = amax.scene_abs();
    if (has_nodes && n != 0) grid_over(lo, hi, out.grid_min, out.grid_cell);
    return out;
}

void refit(Built& t, const float4* shape, const uint32_t* shape_tag, uint32_t n) {
    const size_t n_slots = t.leaf_ids.size(), n_nodes = t.wide.size();
    std::vector<Box> slot_box(n_slots), node_box(n_nodes);
    AbsMax amax;
    t.non_finite = 0;
    for (size_t i = 0; i < n_slots; ++i) {
        const uint32_t w = t.leaf_ids[i];
        if (w == kDone) continue;                                // padding slot: zero records, as build() left them
        const uint32_t o = w & ~kTriangleBit;
        if (o >= n) continue;
        const bool tri = shape_tag[o] != 0;
        float4 r[3];
        leaf_records(shape, tri, o, r);
        t.leaf_rec[3 * i] = r[0]; t.leaf_rec[3 * i + 1] = r[1]; t.leaf_rec[3 * i + 2] = r[2];
        t.leaf_lead[i] = r[0];
        if (!primitive_box(shape[3 * (size_t)o], shape[3 * (size_t)o + 1], shape[3 * (size_t)o + 2], tri, slot_box[i].lo, slot_box[i].hi)) t.non_finite++;
        else amax.add(slot_box[i].lo, slot_box[i].hi);
    }
    t.scene_abs = amax.scene_abs();
    for (const uint32_t k : t.height_order) {                    // bottom-up: the child nodes of k come earlier in the order
        WideNode& wn = t.wide[k];
        node_box[k].reset();
        for (uint32_t c = 0; c < wn.n; ++c) {
            Box b; b.reset();
            const uint32_t code = wn.code[c];
            if (code & kLeafBit) {
                const uint32_t first = code & 0x0FFFFFFFu, cnt = ((code >> 28) & 7u) + 1u;
                for (uint32_t i = first; i < first + cnt; ++i) b.grow(slot_box[i]);
            } else {
                b = node_box[code];
            }
            for (int a = 0; a < 3; ++a) { wn.lo[c][a] = b.lo[a]; wn.hi[c][a] = b.hi[a]; }
            node_box[k].grow(b);
        }
    }
    quantise(t);
}

namespace {

uint32_t ceil_log2(uint64_t x) {             // x >= 1
    uint32_t l = 0;
    while (((uint64_t)1 << l) < x) ++l;
    return l;
}

struct MortonPlanner {
    Topology& t;
    uint32_t n;
    uint32_t leaf_code(uint32_t j) const { return kLeafBit | ((std::min(kMaxLeaf, n - 4u * j) - 1u) << 28) | (4u * j); }
    // the arity of a node over m leaves with budget B (0: none fits)
    static uint32_t arity(uint32_t m, uint32_t budget) {
        for (uint32_t a = kWidth; a >= 2u; --a)
            if (a <= m && (a - 1u) + ceil_log2((m + a - 1u) / a) <= budget) return a;
        return 0u;
    }
    // node over the leaves [b, e), e - b >= 2; returns its index; *need = stack entries below the node's parent, *levels = binary levels
    uint32_t node(uint32_t b, uint32_t e, uint32_t budget, uint32_t* need, uint32_t* levels) {
        const uint32_t m = e - b, a = arity(m, budget);
        const uint32_t k = (uint32_t)(t.codes.size() / kWidth);
        t.codes.insert(t.codes.end(), kWidth, kDone);
        t.node_height.push_back(0u);
        uint32_t need_below = 0, levels_below = 0, height = 0;
        for (uint32_t i = 0; i < a; ++i) {
            const uint32_t cb = b + (uint32_t)((uint64_t)i * m / a), ce = b + (uint32_t)((uint64_t)(i + 1u) * m / a);
            uint32_t code;
            if (ce - cb == 1u) {
                code = leaf_code(cb);
            } else {
                uint32_t nd = 0, lv = 0;
                code = node(cb, ce, budget - (a - 1u), &nd, &lv);
                need_below = std::max(need_below, nd);
                levels_below = std::max(levels_below, lv);
                height = std::max(height, 1u + t.node_height[code]);
            }
            t.codes[kWidth * (size_t)k + i] = code;
        }
        t.node_height[k] = height;
        *need = (a - 1u) + need_below;
        *levels = (a == 2u ? 1u : 2u) + levels_below;
        return k;
    }
};

}  // namespace

Topology morton_topology(uint32_t n) {
    Topology t;
    const uint32_t n_leaves = n / 4u + (n % 4u != 0u);
    t.n_slots = 4u * n_leaves;
    MortonPlanner p{t, n};
    if (n_leaves == 1u) {
        t.root = p.leaf_code(0);
    } else if (n_leaves > 1u) {
        if (!MortonPlanner::arity(n_leaves, kStackDepth - 1u)) { t.ok = false; t.n_slots = 0; return t; }
        t.codes.reserve(kWidth * (size_t)n_leaves);              // (a tree over L leaves has fewer than L nodes)
        t.node_height.reserve(n_leaves);
        uint32_t need = 0, levels = 0;
        t.root = p.node(0, n_leaves, kStackDepth - 1u, &need, &levels);
        t.stack_need = 1u + need;
        t.depth = levels;
    }
    // the order by height, as order_by_height() forms it
    const size_t n_nodes = t.node_height.size();
    uint32_t top = 0;
    for (const uint32_t h : t.node_height) top = std::max(top, h);
    t.height_first.assign(n_nodes ? top + 2u : 1u, 0u);
    for (size_t k = 0; k < n_nodes; ++k) t.height_first[t.node_height[k] + 1u]++;
    for (size_t h = 1; h < t.height_first.size(); ++h) t.height_first[h] += t.height_first[h - 1];
    t.height_order.assign(n_nodes, 0u);
    std::vector<uint32_t> at(t.height_first.begin(), t.height_first.end());
    for (size_t k = 0; k < n_nodes; ++k) t.height_order[at[t.node_height[k]]++] = (uint32_t)k;
    return t;
}

namespace {
// the tree of the count-only topology t over the objects in the given order: leaf_ids, the nodes' codes, and the rest by refit()
void fill_ordered(Built& out, Topology& t, const std::vector<uint32_t>& order, const float4* shape, const uint32_t* shape_tag, uint32_t n) {
    const size_t n_nodes = t.node_height.size();
    out.leaf_ids.assign(t.n_slots, kDone);
    for (uint32_t p = 0; p < n; ++p) out.leaf_ids[p] = order[p] | (shape_tag[order[p]] != 0 ? kTriangleBit : 0u);
    out.leaf_rec.assign(3 * (size_t)t.n_slots, make_float4(0, 0, 0, 0));
    out.leaf_lead.assign(t.n_slots, make_float4(0, 0, 0, 0));
    out.leaf_prims = n;
    out.root = t.root;
    out.depth = t.depth;
    out.stack_need = t.stack_need;
    out.wide.resize(n_nodes);
    for (size_t k = 0; k < n_nodes; ++k) {
        WideNode& w = out.wide[k];
        w.n = 0;
        for (uint32_t c = 0; c < kWidth; ++c) {
            w.code[c] = t.codes[kWidth * k + c];
            if (w.code[c] != kDone) w.n = c + 1u;
        }
    }
    out.node_height = std::move(t.node_height);
    out.height_order = std::move(t.height_order);
    out.height_first = std::move(t.height_first);
    refit(out, shape, shape_tag, n);
}
}  // namespace

bool build_morton(Built& out, const float4* shape, const uint32_t* shape_tag, uint32_t n, std::vector<uint32_t>* keys_out, std::vector<uint32_t>* order_out) {
    out = Built{};
    Topology t = morton_topology(n);
    if (keys_out) keys_out->clear();
    if (order_out) order_out->clear();
    if (!t.ok) return false;
    const size_t n_nodes = t.node_height.size();
    const Bounds bd = scene_bounds(shape, shape_tag, n, n_nodes != 0);
    std::vector<uint32_t> keys(n, 0u), order(n);
    for (uint32_t i = 0; i < n; ++i) {
        order[i] = i;
        if (n_nodes == 0) continue;                              // no node, no grid: every key is 0
        float lo[3], hi[3];
        primitive_box(shape[3 * (size_t)i], shape[3 * (size_t)i + 1], shape[3 * (size_t)i + 2], shape_tag[i] != 0, lo, hi);
        keys[i] = morton_key(lo, hi, bd.grid_min, bd.grid_cell);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b] || (keys[a] == keys[b] && a < b); });
    fill_ordered(out, t, order, shape, shape_tag, n);
    if (keys_out) *keys_out = std::move(keys);
    if (order_out) *order_out = std::move(order);
    return true;
}

MedianPlan median_plan(uint32_t n) {
    MedianPlan pl;
    const Topology t = morton_topology(n);
    if (!t.ok) { pl.ok = false; return pl; }
    while (pl.index_bits < 32u && ((uint64_t)1 << pl.index_bits) < (uint64_t)n) ++pl.index_bits;
    const size_t n_nodes = t.node_height.size();
    if (n_nodes == 0) return pl;
    // the leaf range of every node: a node is numbered before the nodes beneath it
    std::vector<uint32_t> first(n_nodes), last(n_nodes);
    const auto child_range = [&](uint32_t code, uint32_t* b, uint32_t* e) {
        if (code & kLeafBit) { *b = (code & 0x0FFFFFFFu) / 4u; *e = *b + 1u; }
        else { *b = first[code]; *e = last[code]; }
    };
    for (size_t k = n_nodes; k-- > 0;) {
        uint32_t b = 0, e = 0, e_last = 0;
        child_range(t.codes[kWidth * k], &first[k], &e_last);
        for (uint32_t c = 0; c < kWidth && t.codes[kWidth * k + c] != kDone; ++c) { child_range(t.codes[kWidth * k + c], &b, &e); e_last = e; }
        last[k] = e_last;
    }
    // the steps, depth first (the recursion is as deep as the tree's binary levels)
    struct Planner {
        const Topology& t;
        const std::vector<uint32_t>&first, &last;
        uint32_t n;
        std::vector<MedianStep>& steps;
        std::vector<uint32_t>& tile_of;                          // per step: the tile it belongs to (kDone: above T)
        uint32_t n_tiles = 0;
        uint32_t pos(uint32_t leaf) const { return (uint32_t)std::min<uint64_t>(4ull * leaf, n); }
        uint32_t begin(uint32_t code) const { return code & kLeafBit ? (code & 0x0FFFFFFFu) / 4u : first[code]; }
        void node(uint32_t k, uint32_t level, uint32_t tile) {
            uint32_t c[kWidth + 1], a = 0;
            for (; a < kWidth && t.codes[kWidth * (size_t)k + a] != kDone; ++a) c[a] = begin(t.codes[kWidth * (size_t)k + a]);
            c[a] = last[k];
            split(k, c, 0, a, level, tile);
        }
        void split(uint32_t k, const uint32_t* c, uint32_t lo, uint32_t hi, uint32_t level, uint32_t tile) {
            if (hi - lo == 1u) {
                const uint32_t code = t.codes[kWidth * (size_t)k + lo];
                if (!(code & kLeafBit)) node(code, level, tile);
                return;
            }
            const uint32_t mid = lo + (hi - lo + 1u) / 2u;
            const MedianStep s{level, pos(c[lo]), pos(c[hi]), pos(c[mid])};
            if (tile == kDone && s.Q - s.P <= kMedianTile) tile = n_tiles++;   // the highest step of at most T positions
            steps.push_back(s);
            tile_of.push_back(tile);
            split(k, c, lo, mid, level + 1u, tile);
            split(k, c, mid, hi, level + 1u, tile);
        }
    };
    std::vector<MedianStep> found;
    std::vector<uint32_t> tile_of;
    Planner planner{t, first, last, n, found, tile_of};
    planner.node(t.root, 0u, kDone);
    std::vector<uint32_t> by(found.size());                      // ascending by (level, P); depth first found them ascending by P per level
    for (size_t k = 0; k < by.size(); ++k) by[k] = (uint32_t)k;
    std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) { return found[a].level < found[b].level; });
    pl.steps.reserve(found.size());
    for (const uint32_t k : by) pl.steps.push_back(found[k]);
    // the device's view: levels of steps above T, then the tiles
    size_t i = 0;
    while (i < pl.steps.size()) {
        const uint32_t level = pl.steps[i].level;
        MedianPlan::Level lv{(uint32_t)pl.group_start.size(), 0u, 0u};
        uint32_t at = 0;                                         // first position not yet in a group
        const auto gap_to = [&](uint32_t to) {
            while (at < to) { pl.group_start.push_back(at); ++lv.groups; at = (uint32_t)std::min<uint64_t>((uint64_t)at + kMedianChunk, to); }
        };
        for (; i < pl.steps.size() && pl.steps[i].level == level; ++i) {
            const MedianStep& s = pl.steps[i];
            if (s.Q - s.P <= kMedianTile) continue;
            gap_to(s.P);
            pl.group_start.push_back(s.P | 0x80000000u);
            ++lv.groups;
            at = s.Q;
        }
        if (at == 0u) { pl.group_start.resize(lv.first); break; }   // no step of this level is above T, so none beneath is
        gap_to(n);
        pl.group_start.push_back(n);
        while (((uint64_t)1 << lv.bits) < (uint64_t)lv.groups) ++lv.bits;
        pl.max_groups = std::max(pl.max_groups, lv.groups);
        pl.levels.push_back(lv);
    }
    // the tiles (depth first numbered them ascending by P), each with its steps ascending by (level, P)
    pl.tiles.assign(planner.n_tiles, make_uint4(0u, 0u, 0u, 0u));
    for (const uint32_t k : by)
        if (tile_of[k] != kDone) pl.tiles[tile_of[k]].w++;
    uint32_t total = 0;
    for (uint4& tl : pl.tiles) { tl.z = total; total += tl.w; tl.w = 0u; }
    pl.tile_steps.resize(total);
    std::vector<uint32_t> level0(planner.n_tiles, 0u);
    for (const uint32_t k : by) {
        if (tile_of[k] == kDone) continue;
        uint4& tl = pl.tiles[tile_of[k]];
        const MedianStep& s = found[k];
        if (tl.w == 0u) { tl.x = s.P; tl.y = s.Q; level0[tile_of[k]] = s.level; }   // the tile's own step comes first
        pl.tile_steps[tl.z + tl.w++] = make_uint2((s.P - tl.x) | ((s.level - level0[tile_of[k]]) << 16), s.Q - tl.x);
    }
    return pl;
}

bool build_median(Built& out, const float4* shape, const uint32_t* shape_tag, uint32_t n, std::vector<uint32_t>* g_out, std::vector<uint32_t>* order_out) {
    out = Built{};
    Topology t = morton_topology(n);
    if (g_out) g_out->clear();
    if (order_out) order_out->clear();
    if (!t.ok) return false;
    const size_t n_nodes = t.node_height.size();
    const Bounds bd = scene_bounds(shape, shape_tag, n, n_nodes != 0);
    std::vector<uint32_t> g(3 * (size_t)n, 0u), order(n);
    for (uint32_t i = 0; i < n; ++i) {
        order[i] = i;
        if (n_nodes == 0) continue;                              // no node, no grid, no step
        float lo[3], hi[3];
        primitive_box(shape[3 * (size_t)i], shape[3 * (size_t)i + 1], shape[3 * (size_t)i + 2], shape_tag[i] != 0, lo, hi);
        for (int k = 0; k < 3; ++k) g[3 * (size_t)i + k] = grid_coord(lo, hi, bd.grid_min, bd.grid_cell, k);
    }
    const MedianPlan pl = median_plan(n);
    for (const MedianStep& s : pl.steps) {                       // by level: a parent before its children
        uint32_t gmin[3] = {65535u, 65535u, 65535u}, gmax[3] = {0u, 0u, 0u};
        for (uint32_t p = s.P; p < s.Q; ++p)
            for (int k = 0; k < 3; ++k) {
                const uint32_t v = g[3 * (size_t)order[p] + k];
                gmin[k] = std::min(gmin[k], v); gmax[k] = std::max(gmax[k], v);
            }
        int axis = 0;
        double widest = (double)(gmax[0] - gmin[0]) * (double)bd.grid_cell[0];
        for (int k = 1; k < 3; ++k) {
            const double w = (double)(gmax[k] - gmin[k]) * (double)bd.grid_cell[k];
            if (w > widest) { widest = w; axis = k; }
        }
        std::sort(order.begin() + s.P, order.begin() + s.Q, [&](uint32_t a, uint32_t b) {
            const uint32_t ga = g[3 * (size_t)a + axis], gb = g[3 * (size_t)b + axis];
            return ga < gb || (ga == gb && a < b);
        });
    }
    fill_ordered(out, t, order, shape, shape_tag, n);
    if (g_out) *g_out = std::move(g);
    if (order_out) *order_out = std::move(order);
    return true;
}

}  // namespace ptbvh
