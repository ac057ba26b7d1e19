// pt_bvh_check.cpp -- the host-side verification of the BVH builders (no device, no kernel object; compiled by the host-only
// sanitizer build beside pt_host.cpp): the invariants of a tree (bvh_verify), and the pt_debug_bvh_* entries that run the host
// rules of pt_bvh.cpp -- build, refit, the Morton and the median order -- verify the result and export it (struct BvhExport,
// pt_scene_bvh.h: the contract pt_debug_bvh_read writes from the device).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_bvh.h"
#include "pt_context.h"
#include "pt_scene_records.h"

using ptscene::shape_records;

namespace {

// gather records, scan records and shape tags of the objects, as an upload forms them
int bvh_records(const char* who, const PtObject* objs, uint32_t n, std::vector<float4>& shape, std::vector<float4>& scan, std::vector<uint32_t>& tag) {
    shape.assign(3 * (size_t)n + 1, make_float4(0, 0, 0, 0)); scan.assign(3 * (size_t)n + 1, make_float4(0, 0, 0, 0));
    tag.assign(n + 1, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        if (objs[i].shape_tag > PT_SHAPE_TRIANGLE) return fail(PT_ERR_INVALID_ARG, "%s: object %u: bad shape_tag %u", who, i, objs[i].shape_tag);
        int ns = 0;
        shape_records(objs[i], &shape[3 * (size_t)i], &scan[3 * (size_t)i], &ns);
        tag[i] = objs[i].shape_tag;
    }
    return PT_OK;
}

// The invariants of a tree over the n objects with these records (pt_debug_bvh_check, pt_debug_bvh_refit_check): PT_OK, or
// PT_ERR_UNSUPPORTED with the violated one in pt_last_error().
int bvh_verify(const ptbvh::Built& b, const std::vector<float4>& shape, const std::vector<float4>& scan, const std::vector<uint32_t>& tag, uint32_t n) {
    if (b.non_finite) return fail(PT_ERR_UNSUPPORTED, "accel: %u object(s) with a NaN/inf coordinate", b.non_finite);
    if (b.depth + 2u > ptbvh::kStackDepth || b.stack_need > ptbvh::kStackDepth)
        return fail(PT_ERR_UNSUPPORTED, "BVH (depth %u, stack need %u) exceeds the traversal stack", b.depth, b.stack_need);
    if (b.leaf_prims != n || b.leaf_rec.size() != 3 * b.leaf_ids.size() || b.leaf_lead.size() != b.leaf_ids.size() || b.leaf_ids.size() % 4u != 0u)
        return fail(PT_ERR_UNSUPPORTED, "%u primitives in %zu leaf slots for %u objects", b.leaf_prims, b.leaf_ids.size(), n);
    if (n == 0) return b.root == ptbvh::kDone ? PT_OK : fail(PT_ERR_UNSUPPORTED, "empty scene: root is not the sentinel");
    // boxes of the primitives in f64 from the same f32 records the device tests
    auto prim_box = [&](uint32_t o, double lo[3], double hi[3]) {
        const float4 r0 = shape[3 * (size_t)o], r1 = shape[3 * (size_t)o + 1], r2 = shape[3 * (size_t)o + 2];
        if (tag[o] == PT_SHAPE_SPHERE) {
            const double r = std::sqrt((double)(r0.w * r0.w));
            const double c[3] = {r0.x, r0.y, r0.z};
            for (int k = 0; k < 3; ++k) { lo[k] = c[k] - r; hi[k] = c[k] + r; }
        } else {
            const double v0[3] = {r0.x, r0.y, r0.z}, e1[3] = {r1.x, r1.y, r1.z}, e2[3] = {r2.x, r2.y, r2.z};
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(v0[k], std::min(v0[k] + e1[k], v0[k] + e2[k]));
                hi[k] = std::max(v0[k], std::max(v0[k] + e1[k], v0[k] + e2[k]));
            }
        }
    };
    std::vector<uint8_t> seen(n, 0);
    std::string err;
    // returns the exact bounds of the subtree and the stack entries a traversal can need below it (sum over the deepest
    // path of children - 1); checks the bounds against the box the parent stores for the subtree
    struct Walker {
        const ptbvh::Built& b; const std::vector<float4>& scan; const std::vector<uint32_t>& tag; std::vector<uint8_t>& seen;
        decltype(prim_box)& pbox; std::string& err; uint32_t n;
        bool walk(uint32_t code, double lo[3], double hi[3], uint32_t* need) {
            for (int k = 0; k < 3; ++k) { lo[k] = 1e300; hi[k] = -1e300; }
            *need = 0;
            if (code == ptbvh::kDone) { err = "sentinel inside the tree"; return false; }
            if (code & ptbvh::kLeafBit) {
                const uint32_t first = code & 0x0FFFFFFFu, cnt = ((code >> 28) & 7u) + 1u;
                if (cnt > ptbvh::kMaxLeaf || (size_t)first + cnt > b.leaf_ids.size() || first % 4u != 0u) { err = "leaf range out of bounds or not aligned to 4 slots"; return false; }
                for (uint32_t i = first; i < first + cnt; ++i) {
                    const uint32_t w = b.leaf_ids[i], o = w & 0x7FFFFFFFu;
                    if (o >= n || seen[o]) { err = "object missing or in two leaves"; return false; }
                    seen[o] = 1;
                    if (((w >> 31) != 0) != (tag[o] == PT_SHAPE_TRIANGLE)) { err = "leaf tag bit differs from the object's shape"; return false; }
                    const int ns = tag[o] == PT_SHAPE_TRIANGLE ? 3 : 1;
                    if (std::memcmp(&b.leaf_rec[3 * (size_t)i], &scan[3 * (size_t)o], ns * sizeof(float4)) != 0) { err = "leaf record differs from the scan record"; return false; }
                    if (std::memcmp(&b.leaf_lead[i], &scan[3 * (size_t)o], sizeof(float4)) != 0) { err = "lead record differs from the scan record"; return false; }
                    double pl[3], ph[3];
                    pbox(o, pl, ph);
                    for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], pl[k]); hi[k] = std::max(hi[k], ph[k]); }
                }
                return true;
            }
            if ((size_t)code >= b.wide.size()) { err = "node index out of bounds"; return false; }
            const ptbvh::WideNode& wn = b.wide[code];
            if (wn.n < 2 || wn.n > ptbvh::kWidth) { err = "node with fewer than 2 or more than 4 children"; return false; }
            // what the device traverses: the boxes decoded from the 16-bit grid; they must contain the f32 boxes
            if (4 * (size_t)code + 3 >= b.qnodes.size()) { err = "quantised node index out of bounds"; return false; }
            const uint4 qa = b.qnodes[4 * (size_t)code], qb = b.qnodes[4 * (size_t)code + 1], qc = b.qnodes[4 * (size_t)code + 2],
                        qd = b.qnodes[4 * (size_t)code + 3];
            const uint32_t qcode[4] = {qd.x, qd.y, qd.z, qd.w};
            const uint32_t qw[4][3] = {{qa.x, qa.y, qa.z}, {qa.w, qb.x, qb.y}, {qb.z, qb.w, qc.x}, {qc.y, qc.z, qc.w}};
            uint32_t need_below = 0;
            for (uint32_t c = 0; c < ptbvh::kWidth; ++c) {
                if (qcode[c] != wn.code[c]) { err = "quantised node carries other child codes"; return false; }
                if (c >= wn.n) {
                    if (wn.code[c] != ptbvh::kDone) { err = "unused child slot without the sentinel code"; return false; }
                    continue;
                }
                const uint32_t q[6] = {qw[c][0] & 0xFFFFu, qw[c][0] >> 16, qw[c][1] & 0xFFFFu, qw[c][1] >> 16, qw[c][2] & 0xFFFFu, qw[c][2] >> 16};
                float blo[3], bhi[3];
                for (int k = 0; k < 3; ++k) {
                    blo[k] = std::fmaf((float)q[k], b.grid_cell[k], b.grid_min[k]);
                    bhi[k] = std::fmaf((float)q[3 + k], b.grid_cell[k], b.grid_min[k]);
                    if (!(blo[k] <= wn.lo[c][k] && bhi[k] >= wn.hi[c][k])) { err = "quantised child box does not contain the f32 box"; return false; }
                }
                double cl[3], ch[3];
                uint32_t nd = 0;
                if (!walk(wn.code[c], cl, ch, &nd)) return false;
                need_below = std::max(need_below, nd);
                for (int k = 0; k < 3; ++k) {
                    if (!((double)blo[k] <= cl[k] && (double)bhi[k] >= ch[k])) { err = "child box does not enclose its subtree"; return false; }
                    lo[k] = std::min(lo[k], cl[k]); hi[k] = std::max(hi[k], ch[k]);
                }
            }
            *need = (wn.n - 1u) + need_below;
            return true;
        }
    } w{b, scan, tag, seen, prim_box, err, n};
    uint32_t need = 0;
    double lo[3], hi[3];
    if (!w.walk(b.root, lo, hi, &need)) return fail(PT_ERR_UNSUPPORTED, "BVH invariant: %s", err.c_str());
    for (uint32_t i = 0; i < n; ++i) if (!seen[i]) return fail(PT_ERR_UNSUPPORTED, "BVH invariant: object %u is in no leaf", i);
    if (1u + need != b.stack_need) return fail(PT_ERR_UNSUPPORTED, "BVH invariant: stack need %u reported, %u found", b.stack_need, 1u + need);
    double amax = 0.0;
    for (int k = 0; k < 3; ++k) amax += std::max(std::fabs(lo[k]), std::fabs(hi[k]));
    if (!((double)b.scene_abs >= amax)) return fail(PT_ERR_UNSUPPORTED, "BVH invariant: scene_abs %g below the scene extent %g", (double)b.scene_abs, amax);
    return PT_OK;
}

// The tree into the caller's arrays, clamped by their capacities (the tail of the three checks below)
void export_tree(const ptbvh::Built& b, const BvhExport& out) {
    const size_t nn = out.nodes(b.wide.size()), nsl = out.slots(b.leaf_ids.size());
    if (nn) std::memcpy(out.qnodes, b.qnodes.data(), nn * 4 * sizeof(uint4));
    if (nsl) {
        std::memcpy(out.leaf_rec, b.leaf_rec.data(), nsl * 3 * sizeof(float4));
        std::memcpy(out.leaf_lead, b.leaf_lead.data(), nsl * sizeof(float4));
        std::memcpy(out.leaf_ids, b.leaf_ids.data(), nsl * sizeof(uint32_t));
    }
    out.scalars(b.grid_min, b.grid_cell, b.scene_abs, b.root);
    for (int k = 0; k < 3; ++k)
        if (out.cost_now) out.cost_now[k] = b.cost[k];
}

// The Morton rule: the order is ascending by (key, index), and slot p holds sorted position p
int morton_order_check(const ptbvh::Built& b, const std::vector<uint32_t>& keys, const std::vector<uint32_t>& order, uint32_t n) {
    for (uint32_t p = 0; p < n; ++p) {
        if (p && !(keys[order[p - 1]] < keys[order[p]] || (keys[order[p - 1]] == keys[order[p]] && order[p - 1] < order[p])))
            return fail(PT_ERR_UNSUPPORTED, "BVH build: sorted positions %u and %u are out of order", p - 1, p);
        if ((b.leaf_ids[p] & ~ptbvh::kTriangleBit) != order[p]) return fail(PT_ERR_UNSUPPORTED, "BVH build: slot %u does not hold sorted position %u", p, p);
    }
    return PT_OK;
}

// The median rule: the slots hold the order it gives -- the steps once more, each as "the range in index order, then a stable sort
// by the axis' coordinate", another route to the same total order.  cell: the grid of the build pose
int median_order_check(const ptbvh::Built& b, const std::vector<uint32_t>& g, const std::vector<uint32_t>& order, uint32_t n, const float cell[3]) {
    std::vector<uint32_t> again(n);
    for (uint32_t i = 0; i < n; ++i) again[i] = i;
    const ptbvh::MedianPlan pl = ptbvh::median_plan(n);
    for (const ptbvh::MedianStep& st : pl.steps) {
        if (!(st.P < st.cut && st.cut < st.Q && st.Q <= n)) return fail(PT_ERR_UNSUPPORTED, "BVH build: step [%u, %u) with its cut at %u", st.P, st.Q, st.cut);
        std::sort(again.begin() + st.P, again.begin() + st.Q);
        int axis = 0;
        double widest = -1.0;
        for (int k = 0; k < 3; ++k) {
            uint32_t mn = 0xFFFFFFFFu, mx = 0u;
            for (uint32_t p = st.P; p < st.Q; ++p) { mn = std::min(mn, g[3 * (size_t)again[p] + k]); mx = std::max(mx, g[3 * (size_t)again[p] + k]); }
            const double w = (double)(mx - mn) * (double)cell[k];
            if (k == 0 || w > widest) { widest = w; axis = k; }
        }
        std::stable_sort(again.begin() + st.P, again.begin() + st.Q, [&](uint32_t x, uint32_t y) { return g[3 * (size_t)x + axis] < g[3 * (size_t)y + axis]; });
    }
    for (uint32_t p = 0; p < n; ++p)
        if (again[p] != order[p] || (b.leaf_ids[p] & ~ptbvh::kTriangleBit) != order[p])
            return fail(PT_ERR_UNSUPPORTED, "BVH build: slot %u does not hold the object the median rule puts at position %u", p, p);
    return PT_OK;
}

// pt_debug_bvh_morton_check and pt_debug_bvh_median_check: the tree of objs by the host rule of the order, verified; carried to
// refit_objs (another pose of the same objects) by the host refit and verified again; the order's own rule; the export, with per
// object (up to cap_objs) its key -- one Morton key, or the three grid cells of the median order -- and the object at every position.
int order_check(const char* who, bool median, const PtObject* objs, const PtObject* refit_objs, uint32_t n, const BvhExport& out, uint32_t* n_nodes,
                uint32_t* n_slots, uint32_t* out_keys, uint32_t* out_order, uint32_t cap_objs) {
    if (n && !objs) return fail(PT_ERR_INVALID_ARG, "%s: null objects", who);
    if (out.null_array() || (cap_objs && (!out_keys || !out_order))) return fail(PT_ERR_INVALID_ARG, "%s: null output array with a non-zero capacity", who);
    std::vector<float4> shape, scan;
    std::vector<uint32_t> tag, keys, order;
    if (int rc = bvh_records(who, objs, n, shape, scan, tag)) return rc;
    ptbvh::Built b;
    if (!(median ? ptbvh::build_median : ptbvh::build_morton)(b, shape.data(), tag.data(), n, &keys, &order))
        return fail(PT_ERR_UNSUPPORTED, "%s: no tree over %u objects fits the traversal stack (%u entries)", who, n, ptbvh::kStackDepth);
    if (n_nodes) *n_nodes = (uint32_t)b.wide.size();
    if (n_slots) *n_slots = (uint32_t)b.leaf_ids.size();
    if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    const float cell[3] = {b.grid_cell[0], b.grid_cell[1], b.grid_cell[2]};    // the grid of the build pose
    if (refit_objs) {
        for (uint32_t i = 0; i < n; ++i)
            if (objs[i].shape_tag != refit_objs[i].shape_tag)
                return fail(PT_ERR_INVALID_ARG, "%s: object %u: shape tags %u and %u", who, i, objs[i].shape_tag, refit_objs[i].shape_tag);
        if (int rc = bvh_records(who, refit_objs, n, shape, scan, tag)) return rc;
        ptbvh::refit(b, shape.data(), tag.data(), n);
        if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    }
    if (int rc = median ? median_order_check(b, keys, order, n, cell) : morton_order_check(b, keys, order, n)) return rc;
    export_tree(b, out);
    if (const size_t no = std::min<size_t>(n, cap_objs)) {
        std::memcpy(out_keys, keys.data(), no * (median ? 3 : 1) * sizeof(uint32_t));
        std::memcpy(out_order, order.data(), no * sizeof(uint32_t));
    }
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_debug_bvh_check(const PtObject* objs, uint32_t n, uint32_t* depth, uint32_t* n_nodes, uint32_t* n_leaf_slots) {
    if (!objs && n) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_check: null objects");
    if (n >= (1u << 28)) return fail(PT_ERR_UNSUPPORTED, "accel: %u objects exceed the 2^28 leaf slots", n);
    std::vector<float4> shape, scan;
    std::vector<uint32_t> tag;
    if (int rc = bvh_records("pt_debug_bvh_check", objs, n, shape, scan, tag)) return rc;
    const ptbvh::Built b = ptbvh::build(shape.data(), tag.data(), n);
    if (depth) *depth = b.depth;
    if (n_nodes) *n_nodes = (uint32_t)b.wide.size();
    if (n_leaf_slots) *n_leaf_slots = b.leaf_prims;          // slots that hold a primitive (leaves are padded to multiples of 4 slots)
    return bvh_verify(b, shape, scan, tag, n);
}

int pt_debug_bvh_refit_check(const PtObject* prev_objs, const PtObject* cur_objs, uint32_t n, uint32_t refit, uint32_t* out_qnodes, uint32_t cap_nodes,
                             float* out_leaf_rec, float* out_leaf_lead, uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes,
                             uint32_t* n_slots, float* out_grid, uint32_t* root, uint64_t* cost_now, uint64_t* cost_at_build) {
    const BvhExport out{out_qnodes, cap_nodes, out_leaf_rec, out_leaf_lead, out_leaf_ids, cap_slots, out_grid, root, cost_now};
    if (n && (!prev_objs || !cur_objs)) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_refit_check: null objects");
    if (out.null_array()) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_refit_check: null output array with a non-zero capacity");
    if (n >= (1u << 28)) return fail(PT_ERR_UNSUPPORTED, "accel: %u objects exceed the 2^28 leaf slots", n);
    for (uint32_t i = 0; i < n; ++i)
        if (prev_objs[i].shape_tag != cur_objs[i].shape_tag)
            return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_refit_check: object %u: shape tags %u and %u", i, prev_objs[i].shape_tag, cur_objs[i].shape_tag);
    std::vector<float4> shape, scan;
    std::vector<uint32_t> tag;
    if (int rc = bvh_records("pt_debug_bvh_refit_check", prev_objs, n, shape, scan, tag)) return rc;
    ptbvh::Built b = ptbvh::build(shape.data(), tag.data(), n);
    if (b.non_finite) return fail(PT_ERR_UNSUPPORTED, "accel: %u object(s) of the build pose with a NaN/inf coordinate", b.non_finite);
    const std::vector<uint32_t> ids0 = b.leaf_ids;
    std::vector<uint32_t> codes0;
    for (const ptbvh::WideNode& w : b.wide) codes0.insert(codes0.end(), w.code, w.code + ptbvh::kWidth);
    const uint32_t root0 = b.root;
    const uint64_t cost0[3] = {b.cost[0], b.cost[1], b.cost[2]};
    if (refit) {                                                 // (0: the tree as built, verified against prev_objs)
        if (int rc = bvh_records("pt_debug_bvh_refit_check", cur_objs, n, shape, scan, tag)) return rc;
        ptbvh::refit(b, shape.data(), tag.data(), n);
    }
    if (n_nodes) *n_nodes = (uint32_t)b.wide.size();
    if (n_slots) *n_slots = (uint32_t)b.leaf_ids.size();
    if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    // the topology is the build's
    if (b.root != root0 || b.leaf_ids != ids0) return fail(PT_ERR_UNSUPPORTED, "BVH refit: root or leaf ids differ from the build's");
    for (size_t k = 0; k < b.wide.size(); ++k)
        if (std::memcmp(b.wide[k].code, &codes0[ptbvh::kWidth * k], sizeof b.wide[k].code) != 0)
            return fail(PT_ERR_UNSUPPORTED, "BVH refit: node %zu carries other child codes than the build's", k);
    // the same bounds from one pass over the objects (what pt_scene_refit computes on the host)
    const ptbvh::Bounds bd = ptbvh::scene_bounds(shape.data(), tag.data(), n, !b.wide.empty());
    if (std::memcmp(bd.grid_min, b.grid_min, sizeof bd.grid_min) != 0 || std::memcmp(bd.grid_cell, b.grid_cell, sizeof bd.grid_cell) != 0 ||
        std::memcmp(&bd.scene_abs, &b.scene_abs, sizeof(float)) != 0 || bd.non_finite != b.non_finite)
        return fail(PT_ERR_UNSUPPORTED, "BVH refit: the bounds of the objects differ from the bounds of the child boxes");
    export_tree(b, out);
    for (int k = 0; k < 3; ++k)
        if (cost_at_build) cost_at_build[k] = cost0[k];
    return PT_OK;
}

int pt_debug_bvh_morton_check(const PtObject* objs, const PtObject* refit_objs, uint32_t n, uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead,
                              uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid, uint32_t* root,
                              uint64_t* cost_now, uint32_t* out_keys, uint32_t* out_order, uint32_t cap_objs) {
    return order_check("pt_debug_bvh_morton_check", false, objs, refit_objs, n, {out_qnodes, cap_nodes, out_leaf_rec, out_leaf_lead, out_leaf_ids, cap_slots, out_grid, root, cost_now},
                       n_nodes, n_slots, out_keys, out_order, cap_objs);
}
int pt_debug_bvh_median_check(const PtObject* objs, const PtObject* refit_objs, uint32_t n, uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead,
                              uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid, uint32_t* root,
                              uint64_t* cost_now, uint32_t* out_keys, uint32_t* out_order, uint32_t cap_objs) {
    return order_check("pt_debug_bvh_median_check", true, objs, refit_objs, n, {out_qnodes, cap_nodes, out_leaf_rec, out_leaf_lead, out_leaf_ids, cap_slots, out_grid, root, cost_now},
                       n_nodes, n_slots, out_keys, out_order, cap_objs);
}

int pt_debug_bvh_morton_topology(uint32_t n, uint32_t* out_codes, uint32_t* out_height, uint32_t* out_order, uint32_t cap_nodes, uint32_t* out_height_first,
                                 uint32_t cap_heights, uint32_t* n_nodes, uint32_t* n_heights, uint32_t* n_slots, uint32_t* root, uint32_t* stack_need,
                                 uint32_t* depth) {
    if ((cap_nodes && (!out_codes || !out_height || !out_order)) || (cap_heights && !out_height_first))
        return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_morton_topology: null output array with a non-zero capacity");
    // (callers ask twice, for the sizes and then for the arrays: the plan of the last count is kept per thread)
    static thread_local ptbvh::Topology t;
    static thread_local int64_t t_n = -1;
    if (t_n != (int64_t)n) { t = ptbvh::morton_topology(n); t_n = (int64_t)n; }
    if (!t.ok) return fail(PT_ERR_UNSUPPORTED, "pt_debug_bvh_morton_topology: no tree over %u objects fits the traversal stack (%u entries)", n, ptbvh::kStackDepth);
    const size_t nn = std::min<size_t>(t.node_height.size(), cap_nodes), nh = std::min<size_t>(t.height_first.size(), cap_heights);
    if (nn) {
        std::memcpy(out_codes, t.codes.data(), nn * ptbvh::kWidth * sizeof(uint32_t));
        std::memcpy(out_height, t.node_height.data(), nn * sizeof(uint32_t));
        std::memcpy(out_order, t.height_order.data(), nn * sizeof(uint32_t));
    }
    if (nh) std::memcpy(out_height_first, t.height_first.data(), nh * sizeof(uint32_t));
    if (n_nodes) *n_nodes = (uint32_t)t.node_height.size();
    if (n_heights) *n_heights = (uint32_t)t.height_first.size();
    if (n_slots) *n_slots = t.n_slots;
    if (root) *root = t.root;
    if (stack_need) *stack_need = t.stack_need;
    if (depth) *depth = t.depth;
    if (nn && nn == t.node_height.size()) { t = ptbvh::Topology{}; t_n = -1; }   // delivered in full: let the memory go
    return PT_OK;
}

int pt_debug_bvh_median_plan(uint32_t n, uint32_t* out_steps, uint32_t cap_steps, uint32_t* n_steps, uint32_t* tile) {
    if (cap_steps && !out_steps) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_median_plan: null output array with a non-zero capacity");
    // (callers ask twice, for the size and then for the array: the plan of the last count is kept per thread)
    static thread_local ptbvh::MedianPlan pl;
    static thread_local int64_t pl_n = -1;
    if (pl_n != (int64_t)n) { pl = ptbvh::median_plan(n); pl_n = (int64_t)n; }
    if (!pl.ok) return fail(PT_ERR_UNSUPPORTED, "pt_debug_bvh_median_plan: no tree over %u objects fits the traversal stack (%u entries)", n, ptbvh::kStackDepth);
    static_assert(sizeof(ptbvh::MedianStep) == 4 * sizeof(uint32_t), "a step is four words");
    const size_t ns = std::min<size_t>(pl.steps.size(), cap_steps);
    if (ns) std::memcpy(out_steps, pl.steps.data(), ns * sizeof(ptbvh::MedianStep));
    if (n_steps) *n_steps = (uint32_t)pl.steps.size();
    if (tile) *tile = ptbvh::kMedianTile;
    if (ns && ns == pl.steps.size()) { pl = ptbvh::MedianPlan{}; pl_n = -1; }   // delivered in full: let the memory go
    return PT_OK;
}

}  // extern "C"
