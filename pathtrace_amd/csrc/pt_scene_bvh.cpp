// pt_scene_bvh.cpp -- struct DeviceBvh (pt_scene_bvh.h): every operation on the context's device tree and the one place its
// invariants I1 .. I6 are kept.  pt_scene.cpp decides which operations a scene call runs; the kernels are pt_film_bvh.h's.
#include <utility>

#include "pt_context.h"

void DeviceBvh::bind(ptk::SceneView& view, uint32_t root) const {
    view.bvh.nodes = nodes.p; view.bvh.rec = rec.p; view.bvh.ids = ids.p; view.bvh.lead = lead.p;
    view.bvh.root = root;
}
void DeviceBvh::set_grid(ptk::SceneView& view, const float grid_min[3], const float grid_cell[3], float scene_abs) {
    for (int k = 0; k < 3; ++k) { view.bvh.grid_min[k] = grid_min[k]; view.bvh.grid_cell[k] = grid_cell[k]; }
    view.bvh.scene_abs = scene_abs;
}

int DeviceBvh::why_not() const {
    if (refused) return fail(PT_ERR_UNSUPPORTED, "accel: the scene has object(s) with a NaN/inf coordinate; use the linear scan");
    if (failed) return fail(PT_ERR_UNSUPPORTED, "accel: the BVH of this scene is deeper than the traversal stack; use the linear scan");
    return PT_OK;
}

void DeviceBvh::drop(ptk::SceneView& view, bool is_refused, bool is_failed) {
    view.bvh = ptk::BvhView{};
    has = false;
    refused = is_refused; failed = is_failed;
}

int DeviceBvh::adopt(const ptbvh::Built& b, hipStream_t stream, ptk::SceneView& view) {
    int rc;
    if ((rc = nodes.ensure(b.qnodes.size() + 2)) || (rc = rec.ensure(b.leaf_rec.size() + 3)) || (rc = ids.ensure(b.leaf_ids.size() + 4)) ||
        (rc = lead.ensure(b.leaf_lead.size() + 4)) || (rc = order.ensure(b.height_order.size() + 1)) || (rc = cost_sums.ensure(4)))
        return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    if (!b.qnodes.empty()) HIP_TRY(hipMemcpy(nodes.p, b.qnodes.data(), b.qnodes.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if (!b.leaf_rec.empty()) HIP_TRY(hipMemcpy(rec.p, b.leaf_rec.data(), b.leaf_rec.size() * sizeof(float4), hipMemcpyHostToDevice));
    if (!b.leaf_ids.empty()) HIP_TRY(hipMemcpy(ids.p, b.leaf_ids.data(), b.leaf_ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!b.leaf_lead.empty()) HIP_TRY(hipMemcpy(lead.p, b.leaf_lead.data(), b.leaf_lead.size() * sizeof(float4), hipMemcpyHostToDevice));
    // for the refit: the order of the nodes by height, and the cost sums of the tree as built
    if (!b.height_order.empty()) HIP_TRY(hipMemcpy(order.p, b.height_order.data(), b.height_order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "cost words");
    HIP_TRY(hipMemcpy(cost_sums.p, b.cost, sizeof b.cost, hipMemcpyHostToDevice));
    height_first = b.height_first;
    n_nodes = (uint32_t)b.wide.size();
    n_slots = (uint32_t)b.leaf_ids.size();
    cost_build = ptbvh::cost_value(b.cost, b.grid_cell);
    cost_on_device = false;
    is_morton = false;                           // the arrays hold the host builder's topology now (I4)
    refits = 0;
    bind(view, b.root);
    set_grid(view, b.grid_min, b.grid_cell, b.scene_abs);
    depth = b.depth;
    has = true;
    return PT_OK;
}

int DeviceBvh::plan(uint32_t n, uint32_t order_value, const char* who, Rebuild* out) const {
    Rebuild r;
    r.n = n;
    r.new_topo = topo.n != (int64_t)n;
    if (r.new_topo) {
        r.topo = ptbvh::morton_topology(n);
        if (!r.topo.ok)
            return fail(PT_ERR_UNSUPPORTED, "%s: no tree over %u objects fits the traversal stack (%u entries); use pt_scene_update", who, n, ptbvh::kStackDepth);
    }
    // the median order's split plan likewise (the same counts have one)
    r.median = order_value == PT_BVH_ORDER_MEDIAN;
    r.new_plan = r.median && med_n != (int64_t)n;
    if (r.new_plan) r.med = ptbvh::median_plan(n);
    r.nodes = r.new_topo ? (uint32_t)r.topo.node_height.size() : topo.nodes;
    r.slots = r.new_topo ? r.topo.n_slots : topo.slots;
    *out = std::move(r);
    return PT_OK;
}

int DeviceBvh::reserve_refit() {
    int rc;
    if ((rc = slot_box.ensure(2 * (size_t)n_slots + 1)) || (rc = node_box.ensure(2 * (size_t)n_nodes + 1))) return rc;
    return PT_OK;
}

int DeviceBvh::reserve_rebuild(const Rebuild& r, ptk::SceneView& view) {
    // the tree arrays at the size of r's tree (a held tree's arrays may be too small: growing one drops its content)
    const uint4* nodes0 = nodes.p;
    const uint32_t* order0 = order.p;
    const size_t n = r.n, mt_nodes = r.nodes, mt_slots = r.slots;
    int rc;
    if ((rc = nodes.ensure(4 * mt_nodes + 2)) || (rc = rec.ensure(3 * mt_slots + 3)) || (rc = ids.ensure(mt_slots + 4)) || (rc = lead.ensure(mt_slots + 4)) ||
        (rc = order.ensure(mt_nodes + 1)) || (rc = cost_sums.ensure(4)) || (rc = cost_built.ensure(4)) ||
        (rc = slot_box.ensure(2 * mt_slots + 1)) || (rc = node_box.ensure(2 * mt_nodes + 1)) ||
        (rc = pairs[0].ensure(n + 1)) || (rc = pairs[1].ensure(n + 1)) || (rc = hist.ensure((size_t)ptk::kSortDigits * ptk::bvh_sort_tiles(r.n) + 4)) ||
        (rc = topo.codes.ensure(mt_nodes + 1)) || (rc = topo.order.ensure(mt_nodes + 1)) ||
        (r.median && ((rc = cells.ensure(n + 1)) ||
                      (r.new_plan && ((rc = med_bounds.ensure(6 * (size_t)r.med.max_groups + 1)) || (rc = med_groups.ensure(r.med.group_start.size() + 1)) ||
                                      (rc = med_tiles.ensure(r.med.tiles.size() + 1)) || (rc = med_tsteps.ensure(r.med.tile_steps.size() + 1))))))) {
        view.bvh = ptk::BvhView{};               // I5 (an array of the held tree may be gone), and the caches with it
        has = false;
        is_morton = false;
        topo.n = -1;
        med_n = -1;
        return rc;
    }
    if (nodes.p != nodes0 || order.p != order0) is_morton = false;   // I4
    return PT_OK;
}

int DeviceBvh::upload_plan(Rebuild& r) {
    if (r.new_topo) {
        // the child codes and the order by height
        static_assert(sizeof(uint4) == ptbvh::kWidth * sizeof(uint32_t), "code words of a node");
        topo.n = -1;
        is_morton = false;
        if (r.nodes) {
            HIP_TRY(hipMemcpy(topo.codes.p, r.topo.codes.data(), (size_t)r.nodes * sizeof(uint4), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(topo.order.p, r.topo.height_order.data(), (size_t)r.nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
        topo.height_first = std::move(r.topo.height_first);
        topo.nodes = r.nodes; topo.slots = r.slots; topo.root = r.topo.root; topo.depth = r.topo.depth;
        topo.n = (int64_t)r.n;
    }
    if (r.new_plan) {
        // the groups of the levels above T, the tiles and their steps
        const ptbvh::MedianPlan& p = r.med;
        med_n = -1;
        if (!p.group_start.empty()) HIP_TRY(hipMemcpy(med_groups.p, p.group_start.data(), p.group_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (!p.tiles.empty()) HIP_TRY(hipMemcpy(med_tiles.p, p.tiles.data(), p.tiles.size() * sizeof(uint4), hipMemcpyHostToDevice));
        if (!p.tile_steps.empty()) HIP_TRY(hipMemcpy(med_tsteps.p, p.tile_steps.data(), p.tile_steps.size() * sizeof(uint2), hipMemcpyHostToDevice));
        med_levels.clear();
        for (const ptbvh::MedianPlan::Level& lv : p.levels) med_levels.push_back(ptk::BvhMedianLevel{lv.first, lv.groups, lv.bits});
        med_n_tiles = (uint32_t)p.tiles.size(); med_index_bits = p.index_bits;
        med_n = (int64_t)r.n;
    }
    return PT_OK;
}

// Behind the records and k_scene_setup on the context's stream; nothing here (or in enqueue_refit) waits for the device.
int DeviceBvh::enqueue_build(const Rebuild& r, const ptbvh::Bounds& bd, const float4* shape, const uint32_t* tags, hipStream_t stream, ptk::SceneView& view) {
    ptk::BvhBuildArgs ba{};
    ba.shape = shape; ba.tags = tags;
    ba.pairs[0] = pairs[0].p; ba.pairs[1] = pairs[1].p; ba.hist = hist.p;
    ba.ids = ids.p; ba.rec = rec.p; ba.lead = lead.p;
    ba.n = r.n; ba.n_slots = r.slots;
    for (int k = 0; k < 3; ++k) { ba.grid_min[k] = bd.grid_min[k]; ba.grid_cell[k] = bd.grid_cell[k]; }
    if (r.nodes && r.median) {                   // (without a node there is no grid and no step: the order is the index order)
        ptk::BvhMedianArgs ma{};
        ma.b = ba;
        ma.cells = cells.p; ma.bounds = med_bounds.p; ma.group_start = med_groups.p;
        ma.tiles = med_tiles.p; ma.tile_steps = med_tsteps.p;
        ma.n_tiles = med_n_tiles; ma.index_bits = med_index_bits;
        if (ptk::launch_bvh_median(ma, med_levels.data(), (uint32_t)med_levels.size(), stream)) std::swap(ba.pairs[0], ba.pairs[1]);
    } else if (r.nodes) {                        // (... every key ties)
        ptk::launch_bvh_morton(ba, stream);
        ptk::launch_bvh_sort(ba, stream);
    }
    ptk::launch_bvh_write_ids(ba, r.nodes != 0, stream);
    if (!is_morton && r.nodes) {
        ptk::launch_bvh_codes(nodes.p, topo.codes.p, r.nodes, stream);
        HIP_TRY(hipMemcpyAsync(order.p, topo.order.p, (size_t)r.nodes * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    }
    if (!r.slots) HIP_TRY(hipMemsetAsync(cost_sums.p, 0, 3 * sizeof(unsigned long long), stream));   // (no leaf launch zeroes them)
    HIP_TRY(hipGetLastError());
    is_morton = true;
    height_first = topo.height_first;
    n_nodes = r.nodes; n_slots = r.slots; depth = topo.depth;
    bind(view, topo.root);
    has = true;
    refused = false; failed = false;
    return PT_OK;
}

int DeviceBvh::enqueue_refit(const ptbvh::Bounds& bd, const float4* shape, bool built, hipStream_t stream, ptk::SceneView& view) {
    ptk::BvhRefitArgs ra{};
    ra.shape = shape; ra.ids = ids.p; ra.rec = rec.p; ra.lead = lead.p;
    ra.slot_box = slot_box.p; ra.nodes = nodes.p; ra.node_box = node_box.p;
    ra.order = order.p; ra.cost = cost_sums.p;
    ra.n_slots = n_slots;
    for (int k = 0; k < 3; ++k) { ra.grid_min[k] = bd.grid_min[k]; ra.grid_cell[k] = bd.grid_cell[k]; }
    ptk::launch_bvh_refit_leaves(ra, stream);
    for (size_t h = 0; h + 1 < height_first.size(); ++h) ptk::launch_bvh_refit_level(ra, height_first[h], height_first[h + 1] - height_first[h], stream);
    HIP_TRY(hipGetLastError());
    set_grid(view, bd.grid_min, bd.grid_cell, bd.scene_abs);
    if (built) {
        // the cost of the tree as built stays on the device (cost() reads it there)
        HIP_TRY(hipMemcpyAsync(cost_built.p, cost_sums.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, stream));
        for (int k = 0; k < 3; ++k) cost_cell[k] = bd.grid_cell[k];
        cost_on_device = true;
        refits = 0;
    } else {
        ++refits;
    }
    return PT_OK;
}

int DeviceBvh::read(const ptk::SceneView& view, const BvhExport& out, uint32_t* out_nodes, uint32_t* out_slots) const {
    const size_t nn = out.nodes(n_nodes), ns = out.slots(n_slots);
    if (nn) HIP_TRY(hipMemcpy(out.qnodes, nodes.p, nn * 4 * sizeof(uint4), hipMemcpyDeviceToHost));
    if (ns) {
        HIP_TRY(hipMemcpy(out.leaf_rec, rec.p, ns * 3 * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out.leaf_lead, lead.p, ns * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out.leaf_ids, ids.p, ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (out.cost_now) HIP_TRY(hipMemcpy(out.cost_now, cost_sums.p, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (out_nodes) *out_nodes = n_nodes;
    if (out_slots) *out_slots = n_slots;
    out.scalars(view.bvh.grid_min, view.bvh.grid_cell, view.bvh.scene_abs, view.bvh.root);
    return PT_OK;
}

int DeviceBvh::cost(const ptk::SceneView& view, double* cost_now, double* cost_at_build, uint32_t* out_refits) const {
    uint64_t now[3];
    HIP_TRY(hipMemcpy(now, cost_sums.p, sizeof now, hipMemcpyDeviceToHost));
    if (cost_now) *cost_now = ptbvh::cost_value(now, view.bvh.grid_cell);
    if (cost_at_build) {
        *cost_at_build = cost_build;
        if (cost_on_device) {                    // a device build: the sums it left behind, in the grid of that build (I6)
            uint64_t built[3];
            HIP_TRY(hipMemcpy(built, cost_built.p, sizeof built, hipMemcpyDeviceToHost));
            *cost_at_build = ptbvh::cost_value(built, cost_cell);
        }
    }
    if (out_refits) *out_refits = refits;
    return PT_OK;
}
