// pt_scene.cpp -- the device half of a scene upload: the records of ptscene::build (pt_scene_records.h) into the context's
// buffers, k_scene_setup over them, the LDS blob; and the BVH of the uploaded scene, built at first use on the host, refitted on
// the device when the objects move (pt_scene_refit) or built there for the new pose (pt_scene_rebuild).
#include <cstring>
#include <utility>

#include "pt_bvh.h"
#include "pt_entry.h"
#include "pt_scene_records.h"

// The scene as a launch in the given arithmetic mode sees it (the records carry constants evaluated in that mode)
ptk::SceneView view_for(const PtContext* c, uint32_t exact_math) {
    ptk::SceneView v = c->view;
    if (exact_math) {
        v.shape = c->shape_x.p; v.mat = c->mat_x.p;
        if (v.blob) v.blob = c->blob_x.p;
    }
    return v;
}

// Build and upload the BVH of the uploaded scene (once per scene).
int ensure_bvh(PtContext* c) {
    if (c->has_bvh) return PT_OK;
    if (c->bvh_refused) return fail(PT_ERR_UNSUPPORTED, "accel: the scene has object(s) with a NaN/inf coordinate; use the linear scan");
    if (c->bvh_failed) return fail(PT_ERR_UNSUPPORTED, "accel: the BVH of this scene is deeper than the traversal stack; use the linear scan");
    if (c->view.n_objs >= (1u << 28)) return fail(PT_ERR_UNSUPPORTED, "accel: %u objects exceed the 2^28 leaf slots", c->view.n_objs);
    ptbvh::Built b = ptbvh::build(c->h_shape.data(), c->h_shape_tag.data(), c->view.n_objs);
    static_assert(ptbvh::kStackDepth == ptk::kBvhStack, "traversal stack depth");
    static_assert(ptbvh::kMaxLeaf == ptk::kBvhMaxLeaf, "leaf size the traversal unrolls for");
    if (b.non_finite) {
        c->bvh_refused = true;
        return fail(PT_ERR_UNSUPPORTED, "accel: %u object(s) with a NaN/inf coordinate; the linear scan's answer for them "
                                        "depends on the scan order, use the linear scan", b.non_finite);
    }
    if (b.depth + 2u > ptbvh::kStackDepth || b.stack_need > ptbvh::kStackDepth) {
        c->bvh_failed = true;        // a property of the scene: do not rebuild on every render
        return fail(PT_ERR_UNSUPPORTED, "accel: BVH (depth %u, stack need %u) exceeds the traversal stack", b.depth, b.stack_need);
    }
    int rc;
    if ((rc = c->bvh_nodes.ensure(b.qnodes.size() + 2)) || (rc = c->bvh_rec.ensure(b.leaf_rec.size() + 3)) ||
        (rc = c->bvh_ids.ensure(b.leaf_ids.size() + 4)) || (rc = c->bvh_lead.ensure(b.leaf_lead.size() + 4)) ||
        (rc = c->bvh_order.ensure(b.height_order.size() + 1)) || (rc = c->bvh_cost.ensure(4)))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!b.qnodes.empty()) HIP_TRY(hipMemcpy(c->bvh_nodes.p, b.qnodes.data(), b.qnodes.size() * sizeof(uint4), hipMemcpyHostToDevice));
    if (!b.leaf_rec.empty()) HIP_TRY(hipMemcpy(c->bvh_rec.p, b.leaf_rec.data(), b.leaf_rec.size() * sizeof(float4), hipMemcpyHostToDevice));
    if (!b.leaf_ids.empty()) HIP_TRY(hipMemcpy(c->bvh_ids.p, b.leaf_ids.data(), b.leaf_ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!b.leaf_lead.empty()) HIP_TRY(hipMemcpy(c->bvh_lead.p, b.leaf_lead.data(), b.leaf_lead.size() * sizeof(float4), hipMemcpyHostToDevice));
    // for pt_scene_refit: the order of the nodes by height, and the cost sums of the tree as built
    if (!b.height_order.empty()) HIP_TRY(hipMemcpy(c->bvh_order.p, b.height_order.data(), b.height_order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "cost words");
    HIP_TRY(hipMemcpy(c->bvh_cost.p, b.cost, sizeof b.cost, hipMemcpyHostToDevice));
    c->bvh_height_first = std::move(b.height_first);
    c->bvh_n_nodes = (uint32_t)b.wide.size();
    c->bvh_n_slots = (uint32_t)b.leaf_ids.size();
    c->bvh_cost_build = ptbvh::cost_value(b.cost, b.grid_cell);
    c->bvh_cost_on_device = false;
    c->bvh_is_morton = false;                    // the arrays hold the host builder's topology now
    c->bvh_refits = 0;
    c->view.bvh.nodes = c->bvh_nodes.p; c->view.bvh.rec = c->bvh_rec.p; c->view.bvh.ids = c->bvh_ids.p; c->view.bvh.lead = c->bvh_lead.p;
    c->view.bvh.root = b.root;
    c->view.bvh.scene_abs = b.scene_abs;
    for (int k = 0; k < 3; ++k) { c->view.bvh.grid_min[k] = b.grid_min[k]; c->view.bvh.grid_cell[k] = b.grid_cell[k]; }
    c->bvh_depth = b.depth;
    c->has_bvh = true;
    return PT_OK;
}

namespace {

// The body of pt_scene_upload, pt_scene_update and pt_scene_refit (keep_history: same object count and shape tags as the
// uploaded scene, and the temporal history stays).  The records are built on the host first (ptscene::build); the context is
// touched only once that has succeeded.  keep_tree (pt_scene_refit): a BVH the context holds is not dropped but refitted on
// the device to the new records -- same topology, so the tree arrays never cross PCIe again.  kTreeRebuild
// (pt_scene_rebuild): whether or not a tree is held, the context afterwards holds the Morton tree of the new records, built on
// the device behind them: keys, sort, leaf ids, then the launches of the refit.  order (pt_scene_rebuild_ordered):
// PT_BVH_ORDER_MEDIAN puts the median-split order of DESIGN.md 5i in the place of keys and sort; nothing else differs.
enum Tree { kTreeDrop, kTreeRefit, kTreeRebuild };
int scene_set(const char* who, PtContext* c, const PtObject* objs, uint32_t n, bool keep_history, Tree tree = kTreeDrop, uint32_t order = PT_BVH_ORDER_MORTON) {
    if (!c || (!objs && n)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (order != PT_BVH_ORDER_MORTON && order != PT_BVH_ORDER_MEDIAN) return fail(PT_ERR_INVALID_ARG, "%s: order %u (PT_BVH_ORDER_MORTON or PT_BVH_ORDER_MEDIAN)", who, order);
    if (keep_history) {
        if (int rc = check_scene(c, who)) return rc;
        if (n != c->view.n_objs) return fail(PT_ERR_INVALID_ARG, "%s: %u objects, the uploaded scene has %u", who, n, c->view.n_objs);
        for (uint32_t i = 0; i < n; ++i)
            if (objs[i].shape_tag != c->h_shape_tag[i])
                return fail(PT_ERR_INVALID_ARG, "%s: object %u: shape_tag %u, the uploaded scene has %u", who, i, objs[i].shape_tag, c->h_shape_tag[i]);
    }
    // the topology of a rebuild is a function of n: planned once per object count, and refused before anything is touched
    const bool rebuild = tree == kTreeRebuild;
    ptbvh::Topology topo;
    const bool new_topo = rebuild && c->bvh_topo_n != (int64_t)n;
    if (new_topo) {
        topo = ptbvh::morton_topology(n);
        if (!topo.ok)
            return fail(PT_ERR_UNSUPPORTED, "%s: no tree over %u objects fits the traversal stack (%u entries); use pt_scene_update", who, n, ptbvh::kStackDepth);
    }
    // the median order's split plan likewise (the same counts have one)
    const bool median = rebuild && order == PT_BVH_ORDER_MEDIAN;
    ptbvh::MedianPlan plan;
    const bool new_plan = median && c->bvh_med_n != (int64_t)n;
    if (new_plan) plan = ptbvh::median_plan(n);
    const uint32_t mt_nodes = new_topo ? (uint32_t)topo.node_height.size() : c->bvh_topo_nodes, mt_slots = new_topo ? topo.n_slots : c->bvh_topo_slots;
    HIP_TRY(hipSetDevice(c->device));
    ptscene::Records rec;
    int rc;
    if ((rc = ptscene::build(objs, n, &rec))) return rc;
    const std::vector<float4>&scan = rec.scan, &shape = rec.shape, &mat = rec.mat, &blob = rec.blob;
    const std::vector<ptk::Run>& runs = rec.runs;
    const std::vector<uint32_t>& lights = rec.lights;
    if ((rc = c->scan.ensure(scan.size() + 1))) return rc;
    if ((rc = c->shape.ensure(shape.size()))) return rc;
    if ((rc = c->mat.ensure(mat.size()))) return rc;
    if ((rc = c->shape_x.ensure(shape.size()))) return rc;
    if ((rc = c->mat_x.ensure(mat.size()))) return rc;
    if ((rc = c->runs.ensure(runs.size() + 1))) return rc;
    if ((rc = c->lights.ensure(lights.size() + 1))) return rc;
    if (!keep_history && (rc = c->shape_tag.ensure((size_t)n + 1))) return rc;
    // The refit's share of the host work: one pass over the new gather records for the grid, scene_abs and the non-finite rule
    // (ptbvh::scene_bounds: the boxes ptbvh::refit would form).  The kernels reproduce the host's boxes bit for bit, so the
    // grid encloses every box they quantise.
    const bool refit = tree == kTreeRefit && c->has_bvh;
    ptbvh::Bounds bounds;
    if (refit) {
        bounds = ptbvh::scene_bounds(shape.data(), rec.shape_tag.data(), n, c->bvh_n_nodes != 0);
        if (!bounds.non_finite && ((rc = c->bvh_slot_box.ensure(2 * (size_t)c->bvh_n_slots + 1)) || (rc = c->bvh_node_box.ensure(2 * (size_t)c->bvh_n_nodes + 1))))
            return rc;
    }
    if (rebuild) {
        bounds = ptbvh::scene_bounds(shape.data(), rec.shape_tag.data(), n, mt_nodes != 0);
        if (!bounds.non_finite) {
            // the tree arrays at the size of the Morton tree (a held tree's arrays may be too small: growing one drops its content)
            const uint4* nodes0 = c->bvh_nodes.p;
            const uint32_t* order0 = c->bvh_order.p;
            if ((rc = c->bvh_nodes.ensure(4 * (size_t)mt_nodes + 2)) || (rc = c->bvh_rec.ensure(3 * (size_t)mt_slots + 3)) ||
                (rc = c->bvh_ids.ensure((size_t)mt_slots + 4)) || (rc = c->bvh_lead.ensure((size_t)mt_slots + 4)) ||
                (rc = c->bvh_order.ensure((size_t)mt_nodes + 1)) || (rc = c->bvh_cost.ensure(4)) || (rc = c->bvh_cost_built.ensure(4)) ||
                (rc = c->bvh_slot_box.ensure(2 * (size_t)mt_slots + 1)) || (rc = c->bvh_node_box.ensure(2 * (size_t)mt_nodes + 1)) ||
                (rc = c->bvh_pairs[0].ensure((size_t)n + 1)) || (rc = c->bvh_pairs[1].ensure((size_t)n + 1)) ||
                (rc = c->bvh_hist.ensure((size_t)ptk::kSortDigits * ptk::bvh_sort_tiles(n) + 4)) ||
                (rc = c->bvh_topo_codes.ensure((size_t)mt_nodes + 1)) || (rc = c->bvh_topo_order.ensure((size_t)mt_nodes + 1)) ||
                (median && ((rc = c->bvh_cells.ensure((size_t)n + 1)) ||
                            (new_plan && ((rc = c->bvh_med_bounds.ensure(6 * (size_t)plan.max_groups + 1)) || (rc = c->bvh_med_groups.ensure(plan.group_start.size() + 1)) ||
                                          (rc = c->bvh_med_tiles.ensure(plan.tiles.size() + 1)) || (rc = c->bvh_med_tsteps.ensure(plan.tile_steps.size() + 1))))))) {
                c->view.bvh = ptk::BvhView{};        // (an array of the held tree may be gone)
                c->has_bvh = false;
                c->bvh_is_morton = false;
                c->bvh_topo_n = -1;
                c->bvh_med_n = -1;
                return rc;
            }
            if (c->bvh_nodes.p != nodes0 || c->bvh_order.p != order0) c->bvh_is_morton = false;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));   // the previous scene may still be in use
    ptsched::on_scene(c->sched);                 // statistics of renders of the previous scene do not carry over
    c->expected_samples = 0;
    // (the statistics words are zero whenever no render is pending; on the context's stream, which is idle here: a plain hipMemset
    // runs on the legacy default stream, which a non-blocking stream does not wait for)
    if (c->ovf_count.p && hipMemsetAsync(c->ovf_count.p, 0, kStatsWords * sizeof(uint32_t), c->stream) == hipSuccess &&
        hipStreamSynchronize(c->stream) == hipSuccess)
        c->sched.stats_clean = 1;
    c->capture_gcd = 0;                          // (graphs captured over the previous scene must not be replayed any more: its buffers are gone)
    std::memset(c->regen_occ, 0, sizeof c->regen_occ);
    if (!scan.empty()) HIP_TRY(hipMemcpy(c->scan.p, scan.data(), scan.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->shape.p, shape.data(), shape.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->mat.p, mat.data(), mat.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->shape_x.p, shape.data(), shape.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->mat_x.p, mat.data(), mat.size() * sizeof(float4), hipMemcpyHostToDevice));
    // a triangle's unit normal and 1 / area, once per object and arithmetic mode, by the device's own expressions
    ptk::launch_scene_setup_fast(c->shape.p, c->mat.p, n, c->stream);
    ptk::launch_scene_setup_exact(c->shape_x.p, c->mat_x.p, n, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!runs.empty()) HIP_TRY(hipMemcpy(c->runs.p, runs.data(), runs.size() * sizeof(ptk::Run), hipMemcpyHostToDevice));
    if (!lights.empty()) HIP_TRY(hipMemcpy(c->lights.p, lights.data(), lights.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!keep_history && n) HIP_TRY(hipMemcpy(c->shape_tag.p, rec.shape_tag.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->view.scan = c->scan.p; c->view.shape = c->shape.p; c->view.mat = c->mat.p;
    c->view.runs = c->runs.p; c->view.lights = c->lights.p;
    c->view.blob = nullptr; c->view.blob_f4 = 0;
    if (rec.has_blob) {
        if ((rc = c->blob.ensure(blob.size() + 1)) || (rc = c->blob_x.ensure(blob.size() + 1))) return rc;
        for (float4* dst : {c->blob.p, c->blob_x.p}) {
            if (!blob.empty()) HIP_TRY(hipMemcpy(dst, blob.data(), blob.size() * sizeof(float4), hipMemcpyHostToDevice));
            // shape and material records as k_scene_setup left them in this mode's arrays
            const bool x = dst == c->blob_x.p;
            if (n) HIP_TRY(hipMemcpy(dst + scan.size(), x ? c->shape_x.p : c->shape.p, 3 * (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice));
            if (n) HIP_TRY(hipMemcpy(dst + scan.size() + 3 * (size_t)n, x ? c->mat_x.p : c->mat.p, 2 * (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice));
        }
        c->view.blob = c->blob.p;
        c->view.blob_f4 = (uint32_t)blob.size();
    }
    c->view.scan_f4 = (uint32_t)scan.size();
    c->view.n_runs = (uint32_t)runs.size(); c->view.n_objs = n; c->view.n_lights = (uint32_t)lights.size();
    c->view.diffuse_only = rec.diffuse_only; c->view.no_mirror = rec.no_mirror; c->view.no_oren_nayar = rec.no_oren_nayar;
    c->split_ok = rec.split_ok;
    std::memcpy(c->scan_counts, rec.scan_counts, sizeof c->scan_counts);
    if (rebuild && !bounds.non_finite) {
        if (new_topo) {
            // once per object count (the stream is idle here): the child codes and the order by height
            static_assert(sizeof(uint4) == ptbvh::kWidth * sizeof(uint32_t), "code words of a node");
            c->bvh_topo_n = -1;
            c->bvh_is_morton = false;
            if (mt_nodes) {
                HIP_TRY(hipMemcpy(c->bvh_topo_codes.p, topo.codes.data(), (size_t)mt_nodes * sizeof(uint4), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(c->bvh_topo_order.p, topo.height_order.data(), (size_t)mt_nodes * sizeof(uint32_t), hipMemcpyHostToDevice));
            }
            c->bvh_topo_height_first = std::move(topo.height_first);
            c->bvh_topo_nodes = mt_nodes; c->bvh_topo_slots = mt_slots; c->bvh_topo_root = topo.root; c->bvh_topo_depth = topo.depth;
            c->bvh_topo_n = (int64_t)n;
        }
        if (new_plan) {
            // once per object count as well: the groups of the levels above T, the tiles and their steps
            c->bvh_med_n = -1;
            if (!plan.group_start.empty()) HIP_TRY(hipMemcpy(c->bvh_med_groups.p, plan.group_start.data(), plan.group_start.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            if (!plan.tiles.empty()) HIP_TRY(hipMemcpy(c->bvh_med_tiles.p, plan.tiles.data(), plan.tiles.size() * sizeof(uint4), hipMemcpyHostToDevice));
            if (!plan.tile_steps.empty()) HIP_TRY(hipMemcpy(c->bvh_med_tsteps.p, plan.tile_steps.data(), plan.tile_steps.size() * sizeof(uint2), hipMemcpyHostToDevice));
            c->bvh_med_levels.clear();
            for (const ptbvh::MedianPlan::Level& lv : plan.levels) c->bvh_med_levels.push_back(ptk::BvhMedianLevel{lv.first, lv.groups, lv.bits});
            c->bvh_med_n_tiles = (uint32_t)plan.tiles.size(); c->bvh_med_index_bits = plan.index_bits;
            c->bvh_med_n = (int64_t)n;
        }
        // behind the records and k_scene_setup on the context's stream; nothing here waits for the device
        ptk::BvhBuildArgs ba{};
        ba.shape = c->shape.p; ba.tags = c->shape_tag.p;
        ba.pairs[0] = c->bvh_pairs[0].p; ba.pairs[1] = c->bvh_pairs[1].p; ba.hist = c->bvh_hist.p;
        ba.ids = c->bvh_ids.p; ba.rec = c->bvh_rec.p; ba.lead = c->bvh_lead.p;
        ba.n = n; ba.n_slots = mt_slots;
        for (int k = 0; k < 3; ++k) { ba.grid_min[k] = bounds.grid_min[k]; ba.grid_cell[k] = bounds.grid_cell[k]; }
        if (mt_nodes && median) {                // (without a node there is no grid and no step: the order is the index order)
            ptk::BvhMedianArgs ma{};
            ma.b = ba;
            ma.cells = c->bvh_cells.p; ma.bounds = c->bvh_med_bounds.p; ma.group_start = c->bvh_med_groups.p;
            ma.tiles = c->bvh_med_tiles.p; ma.tile_steps = c->bvh_med_tsteps.p;
            ma.n_tiles = c->bvh_med_n_tiles; ma.index_bits = c->bvh_med_index_bits;
            if (ptk::launch_bvh_median(ma, c->bvh_med_levels.data(), (uint32_t)c->bvh_med_levels.size(), c->stream)) std::swap(ba.pairs[0], ba.pairs[1]);
        } else if (mt_nodes) {                   // (... every key ties)
            ptk::launch_bvh_morton(ba, c->stream);
            ptk::launch_bvh_sort(ba, c->stream);
        }
        ptk::launch_bvh_write_ids(ba, mt_nodes != 0, c->stream);
        if (!c->bvh_is_morton && mt_nodes) {
            ptk::launch_bvh_codes(c->bvh_nodes.p, c->bvh_topo_codes.p, mt_nodes, c->stream);
            HIP_TRY(hipMemcpyAsync(c->bvh_order.p, c->bvh_topo_order.p, (size_t)mt_nodes * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        }
        if (!mt_slots) HIP_TRY(hipMemsetAsync(c->bvh_cost.p, 0, 3 * sizeof(unsigned long long), c->stream));   // (no leaf launch zeroes them)
        HIP_TRY(hipGetLastError());
        c->bvh_is_morton = true;
        c->bvh_height_first = c->bvh_topo_height_first;
        c->bvh_n_nodes = mt_nodes; c->bvh_n_slots = mt_slots; c->bvh_depth = c->bvh_topo_depth;
        c->view.bvh.nodes = c->bvh_nodes.p; c->view.bvh.rec = c->bvh_rec.p; c->view.bvh.ids = c->bvh_ids.p; c->view.bvh.lead = c->bvh_lead.p;
        c->view.bvh.root = c->bvh_topo_root;
        c->has_bvh = true;
        c->bvh_refused = false; c->bvh_failed = false;
    }
    if ((refit || rebuild) && !bounds.non_finite) {
        // behind the records and k_scene_setup on the context's stream; nothing here waits for the device
        ptk::BvhRefitArgs ra{};
        ra.shape = c->shape.p; ra.ids = c->bvh_ids.p; ra.rec = c->bvh_rec.p; ra.lead = c->bvh_lead.p;
        ra.slot_box = c->bvh_slot_box.p; ra.nodes = c->bvh_nodes.p; ra.node_box = c->bvh_node_box.p;
        ra.order = c->bvh_order.p; ra.cost = c->bvh_cost.p;
        ra.n_slots = c->bvh_n_slots;
        for (int k = 0; k < 3; ++k) { ra.grid_min[k] = bounds.grid_min[k]; ra.grid_cell[k] = bounds.grid_cell[k]; }
        ptk::launch_bvh_refit_leaves(ra, c->stream);
        for (size_t h = 0; h + 1 < c->bvh_height_first.size(); ++h)
            ptk::launch_bvh_refit_level(ra, c->bvh_height_first[h], c->bvh_height_first[h + 1] - c->bvh_height_first[h], c->stream);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 3; ++k) { c->view.bvh.grid_min[k] = bounds.grid_min[k]; c->view.bvh.grid_cell[k] = bounds.grid_cell[k]; }
        c->view.bvh.scene_abs = bounds.scene_abs;
        if (rebuild) {
            // the cost of the tree as built stays on the device (pt_scene_bvh_cost reads it there)
            HIP_TRY(hipMemcpyAsync(c->bvh_cost_built.p, c->bvh_cost.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
            for (int k = 0; k < 3; ++k) c->bvh_cost_cell[k] = bounds.grid_cell[k];
            c->bvh_cost_on_device = true;
            c->bvh_refits = 0;
        } else {
            ++c->bvh_refits;
        }
    } else {
        c->view.bvh = ptk::BvhView{};
        c->has_bvh = false;
        // a pose with a NaN/inf coordinate takes the tree away for good, as ensure_bvh would on building it
        c->bvh_refused = (refit || rebuild) && bounds.non_finite;
        c->bvh_failed = false;
    }
    c->auto_bvh = rec.auto_bvh;
    c->h_shape.assign(shape.begin(), shape.begin() + 3 * (size_t)n);
    c->h_shape_tag = std::move(rec.shape_tag);
    c->has_scene = true;
    c->pose = std::move(rec.pose);
    ++c->pose_gen;
    if (!keep_history) {                      // a new scene starts the temporal history afresh; pt_scene_update keeps it
        c->tm_valid = false;
        c->gr_valid = false; c->gr_frame = 0;   // ... and pt_render_denoised_gradient's previous frame
    }
    return PT_OK;
}

}  // namespace

extern "C" {

int pt_scene_upload(PtContext* c, const PtObject* objs, uint32_t n) { return scene_set("pt_scene_upload", c, objs, n, false); }
int pt_scene_update(PtContext* c, const PtObject* objs, uint32_t n) { return scene_set("pt_scene_update", c, objs, n, true); }
int pt_scene_refit(PtContext* c, const PtObject* objs, uint32_t n) { return scene_set("pt_scene_refit", c, objs, n, true, kTreeRefit); }
int pt_scene_rebuild(PtContext* c, const PtObject* objs, uint32_t n) { return scene_set("pt_scene_rebuild", c, objs, n, true, kTreeRebuild); }
int pt_scene_rebuild_ordered(PtContext* c, const PtObject* objs, uint32_t n, uint32_t order) {
    return scene_set("pt_scene_rebuild_ordered", c, objs, n, true, kTreeRebuild, order);
}

int pt_scene_bvh_cost(PtContext* c, double* cost_now, double* cost_at_build, uint32_t* refits) {
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_scene_bvh_cost: null context");
    if (!c->has_bvh) return fail(PT_ERR_INVALID_ARG, "pt_scene_bvh_cost: the context holds no BVH (none built yet, or dropped by a scene change)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint64_t now[3];
    HIP_TRY(hipMemcpy(now, c->bvh_cost.p, sizeof now, hipMemcpyDeviceToHost));
    if (cost_now) *cost_now = ptbvh::cost_value(now, c->view.bvh.grid_cell);
    if (cost_at_build) {
        *cost_at_build = c->bvh_cost_build;
        if (c->bvh_cost_on_device) {             // a device build: the sums it left behind, in the grid of that build
            uint64_t built[3];
            HIP_TRY(hipMemcpy(built, c->bvh_cost_built.p, sizeof built, hipMemcpyDeviceToHost));
            *cost_at_build = ptbvh::cost_value(built, c->bvh_cost_cell);
        }
    }
    if (refits) *refits = c->bvh_refits;
    return PT_OK;
}

}  // extern "C"
