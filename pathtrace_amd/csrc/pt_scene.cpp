// pt_scene.cpp -- the device half of a scene upload, in named stages (scene_set): the records of ptscene::build
// (pt_scene_records.h) into the context's buffers, k_scene_setup over them, the LDS blob; and what becomes of the BVH of the
// uploaded scene -- built at first use on the host (ensure_bvh), refitted on the device when the objects move (pt_scene_refit) or
// built there for the new pose (pt_scene_rebuild).  The tree itself, its state and its invariants: struct DeviceBvh (pt_scene_bvh.h).
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

// Build and upload the BVH of the uploaded scene (once per scene; a scene no tree is built for is remembered as such).
int ensure_bvh(PtContext* c) {
    if (c->tree.held()) return PT_OK;
    if (int rc = c->tree.why_not()) return rc;
    if (c->view.n_objs >= (1u << 28)) return fail(PT_ERR_UNSUPPORTED, "accel: %u objects exceed the 2^28 leaf slots", c->view.n_objs);
    const ptbvh::Built b = ptbvh::build(c->h_shape.data(), c->h_shape_tag.data(), c->view.n_objs);
    static_assert(ptbvh::kStackDepth == ptk::kBvhStack, "traversal stack depth");
    static_assert(ptbvh::kMaxLeaf == ptk::kBvhMaxLeaf, "leaf size the traversal unrolls for");
    if (b.non_finite) {
        c->tree.drop(c->view, true);
        return fail(PT_ERR_UNSUPPORTED, "accel: %u object(s) with a NaN/inf coordinate; the linear scan's answer for them "
                                        "depends on the scan order, use the linear scan", b.non_finite);
    }
    if (b.depth + 2u > ptbvh::kStackDepth || b.stack_need > ptbvh::kStackDepth) {
        c->tree.drop(c->view, false, true);      // a property of the scene: do not rebuild on every render
        return fail(PT_ERR_UNSUPPORTED, "accel: BVH (depth %u, stack need %u) exceeds the traversal stack", b.depth, b.stack_need);
    }
    return c->tree.adopt(b, c->stream, c->view);
}

namespace {

// The body of pt_scene_upload, pt_scene_update, pt_scene_refit, pt_scene_rebuild and pt_scene_rebuild_ordered, in the stages of
// scene_set below.  keep_history: same object count and shape tags as the uploaded scene, and the temporal history stays.  What
// becomes of the tree: kTreeDrop -- dropped, the next accel = 1 render builds it on the host; kTreeRefit (pt_scene_refit) -- a
// held tree is refitted on the device to the new records, same topology, so the tree arrays never cross PCIe again (DESIGN.md
// 5e); kTreeRebuild -- held or not, the context afterwards holds the tree of the new records in `order`, built on the device
// behind them (5f, 5i).  A pose with a NaN/inf coordinate takes the tree away for good, as ensure_bvh would on building it.
enum Tree { kTreeDrop, kTreeRefit, kTreeRebuild };
struct SceneJob {
    const char* who; const PtObject* objs; uint32_t n; bool keep_history; Tree tree; uint32_t order;
    // plan_scene's results: the records, the rebuild's plan, whether a held tree is refitted, the bounds of a refit or rebuild
    ptscene::Records rec;
    DeviceBvh::Rebuild rebuild;
    bool refit = false;
    ptbvh::Bounds bounds;
    bool rebuilds() const { return tree == kTreeRebuild && !bounds.non_finite; }
    bool refits() const { return refit && !bounds.non_finite; }
};

// CHECK: arguments, keep_history compatibility, order value.  Reads the context, touches nothing.
int check_job(const PtContext* c, const SceneJob& j) {
    const char* who = j.who;
    if (!c || (!j.objs && j.n)) return fail(PT_ERR_INVALID_ARG, "%s: null argument", who);
    if (j.order != PT_BVH_ORDER_MORTON && j.order != PT_BVH_ORDER_MEDIAN) return fail(PT_ERR_INVALID_ARG, "%s: order %u (PT_BVH_ORDER_MORTON or PT_BVH_ORDER_MEDIAN)", who, j.order);
    if (j.keep_history) {
        if (int rc = check_scene(c, who)) return rc;
        if (j.n != c->view.n_objs) return fail(PT_ERR_INVALID_ARG, "%s: %u objects, the uploaded scene has %u", who, j.n, c->view.n_objs);
        for (uint32_t i = 0; i < j.n; ++i)
            if (j.objs[i].shape_tag != c->h_shape_tag[i])
                return fail(PT_ERR_INVALID_ARG, "%s: object %u: shape_tag %u, the uploaded scene has %u", who, i, j.objs[i].shape_tag, c->h_shape_tag[i]);
    }
    return PT_OK;
}

// PLAN: the host work, every refusal of it before anything of the context or the device is touched -- the tree of a rebuild
// (a function of n: planned once per object count), the records, and the refit's share: one pass over the new gather records for
// the grid, scene_abs and the non-finite rule (the boxes ptbvh::refit would form; the kernels reproduce them bit for bit, so the
// grid encloses every box they quantise).  The thread's device is set between the two refusals, where it always was.
int plan_scene(PtContext* c, SceneJob& j) {
    if (j.tree == kTreeRebuild)
        if (int rc = c->tree.plan(j.n, j.order, j.who, &j.rebuild)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ptscene::build(j.objs, j.n, &j.rec)) return rc;
    j.refit = j.tree == kTreeRefit && c->tree.held();
    if (j.refit || j.tree == kTreeRebuild)
        j.bounds = ptbvh::scene_bounds(j.rec.shape.data(), j.rec.shape_tag.data(), j.n, j.refit ? c->tree.has_nodes() : j.rebuild.nodes != 0);
    return PT_OK;
}

// RESERVE: the scene's buffers, then the tree's.  A failure leaves the scene as it was; of the tree, see reserve_rebuild.
int reserve(PtContext* c, const SceneJob& j) {
    const ptscene::Records& r = j.rec;
    int rc;
    if ((rc = c->scan.ensure(r.scan.size() + 1))) return rc;
    if ((rc = c->shape.ensure(r.shape.size()))) return rc;
    if ((rc = c->mat.ensure(r.mat.size()))) return rc;
    if ((rc = c->shape_x.ensure(r.shape.size()))) return rc;
    if ((rc = c->mat_x.ensure(r.mat.size()))) return rc;
    if ((rc = c->runs.ensure(r.runs.size() + 1))) return rc;
    if ((rc = c->lights.ensure(r.lights.size() + 1))) return rc;
    if (!j.keep_history && (rc = c->shape_tag.ensure((size_t)j.n + 1))) return rc;
    if (j.refits() && (rc = c->tree.reserve_refit())) return rc;
    if (j.rebuilds() && (rc = c->tree.reserve_rebuild(j.rebuild, c->view))) return rc;
    return PT_OK;
}

// UPLOAD: wait for the previous scene's work, reset what belongs to it (scheduler, statistics, captured graphs), then the records,
// k_scene_setup over them, the LDS blob and the view's scene fields.
int upload(PtContext* c, const SceneJob& j) {
    const uint32_t n = j.n;
    const ptscene::Records& rec = j.rec;
    const std::vector<float4>&scan = rec.scan, &shape = rec.shape, &mat = rec.mat, &blob = rec.blob;
    const std::vector<ptk::Run>& runs = rec.runs;
    const std::vector<uint32_t>& lights = rec.lights;
    int rc;
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
    if (!j.keep_history && n) HIP_TRY(hipMemcpy(c->shape_tag.p, rec.shape_tag.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
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
    c->view.spheres_only = rec.spheres_only;
    c->view.lambert_surfaces = rec.lambert_surfaces;
    c->view.diffuse_only = rec.diffuse_only; c->view.no_mirror = rec.no_mirror; c->view.no_oren_nayar = rec.no_oren_nayar;
    c->split_ok = rec.split_ok;
    std::memcpy(c->scan_counts, rec.scan_counts, sizeof c->scan_counts);
    return PT_OK;
}

// TREE: build, refit or drop, on the context's stream behind the records (the stream is idle for the plan's copies).
int set_tree(PtContext* c, SceneJob& j) {
    if (j.rebuilds()) {
        if (int rc = c->tree.upload_plan(j.rebuild)) return rc;
        if (int rc = c->tree.enqueue_build(j.rebuild, j.bounds, c->shape.p, c->shape_tag.p, c->stream, c->view)) return rc;
    }
    if (j.refits() || j.rebuilds()) return c->tree.enqueue_refit(j.bounds, c->shape.p, j.rebuilds(), c->stream, c->view);
    c->tree.drop(c->view, (j.refit || j.tree == kTreeRebuild) && j.bounds.non_finite);
    return PT_OK;
}

// COMMIT: the host's copy of the scene, the pose and its generation, the history flags.
void commit(PtContext* c, SceneJob& j) {
    c->auto_bvh = j.rec.auto_bvh;
    c->h_shape.assign(j.rec.shape.begin(), j.rec.shape.begin() + 3 * (size_t)j.n);
    c->h_shape_tag = std::move(j.rec.shape_tag);
    c->has_scene = true;
    c->pose = std::move(j.rec.pose);
    ++c->pose_gen;
    if (!j.keep_history) {                    // a new scene starts the temporal history afresh; pt_scene_update keeps it
        c->tm_valid = false;
        c->gr_valid = false; c->gr_frame = 0;   // ... and pt_render_denoised_gradient's previous frame
    }
}

int scene_set(const char* who, PtContext* c, const PtObject* objs, uint32_t n, bool keep_history, Tree tree = kTreeDrop, uint32_t order = PT_BVH_ORDER_MORTON) {
    SceneJob j{who, objs, n, keep_history, tree, order, {}, {}, false, {}};
    int rc;
    if ((rc = check_job(c, j)) || (rc = plan_scene(c, j)) || (rc = reserve(c, j)) || (rc = upload(c, j)) || (rc = set_tree(c, j))) return rc;
    commit(c, j);
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
    if (!c->tree.held()) return fail(PT_ERR_INVALID_ARG, "pt_scene_bvh_cost: the context holds no BVH (none built yet, or dropped by a scene change)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->tree.cost(c->view, cost_now, cost_at_build, refits);
}

}  // extern "C"
