// pt_debug.cpp -- the pt_debug_* entries that launch a kernel over the uploaded scene: closest hits, and one function of the
// device code per launch of k_debug_fn (BSDF, shape and light sampling, camera rays, the joint scan).
#include "pt_entry.h"

namespace {

int debug_hit_impl(PtContext* c, const double* rays, uint32_t n, double t_min, double t_max, uint32_t exact_math,
                   uint32_t accel, int32_t* out_id, float* out_t, float* out_rec) {
    if (!c || !rays || !out_id) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_scene(c, nullptr)) return rc;
    if (int rc = check_accel(accel)) return rc;
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (accel == PT_ACCEL_AUTO) {
        const std::string keep = g_err;
        accel = (c->auto_bvh && c->tree.may_build() && ensure_bvh(c) == PT_OK) ? PT_ACCEL_BVH : PT_ACCEL_LINEAR;
        if (!accel) g_err = keep;
    }
    if (accel) { int rb = ensure_bvh(c); if (rb) return rb; }
    std::vector<float> r6(6 * (size_t)n);
    for (size_t i = 0; i < r6.size(); ++i) r6[i] = (float)rays[i];
    DevBuf<float> d_r, d_t, d_rec;
    DevBuf<int32_t> d_id;
    DevBuf<float4> d_scratch;
    int rc;
    if ((rc = d_r.ensure(r6.size())) || (rc = d_id.ensure(n)) || (rc = d_t.ensure(n))) return rc;
    if (out_rec && (rc = d_rec.ensure(8 * (size_t)n))) return rc;
    if (accel && (rc = d_scratch.ensure(3 * (size_t)n))) return rc;
    HIP_TRY(hipMemcpy(d_r.p, r6.data(), r6.size() * sizeof(float), hipMemcpyHostToDevice));
    if (exact_math) ptk::launch_debug_hit_exact(view_for(c, 1), accel, d_r.p, n, (float)t_min, (float)t_max, d_scratch.p, d_id.p, d_t.p, d_rec.p, c->stream);
    else ptk::launch_debug_hit_fast(c->view, accel, d_r.p, n, (float)t_min, (float)t_max, d_scratch.p, d_id.p, d_t.p, d_rec.p, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out_id, d_id.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_t) HIP_TRY(hipMemcpy(out_t, d_t.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (out_rec) HIP_TRY(hipMemcpy(out_rec, d_rec.p, 8 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

// One launch of k_debug_fn: in = n * in_stride floats (host), words = n * 4 raw words or null, out = n * out_stride floats.
int debug_fn(PtContext* c, uint32_t op, uint32_t obj, const std::vector<float>& in, uint32_t in_stride, const uint32_t* words,
             uint32_t n, uint32_t out_stride, uint32_t exact_math, const PtCamera* cam, float* out) {
    if (!c || !out) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int rc = check_scene(c, nullptr)) return rc;
    if (op != ptk::kFnLightPoint && op != ptk::kFnCameraRay && obj >= c->view.n_objs)
        return fail(PT_ERR_INVALID_ARG, "object %u out of range (%u objects)", obj, c->view.n_objs);
    if (n == 0) return PT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = c->fn_in.ensure(in.size() + 1)) || (rc = c->fn_out.ensure((size_t)n * out_stride)) ||
        (rc = c->fn_words.ensure(4 * (size_t)n)))
        return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!in.empty()) HIP_TRY(hipMemcpy(c->fn_in.p, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
    if (words) HIP_TRY(hipMemcpy(c->fn_words.p, words, 4 * (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    ptk::DebugFnArgs a{};
    a.sc = view_for(c, exact_math);
    if (cam) {
        for (int k = 0; k < 3; ++k) {
            a.cam.origin[k] = (float)cam->origin[k]; a.cam.lower_left[k] = (float)cam->lower_left[k];
            a.cam.horizontal[k] = (float)cam->horizontal[k]; a.cam.vertical[k] = (float)cam->vertical[k];
        }
        a.cam.width = cam->width; a.cam.height = cam->height;
    }
    a.op = op; a.obj = obj; a.n = n; a.in_stride = in_stride; a.out_stride = out_stride;
    a.in = c->fn_in.p; a.words = words ? c->fn_words.p : nullptr; a.out = c->fn_out.p;
    if (exact_math) ptk::launch_debug_fn_exact(a, c->stream); else ptk::launch_debug_fn_fast(a, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->fn_out.p, (size_t)n * out_stride * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}
std::vector<float> to_f32(const double* p, size_t n) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (float)p[i];
    return v;
}

}  // namespace

// pt_debug_lens_rays, pt_debug_projection_rays and pt_debug_bake_rays behind their checks: the words, the source's debug form, the
// floats back
int debug_source_rays(PtContext* c, const ptk::RaySourceF& src, const uint32_t* xys, uint32_t n, uint32_t exact_math, uint32_t stride, float* out) {
    if (n == 0) return PT_OK;
    int rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = c->fn_out.ensure(stride * (size_t)n)) || (rc = c->fn_words.ensure(4 * (size_t)n))) return rc;
    std::vector<uint32_t> w(4 * (size_t)n, 0u);
    for (size_t i = 0; i < n; ++i) { w[4 * i] = xys[3 * i]; w[4 * i + 1] = xys[3 * i + 1]; w[4 * i + 2] = xys[3 * i + 2]; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->fn_words.p, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!ptk::launch_debug_source_rays(exact_math, src, c->fn_words.p, n, c->fn_out.p, c->stream))
        return fail(PT_ERR_INVALID_ARG, "ray source %u has no debug-ray kernel", src.tag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->fn_out.p, stride * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" {

int pt_debug_hit_scene(PtContext* c, const double* rays, uint32_t n, double t_min, double t_max, uint32_t exact_math,
                       uint32_t accel, int32_t* out_id, float* out_t) {
    if (!out_t) return fail(PT_ERR_INVALID_ARG, "null argument");
    return debug_hit_impl(c, rays, n, t_min, t_max, exact_math, accel, out_id, out_t, nullptr);
}
int pt_debug_hit_records(PtContext* c, const double* rays, uint32_t n, double t_min, double t_max, uint32_t exact_math,
                         uint32_t accel, int32_t* out_id, float* out_rec) {
    if (!out_rec) return fail(PT_ERR_INVALID_ARG, "null argument");
    return debug_hit_impl(c, rays, n, t_min, t_max, exact_math, accel, out_id, nullptr, out_rec);
}

int pt_debug_bsdf_eval(PtContext* c, uint32_t obj, const double* in10, uint32_t n, uint32_t exact_math, float* out4) {
    if (!in10 && n) return fail(PT_ERR_INVALID_ARG, "null argument");
    return debug_fn(c, ptk::kFnBsdfEval, obj, to_f32(in10, 10 * (size_t)n), 10, nullptr, n, 4, exact_math, nullptr, out4);
}
int pt_debug_bsdf_sample(PtContext* c, uint32_t obj, const double* in7, const uint32_t* words4, uint32_t n,
                         uint32_t exact_math, float* out8) {
    if ((!in7 || !words4) && n) return fail(PT_ERR_INVALID_ARG, "null argument");
    return debug_fn(c, ptk::kFnBsdfSample, obj, to_f32(in7, 7 * (size_t)n), 7, words4, n, 8, exact_math, nullptr, out8);
}
int pt_debug_shape_sample(PtContext* c, uint32_t obj, const double* from3, const double* target3, const double* r12,
                          uint32_t n, uint32_t exact_math, float* out8) {
    if ((!from3 || (!target3 && !r12)) && n) return fail(PT_ERR_INVALID_ARG, "null argument");
    std::vector<float> in(9 * (size_t)n, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) in[9 * i + k] = (float)from3[3 * i + k];
        if (target3) { for (int k = 0; k < 3; ++k) in[9 * i + 3 + k] = (float)target3[3 * i + k]; in[9 * i + 8] = 1.0f; }
        else { in[9 * i + 6] = (float)r12[2 * i]; in[9 * i + 7] = (float)r12[2 * i + 1]; }
    }
    return debug_fn(c, ptk::kFnShapeSample, obj, in, 9, nullptr, n, 8, exact_math, nullptr, out8);
}
int pt_debug_light_point(PtContext* c, const double* from3, const uint32_t* words4, uint32_t n, uint32_t exact_math,
                         float* out8) {
    if ((!from3 || !words4) && n) return fail(PT_ERR_INVALID_ARG, "null argument");
    return debug_fn(c, ptk::kFnLightPoint, 0, to_f32(from3, 3 * (size_t)n), 3, words4, n, 8, exact_math, nullptr, out8);
}
int pt_debug_camera_rays(PtContext* c, const PtCamera* cam, const uint32_t* xys, uint32_t n, uint32_t exact_math, float* out8) {
    if ((!cam || !xys) && n) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int rc = cam ? check_camera_size(cam) : PT_OK) return rc;
    std::vector<uint32_t> w(4 * (size_t)n, 0u);
    for (size_t i = 0; i < n; ++i) { w[4 * i] = xys[3 * i]; w[4 * i + 1] = xys[3 * i + 1]; w[4 * i + 2] = xys[3 * i + 2]; }
    return debug_fn(c, ptk::kFnCameraRay, 0, std::vector<float>(), 1, w.data(), n, 8, exact_math, cam, out8);
}

int pt_debug_joint_scan(PtContext* c, const double* rays10, uint32_t n, double t_min, double t_max_b, uint32_t exact_math, float* out6) {
    if (!rays10 && n) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (c && c->has_scene && (c->view.n_objs > ptk::kSmallObjs || c->view.blob_f4 == 0))
        return fail(PT_ERR_UNSUPPORTED, "pt_debug_joint_scan: the scene (%u objects) does not live in LDS", c->view.n_objs);
    std::vector<float> in(12 * (size_t)n);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 10; ++k) in[12 * i + k] = (float)rays10[10 * i + k];
        in[12 * i + 10] = (float)t_min; in[12 * i + 11] = (float)t_max_b;
    }
    return debug_fn(c, ptk::kFnJointScan, 0, in, 12, nullptr, n, 6, exact_math, nullptr, out6);
}

// The context's device tree, copied back (the outputs of pt_debug_bvh_refit_check: struct BvhExport; blocking)
int pt_debug_bvh_read(PtContext* c, uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead, uint32_t* out_leaf_ids,
                      uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid, uint32_t* root, uint64_t* cost_now) {
    const BvhExport out{out_qnodes, cap_nodes, out_leaf_rec, out_leaf_lead, out_leaf_ids, cap_slots, out_grid, root, cost_now};
    if (!c) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_read: null context");
    if (out.null_array()) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_read: null output array with a non-zero capacity");
    if (!c->tree.held()) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_read: the context holds no BVH");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->tree.read(c->view, out, n_nodes, n_slots);
}

}  // extern "C"
