// pt_host.cpp -- the part of the C ABI that needs no device and no kernel object: the error channel, defaults, tile rows,
// the scene records of an upload (pt_scene_records.h), the BVH verifier and the host-side debug tables.  The host-only
// sanitizer build (tests/tools/run_sanitizers.sh) compiles this file as it is: HIP headers for float4, no HIP library.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "pt_bvh.h"
#include "pt_context.h"
#include "pt_motion.h"
#include "pt_scene_records.h"

thread_local std::string g_err;
// shared by every host file (pt_context.h: fail)
int pt_internal_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace ptscene {

// Shape records of one object: gather form (3 float4, pt_device.h) and scan records (1 float4 for a sphere, 3 for a triangle)
void shape_records(const PtObject& o, float4 gather[3], float4 scan[3], int* n_scan) {
    if (o.shape_tag == PT_SHAPE_SPHERE) {
        float4 s = make_float4((float)o.shape[0], (float)o.shape[1], (float)o.shape[2], (float)o.shape[3]);
        gather[0] = s;
        gather[1] = make_float4(1.0f / s.w, 0, 0, 0);       // 1/radius (shape.rs:86)
        gather[2] = make_float4(0, 0, 0, 0);
        s.w = s.w * s.w;                                     // scan record carries r^2 (shape.rs:63)
        scan[0] = s;
        *n_scan = 1;
    } else {
        float v0[3], v1[3], v2[3];
        for (int k = 0; k < 3; ++k) { v0[k] = (float)o.shape[k]; v1[k] = (float)o.shape[3 + k]; v2[k] = (float)o.shape[6 + k]; }
        gather[0] = make_float4(v0[0], v0[1], v0[2], 0.f);
        gather[1] = make_float4(v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2], 0.f);   // edge1, shape.rs:163
        gather[2] = make_float4(v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2], 0.f);   // edge2, shape.rs:164
        ptbvh::triangle_scan_record(gather[0], gather[1], gather[2], scan);       // plane + barycentric gradients (pt_bvh.h)
        *n_scan = 3;
    }
}

// World::new's tail (world.rs:213-225) + flattening of Box<dyn Shape>/Box<dyn Material>: everything pt_scene_upload and
// pt_scene_update compute on the host.
int build(const PtObject* objs, uint32_t n, Records* out) {
    Records r;
    std::vector<float4>&scan = r.scan, &shape = r.shape, &mat = r.mat;
    std::vector<ptk::Run>& runs = r.runs;
    std::vector<uint32_t>& lights = r.lights;
    shape.resize(3 * (size_t)n + 1); mat.resize(2 * (size_t)n + 1);
    std::vector<float4> obj_scan(3 * (size_t)n + 1);
    std::vector<int> obj_ns(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const PtObject& o = objs[i];
        if (o.shape_tag > PT_SHAPE_TRIANGLE) return fail(PT_ERR_INVALID_ARG, "object %u: bad shape_tag %u", i, o.shape_tag);
        if (o.mat_tag > PT_MAT_OREN_NAYAR) return fail(PT_ERR_INVALID_ARG, "object %u: bad mat_tag %u", i, o.mat_tag);
        shape_records(o, &shape[3 * (size_t)i], &obj_scan[3 * (size_t)i], &obj_ns[i]);
        float p[6] = {(float)o.mat[0], (float)o.mat[1], (float)o.mat[2], (float)o.mat[3], (float)o.mat[4], (float)o.mat[5]};
        uint32_t emits = 0;
        if (o.mat_tag == PT_MAT_EMISSIVE) {
            // emit().length() > 0 (world.rs:219-222), evaluated in f32
            float l2 = std::fmaf(p[2], p[2], std::fmaf(p[1], p[1], p[0] * p[0]));
            emits = std::sqrt(l2) > 0.0f ? 1u : 0u;
        }
        if (o.mat_tag == PT_MAT_OREN_NAYAR) {
            float s2 = p[3] * p[3];                              // OrenNayar::new, material.rs:182-193
            float A = 1.0f - 0.5f * s2 / (s2 + 0.33f);
            float B = 0.45f * s2 / (s2 + 0.09f);
            p[3] = A; p[4] = B; p[5] = 0.f;
        }
        uint32_t bits = o.mat_tag | (o.shape_tag << 8) | (emits << 16);
        float fb;
        std::memcpy(&fb, &bits, 4);
        mat[2 * (size_t)i] = make_float4(fb, p[0], p[1], p[2]);
        mat[2 * (size_t)i + 1] = make_float4(p[3], p[4], p[5], 0.f);
        if (emits) lights.push_back(i);
    }
    // Scan array: runs of same-kind primitives in object order (the order decides closest-hit ties, world.rs:281-287).
    // Two consecutive triangles whose records carry the SAME vertex v0 and the SAME plane normal bit for bit -- the two
    // halves of a parallelogram fanned from one corner, like every wall of World::new() (world.rs:82-182) -- form a PAIR:
    // determinant, t, the range test and the hit point are then literally the same numbers for both, and the scan
    // computes them once (tripair_test, pt_kernels_scan.h).  Nothing changes in any result.
    for (uint32_t i = 0; i < n;) {
        const bool tri = objs[i].shape_tag == PT_SHAPE_TRIANGLE;
        bool pair = false;
        if (tri && i + 1 < n && objs[i + 1].shape_tag == PT_SHAPE_TRIANGLE) {
            const float4 *a = &obj_scan[3 * (size_t)i], *b = &obj_scan[3 * (size_t)i + 3];
            pair = std::memcmp(&a[0], &b[0], 3 * sizeof(float)) == 0 && std::memcmp(&a[1], &b[1], 3 * sizeof(float)) == 0;   // n, v0
        }
        const uint32_t tag = !tri ? (uint32_t)ptk::kRunSphere : pair ? (uint32_t)ptk::kRunTrianglePair : (uint32_t)ptk::kRunTriangle;
        if (runs.empty() || runs.back().tag != tag) {
            ptk::Run run;
            run.tag = tag; run.first_obj = i; run.count = 0; run.off4 = (uint32_t)scan.size();
            runs.push_back(run);
        }
        runs.back().count++;
        if (!pair) scan.insert(scan.end(), &obj_scan[3 * (size_t)i], &obj_scan[3 * (size_t)i] + obj_ns[i]);
        if (pair) {
            // pair record, 5 float4 in the order tripair_test reads them: (n, -) (v0, -) and then the four barycentric gradients
            // back to back from a 16-byte boundary -- (N1, N2.x) (N2.y, N2.z, N1'.x, N1'.y) (N1'.z, N2') -- so that the part only
            // rays inside the pair's t range read is three aligned 16-byte reads (round 5; before: five 8-byte pieces)
            const float4 *a = &obj_scan[3 * (size_t)i], *b = &obj_scan[3 * (size_t)i + 3];
            scan.push_back(make_float4(a[0].x, a[0].y, a[0].z, 0.f));
            scan.push_back(make_float4(a[1].x, a[1].y, a[1].z, 0.f));
            scan.push_back(make_float4(a[0].w, a[1].w, a[2].x, a[2].y));
            scan.push_back(make_float4(a[2].z, a[2].w, b[0].w, b[1].w));
            scan.push_back(make_float4(b[2].x, b[2].y, b[2].z, b[2].w));
        }
        i += pair ? 2u : 1u;
    }
    for (const ptk::Run& run : runs) r.scan_counts[run.tag == ptk::kRunSphere ? 0 : run.tag == ptk::kRunTriangle ? 1 : 2] += run.count;
    r.has_blob = n <= ptk::kSmallObjs;
    if (r.has_blob) {
        // LDS image of a small scene: [scan | shape 3n | mat 2n | runs | lights (padded to 16 B)]
        std::vector<float4>& blob = r.blob;
        blob.assign(scan.begin(), scan.end());
        blob.insert(blob.end(), shape.begin(), shape.begin() + 3 * (size_t)n);
        blob.insert(blob.end(), mat.begin(), mat.begin() + 2 * (size_t)n);
        static_assert(sizeof(ptk::Run) == sizeof(float4), "Run must be one float4");
        for (const ptk::Run& run : runs) { float4 f; std::memcpy(&f, &run, sizeof f); blob.push_back(f); }
        for (size_t i = 0; i < lights.size(); i += 4) {
            uint32_t w[4] = {0, 0, 0, 0};
            for (size_t k = 0; k < 4 && i + k < lights.size(); ++k) w[k] = lights[i + k];
            float4 f; std::memcpy(&f, w, sizeof f); blob.push_back(f);
        }
    }
    uint64_t n_mirror = 0, tris = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (objs[i].mat_tag != PT_MAT_LAMBERT && objs[i].mat_tag != PT_MAT_EMISSIVE) r.diffuse_only = false;
        if (objs[i].mat_tag == PT_MAT_OREN_NAYAR) r.no_oren_nayar = false;
        n_mirror += objs[i].mat_tag == PT_MAT_MIRROR;
        tris += objs[i].shape_tag == PT_SHAPE_TRIANGLE;
    }
    r.split_ok = n_mirror != 0 && 2 * n_mirror <= n;   // k_paths_regen_split sets the Mirror vertices aside: worth it while they are the exception
    r.no_mirror = n_mirror == 0;
    r.auto_bvh = n > ptk::kSmallObjs && 2 * (uint64_t)(n - tris) + 5 * tris > 2 * (uint64_t)kAutoBvhWeight;
    r.shape_tag.resize(n);
    r.pose.resize(9 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        r.shape_tag[i] = objs[i].shape_tag;
        std::memcpy(&r.pose[9 * (size_t)i], objs[i].shape, 9 * sizeof(double));
    }
    *out = std::move(r);
    return PT_OK;
}
}  // namespace ptscene

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

}  // namespace

extern "C" {

const char* pt_last_error(void) { return g_err.c_str(); }
uint32_t pt_abi_version(void) { return PT_ABI_VERSION; }

void pt_default_params(PtRenderParams* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->spp = 3000;          // world.rs:18
    p->spp_offset = 0;
    p->min_depth = 4;       // rendering.rs:6
    p->max_depth = 50;      // rendering.rs:7
    p->integrator = PT_INTEGRATOR_MIS;   // Cargo.toml:7 default feature
    p->t_min = 0.001;       // rendering.rs:41
    p->band_rows = 0;
    p->band_index = 0;
    p->band_count = 1;
    p->max_paths_in_flight = 0;
    p->profile = 0;
    p->accel = PT_ACCEL_AUTO;
    p->n_devices = 1;
}

uint32_t pt_tile_rows(uint32_t height, uint32_t band_rows, uint32_t band_index, uint32_t band_count) {
    if (band_rows == 0) band_rows = height ? height : 1;
    if (band_count == 0) band_count = 1;
    uint32_t rows = 0;
    for (uint32_t y = 0; y < height; ++y) rows += (y / band_rows) % band_count == band_index;
    return rows;
}

void pt_default_denoise(PtDenoise* out) {
    if (!out) return;
    out->iterations = 5; out->sigma_l = 4.0f; out->sigma_n = 128.0f; out->sigma_d = 0.025f;
}

void pt_default_temporal(PtTemporal* out) {
    if (!out) return;
    out->alpha = 0.2f; out->depth_tol = 0.1f; out->normal_tol = 0.9f;
}

int pt_debug_motion_maps(const PtObject* prev_objs, const PtObject* cur_objs, uint32_t n, double* out_maps, uint32_t* out_flags) {
    if (n && (!prev_objs || !cur_objs || !out_maps || !out_flags)) return fail(PT_ERR_INVALID_ARG, "pt_debug_motion_maps: null argument");
    for (uint32_t i = 0; i < n; ++i) {
        if (prev_objs[i].shape_tag > PT_SHAPE_TRIANGLE || prev_objs[i].shape_tag != cur_objs[i].shape_tag)
            return fail(PT_ERR_INVALID_ARG, "pt_debug_motion_maps: object %u: shape tags %u and %u", i, prev_objs[i].shape_tag, cur_objs[i].shape_tag);
        out_flags[i] = ptmo::motion_map(cur_objs[i].shape_tag == PT_SHAPE_TRIANGLE, cur_objs[i].shape, prev_objs[i].shape, out_maps + 12 * (size_t)i);
    }
    return PT_OK;
}

// Debug: every instance code ptk::launch_paths_* can return -- the path-kernel instances the library is built with (the
// template arguments of the dispatch in pt_kernels_*.hip), each in both arithmetic modes.  *n = the table's length; up to cap
// codes are written (out may be null to ask for the length).
int pt_debug_path_instances(uint32_t* out, uint32_t cap, uint32_t* n) {
    if (!n || (!out && cap)) return fail(PT_ERR_INVALID_ARG, "null argument");
    std::vector<uint32_t> t;
    for (const bool exact : {true, false}) {
        for (const bool mis : {true, false}) {
            for (const bool ovf : {false, true}) {
                // k_paths<MODE, MIS, OVF, DIFFUSE, LIST>: the diffuse-only instances for whole-image renders out of LDS only
                t.push_back(ptk::instance_code(ptk::kInstPaths, ptk::kModeLds, mis, ovf, true, false, exact));
                for (const int mode : {ptk::kModeLds, ptk::kModeTiled})
                    for (const bool list : {false, true}) t.push_back(ptk::instance_code(ptk::kInstPaths, mode, mis, ovf, false, list, exact));
                // k_paths_bvh<MIS, OVF, DIFFUSE, LIST>: likewise
                t.push_back(ptk::instance_code(ptk::kInstBvh, 0, mis, ovf, true, false, exact));
                for (const bool list : {false, true}) t.push_back(ptk::instance_code(ptk::kInstBvh, 0, mis, ovf, false, list, exact));
            }
            // k_paths_regen<MIS, MATS, LIST> (level-0 launches only; LIST: pt_render_adaptive's passes)
            for (const int mats : {ptk::kMatsAll, ptk::kMatsDiffuse, ptk::kMatsNoMirror})
                for (const bool list : {false, true}) t.push_back(ptk::instance_code(ptk::kInstRegen, 0, mis, false, mats, list, exact));
            // k_paths_regen_split<MIS, PLAIN> (level-0 launches of whole images only)
            for (const int plain : {ptk::kMatsDiffuse, ptk::kMatsNoMirror})
                t.push_back(ptk::instance_code(ptk::kInstRegenSplit, 0, mis, false, plain, false, exact));
        }
    }
    for (size_t i = 0; i < t.size() && i < cap; ++i) out[i] = t[i];
    *n = (uint32_t)t.size();
    return PT_OK;
}

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
    if (n && (!prev_objs || !cur_objs)) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_refit_check: null objects");
    if ((cap_nodes && !out_qnodes) || (cap_slots && (!out_leaf_rec || !out_leaf_lead || !out_leaf_ids)))
        return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_refit_check: null output array with a non-zero capacity");
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
    const size_t nn = std::min<size_t>(b.wide.size(), cap_nodes), nsl = std::min<size_t>(b.leaf_ids.size(), cap_slots);
    if (nn) std::memcpy(out_qnodes, b.qnodes.data(), nn * 4 * sizeof(uint4));
    if (nsl) {
        std::memcpy(out_leaf_rec, b.leaf_rec.data(), nsl * 3 * sizeof(float4));
        std::memcpy(out_leaf_lead, b.leaf_lead.data(), nsl * sizeof(float4));
        std::memcpy(out_leaf_ids, b.leaf_ids.data(), nsl * sizeof(uint32_t));
    }
    if (out_grid) {
        for (int k = 0; k < 3; ++k) { out_grid[k] = b.grid_min[k]; out_grid[3 + k] = b.grid_cell[k]; }
        out_grid[6] = b.scene_abs;
    }
    if (root) *root = b.root;
    for (int k = 0; k < 3; ++k) {
        if (cost_now) cost_now[k] = b.cost[k];
        if (cost_at_build) cost_at_build[k] = cost0[k];
    }
    return PT_OK;
}

int pt_debug_bvh_morton_check(const PtObject* objs, const PtObject* refit_objs, uint32_t n, uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead,
                              uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid, uint32_t* root,
                              uint64_t* cost_now, uint32_t* out_keys, uint32_t* out_order, uint32_t cap_objs) {
    if (n && !objs) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_morton_check: null objects");
    if ((cap_nodes && !out_qnodes) || (cap_slots && (!out_leaf_rec || !out_leaf_lead || !out_leaf_ids)) || (cap_objs && (!out_keys || !out_order)))
        return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_morton_check: null output array with a non-zero capacity");
    std::vector<float4> shape, scan;
    std::vector<uint32_t> tag, keys, order;
    if (int rc = bvh_records("pt_debug_bvh_morton_check", objs, n, shape, scan, tag)) return rc;
    ptbvh::Built b;
    if (!ptbvh::build_morton(b, shape.data(), tag.data(), n, &keys, &order))
        return fail(PT_ERR_UNSUPPORTED, "pt_debug_bvh_morton_check: no tree over %u objects fits the traversal stack (%u entries)", n, ptbvh::kStackDepth);
    if (n_nodes) *n_nodes = (uint32_t)b.wide.size();
    if (n_slots) *n_slots = (uint32_t)b.leaf_ids.size();
    if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    if (refit_objs) {                                            // the tree of objs carried to another pose of the same objects
        for (uint32_t i = 0; i < n; ++i)
            if (objs[i].shape_tag != refit_objs[i].shape_tag)
                return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_morton_check: object %u: shape tags %u and %u", i, objs[i].shape_tag, refit_objs[i].shape_tag);
        if (int rc = bvh_records("pt_debug_bvh_morton_check", refit_objs, n, shape, scan, tag)) return rc;
        ptbvh::refit(b, shape.data(), tag.data(), n);
        if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    }
    // the order is ascending by (key, index), and slot p holds sorted position p
    for (uint32_t p = 0; p < n; ++p) {
        if (p && !(keys[order[p - 1]] < keys[order[p]] || (keys[order[p - 1]] == keys[order[p]] && order[p - 1] < order[p])))
            return fail(PT_ERR_UNSUPPORTED, "BVH build: sorted positions %u and %u are out of order", p - 1, p);
        if ((b.leaf_ids[p] & ~ptbvh::kTriangleBit) != order[p]) return fail(PT_ERR_UNSUPPORTED, "BVH build: slot %u does not hold sorted position %u", p, p);
    }
    const size_t nn = std::min<size_t>(b.wide.size(), cap_nodes), nsl = std::min<size_t>(b.leaf_ids.size(), cap_slots), no = std::min<size_t>(n, cap_objs);
    if (nn) std::memcpy(out_qnodes, b.qnodes.data(), nn * 4 * sizeof(uint4));
    if (nsl) {
        std::memcpy(out_leaf_rec, b.leaf_rec.data(), nsl * 3 * sizeof(float4));
        std::memcpy(out_leaf_lead, b.leaf_lead.data(), nsl * sizeof(float4));
        std::memcpy(out_leaf_ids, b.leaf_ids.data(), nsl * sizeof(uint32_t));
    }
    if (no) {
        std::memcpy(out_keys, keys.data(), no * sizeof(uint32_t));
        std::memcpy(out_order, order.data(), no * sizeof(uint32_t));
    }
    if (out_grid) {
        for (int k = 0; k < 3; ++k) { out_grid[k] = b.grid_min[k]; out_grid[3 + k] = b.grid_cell[k]; }
        out_grid[6] = b.scene_abs;
    }
    if (root) *root = b.root;
    for (int k = 0; k < 3; ++k)
        if (cost_now) cost_now[k] = b.cost[k];
    return PT_OK;
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

int pt_debug_bvh_median_check(const PtObject* objs, const PtObject* refit_objs, uint32_t n, uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead,
                              uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid, uint32_t* root,
                              uint64_t* cost_now, uint32_t* out_keys, uint32_t* out_order, uint32_t cap_objs) {
    if (n && !objs) return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_median_check: null objects");
    if ((cap_nodes && !out_qnodes) || (cap_slots && (!out_leaf_rec || !out_leaf_lead || !out_leaf_ids)) || (cap_objs && (!out_keys || !out_order)))
        return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_median_check: null output array with a non-zero capacity");
    std::vector<float4> shape, scan;
    std::vector<uint32_t> tag, g, order;
    if (int rc = bvh_records("pt_debug_bvh_median_check", objs, n, shape, scan, tag)) return rc;
    ptbvh::Built b;
    if (!ptbvh::build_median(b, shape.data(), tag.data(), n, &g, &order))
        return fail(PT_ERR_UNSUPPORTED, "pt_debug_bvh_median_check: no tree over %u objects fits the traversal stack (%u entries)", n, ptbvh::kStackDepth);
    if (n_nodes) *n_nodes = (uint32_t)b.wide.size();
    if (n_slots) *n_slots = (uint32_t)b.leaf_ids.size();
    if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    const float cell[3] = {b.grid_cell[0], b.grid_cell[1], b.grid_cell[2]};    // the grid of the build pose
    if (refit_objs) {                                            // the tree of objs carried to another pose of the same objects
        for (uint32_t i = 0; i < n; ++i)
            if (objs[i].shape_tag != refit_objs[i].shape_tag)
                return fail(PT_ERR_INVALID_ARG, "pt_debug_bvh_median_check: object %u: shape tags %u and %u", i, objs[i].shape_tag, refit_objs[i].shape_tag);
        if (int rc = bvh_records("pt_debug_bvh_median_check", refit_objs, n, shape, scan, tag)) return rc;
        ptbvh::refit(b, shape.data(), tag.data(), n);
        if (int rc = bvh_verify(b, shape, scan, tag, n)) return rc;
    }
    // the slots hold the order the rule gives: the steps once more, each as "the range in index order, then a stable sort by
    // the axis' coordinate" -- another route to the same total order
    {
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
    }
    const size_t nn = std::min<size_t>(b.wide.size(), cap_nodes), nsl = std::min<size_t>(b.leaf_ids.size(), cap_slots), no = std::min<size_t>(n, cap_objs);
    if (nn) std::memcpy(out_qnodes, b.qnodes.data(), nn * 4 * sizeof(uint4));
    if (nsl) {
        std::memcpy(out_leaf_rec, b.leaf_rec.data(), nsl * 3 * sizeof(float4));
        std::memcpy(out_leaf_lead, b.leaf_lead.data(), nsl * sizeof(float4));
        std::memcpy(out_leaf_ids, b.leaf_ids.data(), nsl * sizeof(uint32_t));
    }
    if (no) {
        std::memcpy(out_keys, g.data(), no * 3 * sizeof(uint32_t));
        std::memcpy(out_order, order.data(), no * sizeof(uint32_t));
    }
    if (out_grid) {
        for (int k = 0; k < 3; ++k) { out_grid[k] = b.grid_min[k]; out_grid[3 + k] = b.grid_cell[k]; }
        out_grid[6] = b.scene_abs;
    }
    if (root) *root = b.root;
    for (int k = 0; k < 3; ++k)
        if (cost_now) cost_now[k] = b.cost[k];
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
