// pt_host.cpp -- the part of the C ABI that needs no device and no kernel object: the error channel, defaults, tile rows,
// the scene records of an upload (pt_scene_records.h), the motion maps and the table of path-kernel instances (the BVH verifier
// and its entries: pt_bvh_check.cpp).  The host-only sanitizer build (tests/tools/run_sanitizers.sh) compiles both files as
// they are: HIP headers for float4, no HIP library.
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
        // the surfaces a path can go on from: a hit on an Emissive that emits ends the path, so only a black one (the path goes on with
        // f = 0, pdf = 1, wo = n), OrenNayar or Mirror is a surface other than Lambertian
        if (o.mat_tag != PT_MAT_LAMBERT && !emits) r.lambert_surfaces = false;
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
    // the shape of the scan array a kernel may be compiled for: nothing but a few spheres (a fact of the object list, like the light count)
    r.spheres_only = runs.size() == 1 && runs[0].tag == ptk::kRunSphere && runs[0].off4 == 0 && runs[0].first_obj == 0 &&
                     runs[0].count == n && n <= ptk::kSpheresOnlyMax;
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

}  // extern "C"
