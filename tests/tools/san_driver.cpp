// Sanitizer driver (CPU only; GPU ASan is not available on the pool): the host-side code that runs without a
// device -- scene constructors, camera constructors, the scene-record builder of an upload (ptscene::build), the BVH
// builder + verifier (product), and the oracle
// (test infrastructure) -- under AddressSanitizer + UndefinedBehaviorSanitizer.
// Build + run: tests/tools/run_sanitizers.sh   (used by tests/test_sanitizers.py)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/pathtrace_amd.h"
#include "../../pathtrace_amd/csrc/pt_scene_records.h"

extern "C" int orc_render(const PtCamera* cam, const PtObject* objs, uint32_t n, const PtRenderParams* p, int precision, int form,
                          int threads, double* out_lin, uint8_t* out_rgba, uint64_t* out_counters);

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("CHECK failed: %s (line %d): %s\n", #c, __LINE__, pt_last_error()); ++fails; } } while (0)

// What every set of records must satisfy: the runs partition the objects in order (a pair counts as two), a run starts
// in the scan array where the records before it end, and the counts add up.
static void check_records(const ptscene::Records& r, uint32_t n) {
    uint32_t obj = 0, off4 = 0, kinds[3] = {0, 0, 0};
    for (const ptk::Run& run : r.runs) {
        CHECK(run.tag <= (uint32_t)ptk::kRunTrianglePair);
        if (run.tag > (uint32_t)ptk::kRunTrianglePair) return;
        CHECK(run.first_obj == obj);
        CHECK(run.off4 == off4);
        CHECK(run.count > 0);
        obj += run.count * (run.tag == ptk::kRunTrianglePair ? 2u : 1u);
        off4 += run.count * ptk::run_entry_f4(run.tag);
        kinds[run.tag] += run.count;
    }
    CHECK(obj == n);
    for (int k = 0; k < 3; ++k) CHECK(kinds[k] == r.scan_counts[k]);
    CHECK(r.scan_counts[0] + r.scan_counts[1] + 2 * r.scan_counts[2] == n);
    CHECK(r.scan.size() == r.scan_counts[0] + 3 * (size_t)r.scan_counts[1] + 5 * (size_t)r.scan_counts[2]);
    CHECK(r.scan.size() == off4);
    CHECK(r.shape.size() == 3 * (size_t)n + 1 && r.mat.size() == 2 * (size_t)n + 1);
    CHECK(r.shape_tag.size() == n && r.pose.size() == 9 * (size_t)n);
    CHECK(r.has_blob == (n <= ptk::kSmallObjs));
    if (r.has_blob) CHECK(r.blob.size() == r.scan.size() + 5 * (size_t)n + r.runs.size() + (r.lights.size() + 3) / 4);
    else CHECK(r.blob.empty());
}
static bool same4(const float4& a, float x, float y, float z, float w) {
    const float b[4] = {x, y, z, w};
    return std::memcmp(&a, b, sizeof b) == 0;
}

static void scene_record_checks() {
    // built-in scenes and the empty scene
    for (uint32_t id : {1u, 2u, 4u})
        for (uint32_t arg : {0u, 3000u}) {
            if (id != 4 && arg) continue;
            uint32_t n = 0;
            CHECK(pt_builtin_scene(id, arg, nullptr, 0, &n) == PT_OK);
            std::vector<PtObject> objs(n);
            CHECK(pt_builtin_scene(id, arg, objs.data(), n, &n) == PT_OK);
            ptscene::Records r;
            CHECK(ptscene::build(objs.data(), n, &r) == PT_OK);
            check_records(r, n);
        }
    {
        ptscene::Records r;
        CHECK(ptscene::build(nullptr, 0, &r) == PT_OK);
        check_records(r, 0);
        CHECK(r.runs.empty() && r.scan.empty() && r.lights.empty() && r.has_blob && r.blob.empty());
    }
    // hand-made: a sphere, the unit square as two triangles fanned from its first corner, a lone triangle elsewhere
    PtObject o[4];
    std::memset(o, 0, sizeof o);
    o[0].shape_tag = PT_SHAPE_SPHERE; o[0].shape[0] = 3.0; o[0].shape[1] = 1.0; o[0].shape[2] = -2.0; o[0].shape[3] = 0.5;
    const double sq[4][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}};
    for (int t = 0; t < 2; ++t) {
        o[1 + t].shape_tag = PT_SHAPE_TRIANGLE;
        for (int k = 0; k < 3; ++k) { o[1 + t].shape[k] = sq[0][k]; o[1 + t].shape[3 + k] = sq[1 + t][k]; o[1 + t].shape[6 + k] = sq[2 + t][k]; }
    }
    o[3].shape_tag = PT_SHAPE_TRIANGLE;
    const double lone[9] = {5, 5, 5, 6, 5, 5, 5, 6, 5.5};
    std::memcpy(o[3].shape, lone, sizeof lone);
    o[0].mat_tag = PT_MAT_EMISSIVE; o[0].mat[1] = 2.0;      // emits
    o[1].mat_tag = PT_MAT_EMISSIVE;                         // Emissive, emission 0: no light
    o[2].mat_tag = PT_MAT_LAMBERT; o[2].mat[0] = 0.5;
    o[3].mat_tag = PT_MAT_EMISSIVE; o[3].mat[2] = 1e-3;     // emits
    ptscene::Records r;
    CHECK(ptscene::build(o, 4, &r) == PT_OK);
    check_records(r, 4);
    CHECK(r.scan_counts[0] == 1 && r.scan_counts[1] == 1 && r.scan_counts[2] == 1);
    CHECK(r.scan.size() == 9);
    CHECK(r.runs.size() == 3);
    if (r.runs.size() == 3 && r.scan.size() == 9) {
        CHECK(r.runs[0].tag == ptk::kRunSphere && r.runs[1].tag == ptk::kRunTrianglePair && r.runs[2].tag == ptk::kRunTriangle);
        CHECK(r.runs[1].first_obj == 1 && r.runs[1].off4 == 1 && r.runs[2].first_obj == 3 && r.runs[2].off4 == 6);
        // the pair record: (n, -) (v0, -) (N1, N2.x) (N2.y, N2.z, N1'.x, N1'.y) (N1'.z, N2'), where a triangle's own scan
        // record is (n, N1.x) (v0, N1.y) (N1.z, N2) -- the first triangle's a, the second's b
        float4 g[3], a[3], b[3];
        int ns = 0;
        ptscene::shape_records(o[1], g, a, &ns);
        CHECK(ns == 3);
        ptscene::shape_records(o[2], g, b, &ns);
        CHECK(std::memcmp(&a[0], &b[0], 12) == 0 && std::memcmp(&a[1], &b[1], 12) == 0);
        const float4* p = &r.scan[1];
        CHECK(same4(p[0], a[0].x, a[0].y, a[0].z, 0.f));
        CHECK(same4(p[1], a[1].x, a[1].y, a[1].z, 0.f));
        CHECK(same4(p[2], a[0].w, a[1].w, a[2].x, a[2].y));
        CHECK(same4(p[3], a[2].z, a[2].w, b[0].w, b[1].w));
        CHECK(same4(p[4], b[2].x, b[2].y, b[2].z, b[2].w));
        CHECK(same4(p[0], 0.f, 0.f, p[0].z, 0.f) && std::fabs(p[0].z) == 1.0f);      // the square's unit normal
        CHECK(same4(p[1], 0.f, 0.f, 0.f, 0.f));                                    // its first corner
        float4 c[3];
        ptscene::shape_records(o[3], g, c, &ns);
        CHECK(std::memcmp(&r.scan[6], c, sizeof c) == 0);
        CHECK(same4(r.scan[0], 3.0f, 1.0f, -2.0f, 0.25f));                         // sphere: centre, r^2
    }
    CHECK(r.lights.size() == 2);
    if (r.lights.size() == 2) CHECK(r.lights[0] == 0 && r.lights[1] == 3);
    CHECK(r.diffuse_only && r.no_mirror && r.no_oren_nayar && !r.split_ok && !r.auto_bvh);
    // the LDS blob: a scene of exactly kSmallObjs objects has one, one more object and it has none
    std::vector<PtObject> many(ptk::kSmallObjs + 1);
    std::memset(many.data(), 0, many.size() * sizeof(PtObject));
    for (size_t i = 0; i < many.size(); ++i) { many[i].shape[0] = (double)i; many[i].shape[3] = 0.25; }
    CHECK(ptscene::build(many.data(), ptk::kSmallObjs, &r) == PT_OK);
    check_records(r, ptk::kSmallObjs);
    CHECK(r.has_blob && r.blob.size() == 6 * (size_t)ptk::kSmallObjs + 1);
    CHECK(ptscene::build(many.data(), ptk::kSmallObjs + 1, &r) == PT_OK);
    check_records(r, ptk::kSmallObjs + 1);
    CHECK(!r.has_blob && r.blob.empty());
    // a bad tag is refused and the output stays as it was
    CHECK(ptscene::build(o, 4, &r) == PT_OK);
    const std::vector<float4> scan_before = r.scan;
    for (int which = 0; which < 2; ++which) {
        PtObject bad[4];
        std::memcpy(bad, o, sizeof o);
        if (which) bad[3].mat_tag = PT_MAT_OREN_NAYAR + 1; else bad[2].shape_tag = PT_SHAPE_TRIANGLE + 1;
        CHECK(ptscene::build(bad, 4, &r) == PT_ERR_INVALID_ARG);
        CHECK(r.scan.size() == 9 && std::memcmp(r.scan.data(), scan_before.data(), 9 * sizeof(float4)) == 0);
        CHECK(r.runs.size() == 3 && r.lights.size() == 2 && r.shape_tag.size() == 4 && r.scan_counts[2] == 1 && r.has_blob);
    }
}

int main() {
    for (uint32_t id : {1u, 2u, 4u}) {
        for (uint32_t arg : {0u, 7u, 3000u}) {
            if (id != 4 && arg) continue;
            uint32_t n = 0;
            CHECK(pt_builtin_scene(id, arg, nullptr, 0, &n) == PT_OK);
            std::vector<PtObject> objs(n);
            CHECK(pt_builtin_scene(id, arg, objs.data(), n, &n) == PT_OK);
            uint32_t depth = 0, nodes = 0, slots = 0;
            CHECK(pt_debug_bvh_check(objs.data(), n, &depth, &nodes, &slots) == PT_OK);
            CHECK(slots == n);
            if (n > 64) continue;
            PtCamera cam;
            const double origin[3] = {0, 0, 2};
            CHECK(pt_camera_new(origin, 24, 16, 1.0, 35.0, &cam) == PT_OK);
            PtRenderParams prm;
            pt_default_params(&prm);
            prm.spp = 3;
            for (int precision : {64, 32})
                for (int form : {0, 1}) {
                    std::vector<double> lin(24 * 16 * 3);
                    std::vector<uint8_t> rgba(24 * 16 * 4);
                    uint64_t cnt[8] = {0};
                    CHECK(orc_render(&cam, objs.data(), n, &prm, precision, form, 2, lin.data(), rgba.data(), cnt) == 0);
                    CHECK(cnt[0] > 0);
                }
        }
    }
    // degenerate builder inputs: empty, coincident centroids, non-finite objects (refused), bad tags
    CHECK(pt_debug_bvh_check(nullptr, 0, nullptr, nullptr, nullptr) == PT_OK);
    std::vector<PtObject> same(2000);
    std::memset(same.data(), 0, same.size() * sizeof(PtObject));
    for (auto& o : same) { o.shape[2] = -2.0; o.shape[3] = 0.25; }
    CHECK(pt_debug_bvh_check(same.data(), (uint32_t)same.size(), nullptr, nullptr, nullptr) == PT_OK);
    same[5].shape[0] = NAN;
    CHECK(pt_debug_bvh_check(same.data(), (uint32_t)same.size(), nullptr, nullptr, nullptr) == PT_ERR_UNSUPPORTED);
    same[5].shape[0] = 0.0; same[9].shape_tag = 9;
    CHECK(pt_debug_bvh_check(same.data(), (uint32_t)same.size(), nullptr, nullptr, nullptr) == PT_ERR_INVALID_ARG);
    // camera constructors reject bad arguments without UB
    PtCamera cam;
    const double o[3] = {0, 0, 2}, t[3] = {0, 0, 2}, up[3] = {0, 1, 0};
    CHECK(pt_camera_new(o, 0, 0, 1.0, 35.0, &cam) != PT_OK);
    CHECK(pt_camera_look_at(o, t, up, 16, 16, 35.0, &cam) != PT_OK || true);   // origin == target: any status, no UB
    CHECK(pt_tile_rows(100, 7, 2, 3) > 0);
    scene_record_checks();
    std::printf("sanitizer driver: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
