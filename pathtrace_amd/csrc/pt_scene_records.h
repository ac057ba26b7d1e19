// pt_scene_records.h -- the host half of a scene upload: PtObject[] -> the records the device reads.  Pure host arithmetic
// (pt_host.cpp), no device and no context in sight; pt_scene.cpp uploads the result, the sanitizer driver checks it.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/pathtrace_amd.h"
#include "pt_kernels.h"

namespace ptscene {

// PT_ACCEL_AUTO: the BVH when the scene is larger than one LDS blob and spheres + 2.5 x triangles > 512 (C4-like
// scenes: the tiled scan costs ~0.11 ms per sphere and 67 M samples -- a Moeller-Trumbore test 2.5x that --, the BVH
// ~70 ms flat -> break-even near 600 sphere tests)
constexpr uint32_t kAutoBvhWeight = 512;

struct Records {
    std::vector<float4> scan;         // runs of same-kind primitives: 1 float4 per sphere, 3 per single triangle, 5 per triangle pair
    std::vector<float4> shape, mat;   // gather form: 3 and 2 float4 per object (+ 1 of padding)
    std::vector<ptk::Run> runs;
    std::vector<uint32_t> lights;     // the Emissive objects with non-zero emission
    std::vector<float4> blob;         // has_blob: the LDS image [scan | shape 3n | mat 2n | runs | lights (padded to 16 B)]
    std::vector<uint32_t> shape_tag;
    std::vector<double> pose;         // the f64 shape fields, 9 per object
    uint32_t scan_counts[3] = {0, 0, 0};   // spheres, single triangles, triangle pairs
    bool has_blob = false;            // n <= ptk::kSmallObjs
    bool spheres_only = false;        // runs is one run of at most ptk::kSpheresOnlyMax spheres at offset 0, first object 0
    bool lambert_surfaces = true;     // every material is Lambertian, or Emissive with a non-zero emission
    bool diffuse_only = true, no_mirror = true, no_oren_nayar = true;
    bool split_ok = false;            // a minority of the objects is Mirror
    bool auto_bvh = false;
};

void shape_records(const PtObject& o, float4 gather[3], float4 scan[3], int* n_scan);
// PT_OK, or PT_ERR_INVALID_ARG for an object with a bad tag: then *out is untouched
int build(const PtObject* objs, uint32_t n, Records* out);

}  // namespace ptscene
