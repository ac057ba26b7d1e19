// pt_kernels.h -- launch interface between the host driver (pt_api.cpp) and the
// HIP kernels (pt_kernels_*.hip).  Plain structs, no HIP types besides float4 and
// hipStream_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_probe_params.h"    // ptgrid::Grid, ptvis::Params, ptupd::Params
#include "pt_kernel_consts.h"   // kBlock, kSmallObjs, kRegenWaves*, kRegenSplitF4PerWave, kRegenCounters, kRegenCounterStride

namespace ptk {

// One contiguous run of same-shape objects of World.objects, in object order
// (the order decides closest-hit ties, src/world.rs:281-287).
// kRunTrianglePair: entries of two consecutive triangles that share v0 and the plane normal bit for bit (the halves of a
// parallelogram fanned from one corner): 5 float4 = the first triangle's record + (N1.xyz, N2.x), (N2.yz, -, -) of the
// second; objects first_obj + 2k and first_obj + 2k + 1.
enum { kRunSphere = 0, kRunTriangle = 1, kRunTrianglePair = 2 };
struct Run {
    uint32_t tag;        // kRunSphere / kRunTriangle (= the shape tags) / kRunTrianglePair
    uint32_t first_obj;  // object index of the run's first primitive
    uint32_t count;      // entries in the run (primitives; pairs)
    uint32_t off4;       // offset of the run in the scan array, in float4 units
};
constexpr uint32_t run_entry_f4(uint32_t tag) { return tag == kRunSphere ? 1u : tag == kRunTriangle ? 3u : 5u; }

// Optional BVH over the objects (pt_bvh.h); built on the host the first time a render asks for it.
struct BvhView {
    const uint4* nodes;      // 4 uint4 (64 bytes) per internal node: up to four child boxes on the 16-bit grid + their child codes (pt_bvh.h)
    float grid_min[3], grid_cell[3];   // box coordinate = grid_min + q * grid_cell
    const float4* rec;       // 3 float4 per leaf slot (scan record of the primitive); the traversal reads e1, e2 of triangles here
    const float4* lead;      // 1 float4 per leaf slot = rec[3 * slot]: sphere (c, r^2) / triangle v0 -- a leaf's <= 4 are one 64-byte line
    const uint32_t* ids;     // object index per leaf slot (bit 31: triangle); a leaf starts at a multiple of 4: one 16-byte load
    uint32_t root;           // child code of the root
    float scene_abs;         // scale of the padding the slab test applies (see bvh_scan)
};

struct SceneView {
    const float4* scan;      // scan records, run-packed: sphere = 1 float4 (c, r^2); triangle = 3 float4 (n, N1.x) (v0, N1.y) (N1.z, N2): pt_bvh.h triangle_scan_record
    const float4* shape;     // 3 float4 per object (gather form), see pt_device.h
    const float4* mat;       // 2 float4 per object
    const Run* runs;
    const uint32_t* lights;  // object indices of the emitters (world.rs:214-225)
    // scenes of <= kSmallObjs objects: the five arrays above packed back to back
    // [scan | shape | mat | runs | lights], copied whole into LDS by every workgroup
    const float4* blob;
    uint32_t blob_f4;        // float4 count of `blob` (0 for larger scenes)
    uint32_t scan_f4;        // float4 count of `scan`
    uint32_t n_runs, n_objs, n_lights;
    uint32_t spheres_only;   // the scan array is ONE run of n_objs <= kSpheresOnlyMax spheres at offset 0, first object 0 (decided at upload: ptscene::build)
    uint32_t lambert_surfaces;   // every material is Lambertian, or Emissive with a non-zero emission (a hit there ends the path): decided at upload too
    uint32_t diffuse_only;   // every material is Lambertian or emissive: kernels without the GGX / OrenNayar code
    uint32_t no_mirror;      // no Mirror surface (k_paths_regen without the GGX code also for scenes with OrenNayar surfaces)
    uint32_t no_oren_nayar;  // no OrenNayar surface (k_paths_regen_split: its plain iterations are then the diffuse-only code)
    BvhView bvh;             // valid only for launches with accel != 0
};

struct CameraF {             // Camera's cached fields in f32 (camera.rs:36-38)
    float origin[3], lower_left[3], horizontal[3], vertical[3];
    uint32_t width, height;
};

// Path-state queue: 4 float4 planes, index = queue slot (coalesced 16 B/lane).
//   ray part    q0 = (o.x, o.y, o.z, d.x)   q1 = (d.y, d.z, bits(tile_row<<16 | x), bits(s_local<<16 | depth))
//   carry part  q2 = (beta.x, beta.y, beta.z, pdf_prev)   q3 = (L.x, L.y, L.z, eta_in)
// so width, tile rows and samples per batch are each < 65536.  The kernels read the carry part of a path only after
// its vertex's scans (it is not needed before), which keeps eight registers free during them.
struct Queue {
    float4* q[4];
};

// Row-band tile (include/pathtrace_amd.h): tile row yl -> image row
//   y = (yl / band_rows) * band_stride + band_first + yl % band_rows
// with yl / band_rows = umulhi(yl, band_magic) (exact for yl, band_rows < 65536).
struct TileMap {
    uint32_t band_rows, band_magic, band_stride, band_first;
};

// Final radiance of one path (per-sample buffer `lsamp`): 12 bytes, so that the buffer and the resolve's reads are a
// quarter smaller than with a float4.
struct Rgb {
    float r, g, b;
};

struct BounceArgs {
    Queue q;                  // compacted in place, one private segment per wave
    // tail hand-off between launches (small scenes): a wave whose segment falls below export_below paths
    // appends them to ovf_out (slot = atomicAdd(ovf_out_count, n)) and retires; a continuation launch
    // (src_mode = 1) takes its n_first paths from ovf_in instead of generating camera rays
    Queue ovf_in, ovf_out;
    uint32_t* ovf_out_count;
    // non-null: level-0 launch in the regenerating form (k_paths_regen; scene in LDS, src_mode 0; a pixel list only for
    // pt_render_adaptive's passes): the waves take the batch's 64-path chunks from this counter (zeroed before the launch)
    // and export what is alive when it runs out
    uint32_t* chunk_counter;
    // non-null (with chunk_counter): the regenerating form that batches Mirror vertices (k_paths_regen_split); per wave of the
    // launch kXqF4PerWave float4 of exchange stacks + parking area
    float4* xchg;
    uint32_t regen_static;    // chunks dealt round-robin to the waves (a multiple of the launch's wave count); the rest by the counters
    // non-null (regenerating launches that overlap their neighbours: pt_api.cpp, lanes): the workgroups from core_blocks on are
    // SPARE -- each reads *posted (host memory: launches the host has enqueued so far) when it starts and ends at once if two
    // or more launches follow this one (seq = this launch's number); otherwise it works like any other
    const uint32_t* posted;
    uint32_t seq, core_blocks;
    uint32_t src_mode;        // 0: pass 0 generates camera rays, 1: pass 0 reads ovf_in
    uint32_t export_below;    // >= 1; 1 = never export (a wave runs until its segment is empty)
    uint32_t seg_cap;         // slots per segment (multiple of 64)
    // accel = 1 only (k_paths_bvh): per-slot scratch of the staged passes, same indexing as q
    float4* aux;              // (closest-hit id, t, occluded, -)
    float4* sray0;            // shadow ray (o, d.x)
    float4* sray1;            // (d.y, d.z, t_max, 1 = the slot has a shadow ray)
    Rgb* lsamp;               // per-path final radiance, index = s_local*np + tile_row*width + x
    unsigned long long* stats;  // [0] shadow rays  [1] path vertices  [2] deepest vertex (max)  [3] vertices of level-0 launches  [4] finished samples (lsamp writes)  [7] internal error flag (k_paths_regen_split: exchange stacks met)
    TileMap tile;
    SceneView sc;
    CameraF cam;
    uint32_t n_first;         // paths of the batch
    // continuation launches may take their path count from device memory instead (the counter the previous launch's
    // waves added their leftovers to): the host then never waits for it.  seg_cap is derived on the device in that case.
    const uint32_t* n_first_dev;
    // pixel-list renders (pt_render_pixels / pt_ray_color): film slot i = (tile_row << 16) | x of the path state,
    // RNG key and camera pixel = pixels[i] = (x, y) of the image.  film_w = row pitch of the film-slot arithmetic
    // (camera width, or 65536 for a list).  A list with chunk_counter set (pt_render_adaptive's passes) takes the
    // regenerating kernel's LIST instances (k_paths_regen<MIS, mats, true>).
    const uint2* pixels;
    uint32_t film_w;
    uint32_t film_w_magic;    // floor(2^32 / film_w), 0xFFFFFFFF for 1 (divmod_magic)
    uint32_t np;              // pixels of the tile
    uint32_t np_magic;        // floor(2^32 / np), 0xFFFFFFFF for 1
    uint32_t s_base;          // sample index of s_local = 0 (spp_offset + batch start)
    uint32_t min_depth, max_depth;
    float t_min;
    uint32_t integrator;
    uint32_t bvh_refill, bvh_leaf;   // traverse_segment thresholds (lanes)
    uint32_t accel;           // 0: linear scan (the reference's hit_scene), 1: BVH traversal, same answers
    uint32_t debug_tag;       // measurement builds (PT_DRAIN_TIMING): plane of ovf_out that receives the per-wave stamps
};

// How a linear-scan kernel finds the closest hit (pt_kernels_main.hip: scene_mode), and the material sets kernels are compiled for
// (pt_kernels_vertex.h: assume_mats).
constexpr int kModeLds = 0, kModeTiled = 1, kModeBvh = 2;
constexpr int kMatsAll = 0, kMatsDiffuse = 1, kMatsNoMirror = 2, kMatsMirror = 3;
// Launch log (pt_debug_launch_log): the path-kernel instance a launch takes, one word recorded by the host as it enqueues the
// launch.  bits 0-1 family, bit 2 MODE of k_paths (kModeLds / kModeTiled), bit 3 MIS, bit 4 OVF, bits 5-6 the material set
// (k_paths, k_paths_bvh: DIFFUSE; k_paths_regen: MATS; k_paths_regen_split: PLAIN), bit 7 LIST, bit 8 exact arithmetic.
// Template arguments the family does not have are 0.  pt_debug_path_instances lists every word the dispatch can record.
enum { kInstPaths = 0, kInstBvh = 1, kInstRegen = 2, kInstRegenSplit = 3 };
constexpr uint32_t instance_code(uint32_t family, int mode, bool mis, bool ovf, int mats, bool list, bool exact) {
    return family | (uint32_t)mode << 2 | (uint32_t)mis << 3 | (uint32_t)ovf << 4 | (uint32_t)mats << 5 | (uint32_t)list << 7 |
           (uint32_t)exact << 8;
}
constexpr uint32_t kTileF4 = 1920;         // 30 KiB LDS tile (divisible by 3: whole triangles); 5 workgroups per CU (measured: 2550 / 4 -> 1214 ms, 1920 / 5 -> 1106 ms on C4)
constexpr uint32_t kRefillBelow = 44;      // BVH traversal: hand out new rays when fewer lanes than this are tracing
constexpr uint32_t kLeafBatch = 20;        // BVH traversal: test leaf primitives when at least this many lanes wait at a leaf
constexpr uint32_t kBvhMaxLeaf = 4;        // primitives per BVH leaf the traversal unrolls for (= ptbvh::kMaxLeaf)
#ifndef PT_BVH_STACK
#define PT_BVH_STACK 24
#endif
constexpr uint32_t kBvhStack = PT_BVH_STACK;         // traversal stack entries per lane, in LDS (= ptbvh::kStackDepth): 24 KiB per workgroup, 5 workgroups per CU

// One launch traces every path of a batch to its end.  grid = number of 256-thread workgroups
// (4 queue segments each).  _exact / _fast: the two arithmetic modes of pt_device.h
// (PtRenderParams.exact_math).
// pt_scene_upload: per-object constants written into the shape / material records (k_scene_setup), one call per arithmetic
// mode on that mode's copy of the records
void launch_scene_setup_exact(float4* shape, float4* mat, uint32_t n_objs, hipStream_t st);
void launch_scene_setup_fast(float4* shape, float4* mat, uint32_t n_objs, hipStream_t st);
// workgroups per CU of the regenerating level-0 kernel `a` selects (sc, integrator, xchg), with the scene's LDS blob; 0 = unknown
uint32_t regen_blocks_per_cu_exact(const BounceArgs& a);
uint32_t regen_blocks_per_cu_fast(const BounceArgs& a);
// One path-kernel launch; returns the instance code (instance_code) of the kernel it enqueued, for the launch log.
uint32_t launch_path_kernel_exact(const BounceArgs& a, uint32_t grid, hipStream_t st);
uint32_t launch_path_kernel_fast(const BounceArgs& a, uint32_t grid, hipStream_t st);
// between the kernel translation units (pt_kernels_unit.h; not called by the host code): k_paths_regen_split's and the BVH form's
// launchers live with their kernels, in pt_kernels_split.hip and pt_kernels_bvh.hip
int regen_split_blocks_per_cu_exact(const BounceArgs& a, size_t lds);
int regen_split_blocks_per_cu_fast(const BounceArgs& a, size_t lds);
uint32_t launch_regen_split_exact(const BounceArgs& b, uint32_t blocks, size_t lds, hipStream_t st);
uint32_t launch_regen_split_fast(const BounceArgs& b, uint32_t blocks, size_t lds, hipStream_t st);
uint32_t launch_paths_bvh_exact(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st, bool diffuse, bool list);
uint32_t launch_paths_bvh_fast(const BounceArgs& a, uint32_t grid, size_t lds, hipStream_t st, bool diffuse, bool list);
void launch_debug_hit_bvh_exact(const SceneView& sc, uint32_t grid, size_t lds, const float* rays6, uint32_t n, float t_min, float t_max,
                                float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st);
void launch_debug_hit_bvh_fast(const SceneView& sc, uint32_t grid, size_t lds, const float* rays6, uint32_t n, float t_min, float t_max,
                               float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st);

// Film: sum the nb samples of every tile pixel in sample order into the f64
// accumulator (world.rs:311), and when finalising write mean, sqrt-gamma and
// truncated RGBA8 (world.rs:315-332).
struct ResolveArgs {
    const Rgb* lsamp;
    double* film;             // np*3 doubles (may be null when the render is a single batch)
    float* out_linear;        // np*3
    uint8_t* out_rgba;        // np*4 or null
    uint32_t np, nb;
    uint32_t load_film;       // start from the f64 sums in `film` (not the first samples of the pixel)
    uint32_t store_film;      // keep the sums in `film` (more samples follow)
    uint32_t finalize;        // write the outputs: mean over spp_div samples, gamma, quantisation
    uint32_t spp_div;
    // non-null: the finalising pass writes ONE 16-byte record per pixel here (12 B linear RGB + 4 B RGBA8: the send
    // buffer of the multi-GPU film gather) INSTEAD of the two planes -- what k_film_pack made of them in a second launch
    void* out_packed;
    // non-null: workgroup 0 clears these words (the chunk / hand-over counters of the batch just resolved, so that the
    // next launch that uses them finds them zero without a memset of its own in the stream)
    uint32_t* zero_words;
    uint32_t n_zero;
};
void launch_resolve(const ResolveArgs& a, hipStream_t st);

// Adaptive sampling (pt_render_adaptive, the rule in pt_adaptive.h).  Image-indexed state: f64 sums per pixel (R, G, B, S1 =
// sum of luminance, S2 = sum of its square) in sample order, sample count, relative error, converged flag.
struct AdaptiveFilm {
    double* sums;             // 5 doubles per image pixel
    uint32_t* count;          // samples per image pixel
    float* rel_err;           // se / max(mean, abs_floor) at count
    uint32_t* conv;           // 1: the last check passed
    float* out_linear;        // image-indexed film (mean), 3 floats per pixel
    uint8_t* out_rgba;        // 4 bytes per pixel
    double rel_tol, abs_floor;
};
// One sample batch of a pass: list slot i (pixel pixels[i], or image pixel i when pixels is null) adds the nb samples
// lsamp[s * n + i] to its sums; on the pass's last batch (finalize) the pixel's film, count (= n_total), rel_err and flag.
struct AdaptiveResolveArgs {
    AdaptiveFilm f;
    const Rgb* lsamp;
    const uint2* pixels;
    uint32_t width, n, nb, n_total;
    uint32_t load;            // start from the stored sums (else from zero: the pixel's first samples)
    uint32_t finalize;
    uint32_t* zero_words;     // as ResolveArgs
    uint32_t n_zero;
};
void launch_resolve_adaptive(const AdaptiveResolveArgs& a, hipStream_t st);
// The pixels of a list (null: every image pixel in order, n = width * height) whose last check failed, compacted into
// out in the list's order.  block_counts: ceil(n / kSelectTile) words of scratch; *out_n = survivors.
constexpr uint32_t kSelectTile = 1024;
void launch_adaptive_select(const uint2* pixels, uint32_t n, uint32_t width, const uint32_t* conv, uint32_t* block_counts,
                            uint2* out, uint32_t* out_n, hipStream_t st);
// The variance plane of pt_denoise_var_device from that state (pt_adaptive_variance_device; the rule in pt_denoise_var.h):
// sums 5 doubles and count one word per image pixel, feat the 2 float4 feature records; var one float per pixel.
void launch_adaptive_variance(const double* sums, const uint32_t* count, const float4* feat, uint32_t np, float* var, hipStream_t st);

// Brightness cascade (pt_render_cascade_device, the rule in pt_cascade.h).  The levels as the host formed them (ptcas::levels), K
// layers.  State of an image of np pixels: (3 K + 3) planes of np doubles -- plane 3 k + c = S_k.c, planes 3 K + c the plain sums
// P.c -- and K planes of np doubles for the counts cnt_k.
struct CascadeResolveArgs {
    double B[8];
    double kappa;
    uint32_t K;
    const Rgb* lsamp;         // nb * np samples, [s * np + p]
    double* state;
    double* cnt;              // written by the finalising launch
    uint32_t np, nb;
    uint32_t load;            // start from the stored sums (else from zero: the pixels' first samples)
    uint32_t finalize;        // the last samples of the pixels: leave the counts for k_cascade_reweight
    uint32_t* zero_words;     // as ResolveArgs
    uint32_t n_zero;
};
void launch_resolve_cascade(const CascadeResolveArgs& a, hipStream_t st);
// The film of a finalised state: out_linear np * 3 floats, out_rgba np * 4 bytes or null, out_plain (P / n_total) np * 3 floats or
// null, out_weights K planes of np floats or null.
struct CascadeReweightArgs {
    double B[8];
    double kappa;
    uint32_t K;
    const double* state;
    const double* cnt;
    uint32_t width, height, n_total;
    float* out_linear;
    uint8_t* out_rgba;
    float* out_plain;
    float* out_weights;
};
void launch_cascade_reweight(const CascadeReweightArgs& a, hipStream_t st);

// Reconstruction filter (pt_render_filtered_device, the rule in pt_filter.h).  State of an image of np pixels: 7 planes of np
// doubles -- planes 0..2 the weighted sums A.c, plane 3 the weight sum Wt, planes 4..6 the plain sums P.c.
struct FilterResolveArgs {
    uint32_t kind, m;         // ptflt::Rule, as the host formed it (ptflt::rule)
    double R, alpha, gR;
    double a3, a2, a0, b3, b2, b1, b0;
    const Rgb* lsamp;         // nb * np samples, [s * np + y * width + x]
    double* state;
    uint32_t width, height, nb;
    uint32_t first_sample;    // the sample index of the batch's first sample (spp_offset + the samples of the batches before it)
    uint32_t n_total;         // samples per pixel once the last batch is in
    uint32_t load;            // start from the stored sums (else from zero: the pixels' first samples)
    uint32_t finalize;        // the last samples of the pixels: write the planes
    float* out_linear;        // np * 3
    uint8_t* out_rgba;        // np * 4 or null
    float* out_plain;         // np * 3 or null
    double* out_wsum;         // np or null
    uint32_t* zero_words;     // as ResolveArgs
    uint32_t n_zero;
};
void launch_resolve_filter(const FilterResolveArgs& a, hipStream_t st);

// Multi-GPU film exchange (pt_multi.cpp): tile -> 16 B per pixel (linear RGB + RGBA8) before the gather, gathered
// padded tiles -> frame in image order after it.
void launch_film_pack(const float* lin, const uint8_t* rgba, uint32_t np, void* packed, hipStream_t st);
void launch_film_unpack(const void* recv, uint32_t W, uint32_t H, uint32_t band_rows, uint32_t n_dev, uint32_t max_rows, float* lin,
                        uint8_t* rgba, hipStream_t st);

// World::hit_scene on arbitrary rays (debug/parity entry).
// scratch: accel = 1 only, 3*n float4 of device memory.  out_rec: optional, 8 floats per ray (t, point3, normal3, front_face).
void launch_debug_hit_exact(const SceneView& sc, uint32_t accel, const float* rays6, uint32_t n, float t_min, float t_max,
                            float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st);
void launch_debug_hit_fast(const SceneView& sc, uint32_t accel, const float* rays6, uint32_t n, float t_min, float t_max,
                           float4* scratch, int32_t* out_id, float* out_t, float* out_rec, hipStream_t st);

// The per-vertex functions on arbitrary inputs (debug/parity entries; layouts at k_debug_fn in pt_kernels_main.hip).
enum { kFnBsdfEval = 0, kFnBsdfSample = 1, kFnShapeSample = 2, kFnLightPoint = 3, kFnCameraRay = 4,
       kFnJointScan = 5 };     // (a kernel of its own: the scene staged in LDS; scenes of <= kSmallObjs objects)
struct DebugFnArgs {
    SceneView sc;
    CameraF cam;              // kFnCameraRay only
    uint32_t op, obj, n;
    uint32_t in_stride, out_stride;   // floats per item
    const float* in;
    const uint32_t* words;    // 4 raw words per item, or null
    float* out;
};
void launch_debug_fn_exact(const DebugFnArgs& a, hipStream_t st);
void launch_debug_fn_fast(const DebugFnArgs& a, hipStream_t st);


// First-hit feature buffers (pt_render_features_device).  launch_feature_resolve: the hits of one batch of feature rays
// (launch_source_feature_rays below; launch_debug_hit's ids and records) -> 32-byte records (albedo rgb, emitter | normal xyz, depth),
// summed per pixel in sample order into out (2 float4 per pixel; load: add to the sums there); finalize divides by n_samples.
struct FeatureResolveArgs {
    const float4* mat;        // material records of the arithmetic mode's scene view
    const int32_t* ids;       // nb * np
    const float* rec;         // nb * np * 8 (t, point3, normal3, front_face)
    float4* out;
    uint32_t np, nb, n_samples, load, finalize;
};
void launch_feature_resolve_exact(const FeatureResolveArgs& a, hipStream_t st);
void launch_feature_resolve_fast(const FeatureResolveArgs& a, hipStream_t st);
inline void launch_feature_resolve(bool exact, const FeatureResolveArgs& a, hipStream_t st) {
    exact ? launch_feature_resolve_exact(a, st) : launch_feature_resolve_fast(a, st);
}

// Edge-avoiding a-trous denoiser (pt_denoise_device; rule: include/pathtrace_amd.h PtDenoise).  init: the film -> the state
// plane dst (u.rgb, var); a step (init = false): src -> dst with the taps at distance `step`.  finalize: the launch writes
// c' = u * a to out_linear and its RGBA8 word to out_rgba (may be null) instead of dst.
struct DenoiseArgs {
    const float* linear;      // width * height * 3, the noisy film
    const float4* feat;       // width * height * 2, the feature records
    const float4* src;
    float4* dst;
    float* out_linear;
    uint8_t* out_rgba;
    uint32_t width, height, step, finalize;
    float sigma_l, sigma_n, sigma_d;
};
void launch_denoise(const DenoiseArgs& a, bool init, hipStream_t st);
// init with a variance plane of the caller's (pt_denoise_var_device): var[p] where it is finite and >= 0, else the 3 x 3 variance
void launch_denoise_init_var(const DenoiseArgs& a, const float* var, hipStream_t st);

// Temporal accumulation in front of the a-trous steps (pt_denoise_temporal_device; rule: include/pathtrace_amd.h PtTemporal).
// One launch per frame in place of k_denoise_init: reads the film, the features and the history hist_src (null: none), writes
// (u.rgb, var) to dn.dst (or, dn.finalize, the film planes) and the frame's history to hist_dst.  History record, 3 float4 per
// pixel: (u.rgb, m1), (m2, n, emitter, 0), (normal xyz, depth).  Cameras in f64: the reprojection is computed in f64.
struct TemporalArgs {
    DenoiseArgs dn;
    const float4* hist_src;
    float4* hist_dst;
    double cur[12], prev[12];  // origin, lower_left, horizontal, vertical of the frame's and of the history's camera
    uint32_t same_camera;      // the two cameras are equal field by field: x' = x, y' = y, d_exp = d_p exactly
    float alpha, depth_tol, normal_tol;
};
void launch_denoise_temporal(const TemporalArgs& a, hipStream_t st);

// Temporal accumulation that follows moving objects (pt_denoise_temporal_motion_device; rule: include/pathtrace_amd.h, rules
// 1', 2', 3', 7').  k_denoise_temporal_motion in place of k_denoise_temporal: additionally reads the pixel's object id and that
// object's motion map (current pose -> history pose, pt_motion.h), and keeps id + 1 in the history's free lane:
// (m2, n, emitter, id + 1 as float; 0 = unknown, which is what k_denoise_temporal stores).
struct MotionMap {             // 104 bytes
    double a[9], b[3];         // x -> a x + b, a row-major
    uint32_t flags, pad;       // bit 0 identity, bit 1 invalid (ptmo::kIdentity, kInvalid)
};
struct TemporalMotionArgs {
    TemporalArgs t;
    const int32_t* ids;        // width * height, the caller's: bounds-checked against n_objs before a map is read
    const MotionMap* maps;     // n_objs
    uint32_t n_objs;
};
void launch_denoise_temporal_motion(const TemporalMotionArgs& a, hipStream_t st);

// The motion form with a per-pixel blend weight (pt_denoise_temporal_alpha_device; rule 4 of include/pathtrace_amd.h with
// alpha[p] in place of t.alpha where that entry is finite and in [0, 1]).  k_denoise_temporal_alpha.
struct TemporalAlphaArgs {
    TemporalMotionArgs m;
    const float* alpha;        // width * height
};
void launch_denoise_temporal_alpha(const TemporalAlphaArgs& a, hipStream_t st);

// Temporal gradients (pt_temporal_gradient_device; rule: pt_gradient.h).  One gradient pixel per 3 x 3 stratum of the image:
// launch_gradient_list writes the strata's pixels (the list the re-trace renders), launch_gradient_strata turns the re-traced
// film (one RGB per stratum, list order) and the previous frame's film into the records (delta, N), launch_gradient_alpha
// sums every pixel's window of records into its blend weight.
struct GradientArgs {
    const float* retraced;     // strata * 3
    const float* prev;         // width * height * 3
    uint2* list;               // strata
    double* rec;               // strata * 2
    float* alpha;              // width * height
    uint32_t width, height, seed, radius;
    float scale, alpha_min;
};
void launch_gradient_list(const GradientArgs& a, hipStream_t st);
void launch_gradient_strata(const GradientArgs& a, hipStream_t st);
void launch_gradient_alpha(const GradientArgs& a, hipStream_t st);
// ... under a moving camera (pt_temporal_gradient_camera_device): the strata lie in the previous frame's image,
// and k_gradient_alpha_camera in place of k_gradient_alpha looks every current pixel's stratum up through the temporal
// reprojection.  Of t it reads dn.feat, dn.width, dn.height, cur (the frame's camera), prev (the previous frame's) and same_camera.
void launch_gradient_alpha_camera(const GradientArgs& a, const TemporalArgs& t, hipStream_t st);

// Device-side BVH refit (pt_scene_refit; rule: ptbvh::refit in pt_bvh.h, whose arrays these launches reproduce bit for bit).
// The topology -- ids, child codes, the order of the nodes by height -- stays; leaf records, child boxes and their quantisation
// are recomputed from the scene's gather records.  The grid is the host's (one O(n) pass over its copy of the records) and
// travels by value.  launch_bvh_refit_leaves first, then launch_bvh_refit_level once per height from 0 upward, all on one
// stream: a node reads what the launches before it wrote, so nothing waits inside a kernel.
struct BvhRefitArgs {
    const float4* shape;      // gather records, 3 float4 per object (the .w lanes of a triangle's records are not read)
    const uint32_t* ids;      // object index per leaf slot (bit 31: triangle; 0xFFFFFFFF: padding slot)
    float4* rec;              // 3 float4 per leaf slot, written
    float4* lead;             // 1 float4 per leaf slot, written
    float4* slot_box;         // scratch, 2 float4 per leaf slot: the primitive's f32 box (lo, -) (hi, -)
    uint4* nodes;             // 4 uint4 per node: the three box words rewritten, the code word kept
    float4* node_box;         // scratch, 2 float4 per node: the union of the node's child boxes, for its parent
    const uint32_t* order;    // node indices by height (0 = all children are leaves), ties by index
    unsigned long long* cost; // 3 words: sums over the used child slots of dx dy, dy dz, dz dx in grid units (d = q_hi - q_lo)
    float grid_min[3], grid_cell[3];
    uint32_t n_slots;
};
void launch_bvh_refit_leaves(const BvhRefitArgs& a, hipStream_t st);   // also zeroes the three cost words
void launch_bvh_refit_level(const BvhRefitArgs& a, uint32_t first, uint32_t count, hipStream_t st);   // nodes order[first, first + count)

// Device-side BVH build (pt_scene_rebuild; rule: ptbvh::build_morton in pt_bvh.h).  What is new beside the refit
// is which object sits in which leaf slot: the objects ordered by (Morton key, index).  All launches on one stream, in this order:
//   launch_bvh_morton      pairs[0][i] = (key of object i, i)
//   launch_bvh_sort        least-significant-digit radix sort of the pairs by key, 8-bit digits, four passes; every pass is
//                          stable, so equal keys stay in index order.  The result is in pairs[0] again.
//   launch_bvh_write_ids   leaf_ids from the order (pairs = nullptr: the index order), padding slots kDone with zero records
//   launch_bvh_codes       (only when the tree arrays hold another topology) the child codes into qnodes[4k + 3]
// and then the refit launches.  No kernel waits for another; the stream orders them.
constexpr uint32_t kSortTile = 2048;       // pairs per workgroup and pass
constexpr uint32_t kSortDigits = 256;
struct BvhBuildArgs {
    const float4* shape;      // gather records, 3 float4 per object
    const uint32_t* tags;     // shape tag per object (0 sphere)
    uint2* pairs[2];          // (key, object index), ping-pong, n each
    uint32_t* hist;           // kSortDigits * tiles words: hist[digit * tiles + tile]
    uint32_t* ids;            // leaf_ids, n_slots
    float4* rec;              // 3 float4 per leaf slot (zeroed for padding slots)
    float4* lead;             // 1 float4 per leaf slot (likewise)
    float grid_min[3], grid_cell[3];
    uint32_t n, n_slots;
};
inline uint32_t bvh_sort_tiles(uint32_t n) { return (n + kSortTile - 1) / kSortTile; }
void launch_bvh_morton(const BvhBuildArgs& a, hipStream_t st);
void launch_bvh_sort(const BvhBuildArgs& a, hipStream_t st);
void launch_bvh_write_ids(const BvhBuildArgs& a, bool sorted, hipStream_t st);
void launch_bvh_codes(uint4* nodes, const uint4* codes, uint32_t n_nodes, hipStream_t st);

// The median order (pt_scene_rebuild_ordered; rule: ptbvh::build_median in pt_bvh.h) in place of launch_bvh_morton
// and launch_bvh_sort.  The plan (ptbvh::MedianPlan) is on the device; all launches on one stream:
//   k_bvh_cells            cells[i] = the three grid cells of object i, pairs[0][p] = p (the index order)
//   per level of steps above T positions (BvhMedianLevel):
//     k_bvh_median_bounds  per step of the level the minimum and maximum cell per axis over its positions (bounds, zeroed before)
//     k_bvh_median_keys    the 64-bit key of every position, (group << (16 + index_bits)) | (v << index_bits) | object, v = the
//                          object's cell on the step's axis, or in a group no step covers the offset inside it: those stay
//     the radix sort over as many 8-bit digits as the key has.  The object index is the lowest part of the key, so the order
//     is (group, cell, index) however the objects stood before.
//   k_bvh_median_unpack    the other pair buffer = (0, object) per position
//   k_bvh_median_tile      one workgroup per tile: its step and every step beneath it in LDS, the result into that buffer
// Returns which pair buffer launch_bvh_write_ids has to read.
struct BvhMedianLevel { uint32_t first, groups, bits; };       // group_start[first, first + groups]; bits to number the groups
struct BvhMedianArgs {
    BvhBuildArgs b;                  // shape, tags, pairs, hist, the grid, n
    uint2* cells;                    // n: (g0 | g1 << 16, g2)
    uint32_t* bounds;                // 6 words per group of the widest level: 65535 - min per axis, max per axis
    const uint32_t* group_start;     // ptbvh::MedianPlan::group_start
    const uint4* tiles;              // ... ::tiles
    const uint2* tile_steps;         // ... ::tile_steps
    uint32_t n_tiles, index_bits;
};
uint32_t launch_bvh_median(const BvhMedianArgs& a, const BvhMedianLevel* levels, uint32_t n_levels, hipStream_t st);

// Auto-exposure and tone mapping (pt_tonemap_device; rule: pt_tonemap.h).  All launches on one stream:
//   launch_film_histogram   the 258 words of the film's luminance histogram, added to hist: the caller zeroes it in front
//   launch_exposure_meter   one wave: hist and the parameters -> the context's exposure state
//   launch_tonemap          per pixel the curve and the transfer under the exposure *e_dev (null: e_manual)
struct ExposureState {         // device words the context owns; all zero = no exposure yet
    double log2E;
    float E;
    uint32_t valid, width, height, pad[2];
};
struct ExposureArgs {
    const uint32_t* hist;
    ExposureState* state;
    uint32_t width, height;
    float pct_lo, pct_hi, key, log2_min, log2_max, adapt;
};
struct TonemapArgs {
    const float* linear;       // width * height * 3; may be out_linear
    float* out_linear;         // may be null
    uint8_t* out_rgba;
    const float* e_dev;
    float e_manual, white;
    uint32_t np, curve, transfer;
};
void launch_film_histogram(const float* linear, uint32_t np, uint32_t* hist, uint32_t n_cus, hipStream_t st);
void launch_exposure_meter(const ExposureArgs& a, hipStream_t st);
void launch_tonemap(const TonemapArgs& a, hipStream_t st);

// Bloom (pt_bloom_device; rule: pt_bloom.h).  A pyramid level is three planes (R, G, B) of `stride` floats.
//   launch_bloom_reduce   one workgroup per 16 x 16 destination tile; first: the source is the film (interleaved RGB) under the bright pass
//   launch_bloom_expand   one workgroup per 32 x 8 destination tile; last = 0: fine holds D_i and receives U_i = (1 - s) D_i + s up(coarse);
//                         last = 1: out = film + intensity up(coarse), the combine (out may be film)
//   launch_bloom_tail     one workgroup: the levels w[0 .. n) x h[0 .. n) in LDS, down and up again; dst receives U of the first of them.
//                         src: the level above it, which the first is reduced from; null: dst already holds D of the first
struct BloomRule {             // pbloom::Rule
    float T, k, clamp, s, oms, intensity;
};
struct BloomReduceArgs {
    const float* src;
    float* dst;
    size_t src_stride, dst_stride;
    uint32_t sw, sh, dw, dh, tiles_x, first;
    BloomRule r;
};
struct BloomExpandArgs {
    const float* coarse;
    size_t coarse_stride;
    uint32_t cw, ch;
    float* fine;               // last = 0
    size_t fine_stride;
    const float* film;         // last = 1
    float* out;
    uint32_t w, h, tiles_x, last;
    BloomRule r;
};
struct BloomTailArgs {
    const float* src;
    size_t src_stride;
    uint32_t sw, sh;
    float* dst;
    size_t dst_stride;
    uint32_t n, w[8], h[8];
    BloomRule r;
};
void launch_bloom_reduce(const BloomReduceArgs& a, uint32_t tiles, hipStream_t st);
void launch_bloom_expand(const BloomExpandArgs& a, uint32_t tiles, hipStream_t st);
void launch_bloom_tail(const BloomTailArgs& a, hipStream_t st);

// Feature-guided upsampling (pt_upsample_device; rule: pt_upsample.h).  One launch: the low film and its feature
// records, the full-size records -> the full-size film planes (out_rgba may be null).
struct UpsampleArgs {
    const float* lo_linear;    // lo_width * lo_height * 3
    const float4* lo_feat;     // lo_width * lo_height * 2
    const float4* feat;        // width * height * 2
    float* out_linear;         // width * height * 3
    uint8_t* out_rgba;
    uint32_t width, height, lo_width, lo_height;
    float sigma_n, sigma_d;
};
void launch_upsample(const UpsampleArgs& a, hipStream_t st);

// Sources of first rays (pt_kernels_rays.hip): the pinhole camera (feature rays only), the thin lens (pt_render_lens_device; rule:
// pt_lens.h), the projections and the caller's rays (pt_render_projection_device, pt_render_rays_device; rule:
// pt_projection.h) and the bakes (pt_bake_lightmap_device, pt_bake_probes_device; rule: pt_bake.h).
// LensF, ProjF: ptlens::Setup and ptproj::Setup as the kernels take them; ProjF::kind: PT_PROJ_*.
struct LensF {
    float lu[3], lv[3], inv_phi;
};
struct ProjF {
    float u[3], v[3], w[3], c[3], aspect, fov720;
    uint32_t kind;
};
enum { kSrcCamera = 0, kSrcLens = 1, kSrcProjection = 2, kSrcBake = 3, kSrcRays = 4, kSrcProbeUpdate = 5 };
struct RaySourceF {
    uint32_t tag;             // kSrc*: which of the words below are read
    CameraF cam;              // every source: the film's width and height; camera, lens, projection: the frame
    LensF lens;
    ProjF proj;
    struct {                  // the film is width x rows = texels (kind 0, data: float[H][W][6], 8-byte aligned) or directions x
        const float* data;    // probes (kind 1, data: float[P][3])
        uint32_t kind, width;
    } bake;
    struct {                  // the render's rays in state order, float[n][6], 8-byte aligned, directions as given; weights3:
        const float* rays6;   // float[n][3], or null = 1
        const float* weights3;
    } rays;
    struct {                  // an update of a probe grid: the film is directions x slots, slot y = probe
        ptgrid::Grid grid;    // first + y stride of the grid; rule.rays_per_probe = the film's width
        ptupd::Params rule;
    } upd;
};
// launch_source_paths: the source's rays of samples s_base .. s_base + nb - 1 of every tile pixel as n = nb * np path states in the
// queue form (state s_local * np + tile pixel), for a path-kernel launch with src_mode = 1 to take up from ovf_in.
struct SourcePathsArgs {
    RaySourceF src;
    TileMap tile;
    float4* q[4];
    uint32_t np, np_magic, w_magic;   // tile pixels; floor(2^32 / np) and floor(2^32 / cam.width), 0xFFFFFFFF for 1
    uint32_t s_base, done, n;         // done: samples of the render before this batch (the caller's rays start at state done * np)
};
// launch_source_feature_rays: the source's rays of samples s_base .. s_base + nb - 1 of every image pixel, ray s_local * np + p, as
// the rays6 launch_debug_hit reads.  launch_debug_source_rays: words = n * (x, y, sample, -) -> out = n * (o3, d3, dx, dy) for the
// lens, n * (o3, d3, a, b) for a projection, n * (o3, d3) for a bake (x < width and y < the rows: the caller has checked).
// false: the source has no kernel of that form (paths: all but the camera; feature rays: camera, lens, projection, bake, probe
// update -- there the "image" is directions x probes --; debug rays: lens, projection, bake, probe update), nothing was launched.
bool launch_source_paths_exact(const SourcePathsArgs& a, hipStream_t st);
bool launch_source_paths_fast(const SourcePathsArgs& a, hipStream_t st);
bool launch_source_feature_rays_exact(const RaySourceF& src, uint32_t s_base, uint32_t nb, float* rays6, hipStream_t st);
bool launch_source_feature_rays_fast(const RaySourceF& src, uint32_t s_base, uint32_t nb, float* rays6, hipStream_t st);
bool launch_debug_source_rays_exact(const RaySourceF& src, const uint32_t* words, uint32_t n, float* out, hipStream_t st);
bool launch_debug_source_rays_fast(const RaySourceF& src, const uint32_t* words, uint32_t n, float* out, hipStream_t st);
inline bool launch_source_paths(bool exact, const SourcePathsArgs& a, hipStream_t st) {
    return exact ? launch_source_paths_exact(a, st) : launch_source_paths_fast(a, st);
}
inline bool launch_source_feature_rays(bool exact, const RaySourceF& src, uint32_t s_base, uint32_t nb, float* rays6, hipStream_t st) {
    return exact ? launch_source_feature_rays_exact(src, s_base, nb, rays6, st) : launch_source_feature_rays_fast(src, s_base, nb, rays6, st);
}
inline bool launch_debug_source_rays(bool exact, const RaySourceF& src, const uint32_t* words, uint32_t n, float* out, hipStream_t st) {
    return exact ? launch_debug_source_rays_exact(src, words, n, out, st) : launch_debug_source_rays_fast(src, words, n, out, st);
}

// What follows a bake's render (pt_sh_project_device too; film unit, one form for both modes).
void launch_bake_mask(const float* texels6, uint32_t n, float* out_linear, uint8_t* out_rgba, hipStream_t st);
void launch_probe_sh(uint32_t n_probes, uint32_t rays_per_probe, const float* radiance, float* sh27, hipStream_t st);

// Irradiance volume (pt_probe_grid_bake_device, pt_probe_shade_device; rule: pt_probe_grid.h; film unit, one form
// for both modes).  launch_probe_positions: the n = nx ny nz positions of a valid grid, 3 floats each.  launch_probe_shade: one
// thread per pixel of the width x height image; fallback may be null, or out_linear itself; out_rgba may be null.
struct ProbeShadeArgs {
    const float4* feat;
    const float* sh27;
    const float* fallback;
    float* out_linear;
    uint8_t* out_rgba;
    double cam[12];               // origin, lower_left, horizontal, vertical
    ptgrid::Grid grid;
    uint32_t width, height, weight;
    float normal_bias;
};
void launch_probe_positions(const ptgrid::Grid& g, uint32_t n, float* out, hipStream_t st);
void launch_probe_shade(const ProbeShadeArgs& a, hipStream_t st);

// Probe visibility (pt_probe_distances_device, pt_probe_moments_device, pt_probe_shade_visibility_device; rule: pt_probe_vis.h,
// DESIGN.md 5t; film unit).  launch_probe_distances: the ids and t of launch_debug_hit for n rays -> out[n], t or +inf.
// launch_probe_moments: distances float[n_probes][rays_per_probe] -> moments float[n_probes][T][T][2], checked parameters.
// launch_probe_shade_vis: launch_probe_shade with the maps (a.weight is not read).
struct ProbeMomentsArgs {
    const float* distances;
    float* moments;
    uint32_t n_probes, rays_per_probe;
    ptvis::Params vis;
};
void launch_probe_distances(const int32_t* ids, const float* t, uint32_t n, float* out, hipStream_t st);
void launch_probe_moments(const ProbeMomentsArgs& a, hipStream_t st);
void launch_probe_shade_vis(const ProbeShadeArgs& a, const float* moments, uint32_t resolution, hipStream_t st);

// Updates of the irradiance volume over frames (pt_probe_blend_device, pt_probe_grid_update_device; rule: pt_probe_update.h, DESIGN.md
// 5u; film unit).  launch_probe_update: one workgroup per slot; radiance float[n_upd][R][3] and distances float[n_upd][R] (null: no
// moments; then moments is not read) of the slots -> the slots' probes of sh27, moments and age, in place.  Checked parameters.
struct ProbeUpdateArgs {
    const float* radiance;
    const float* distances;
    float* sh27;
    float* moments;
    uint32_t* age;
    uint32_t n_probes;
    ptvis::Params vis;            // all zero without maps
    ptupd::Params u;
};
void launch_probe_update(const ProbeUpdateArgs& a, uint32_t n_upd, hipStream_t st);

}  // namespace ptk
