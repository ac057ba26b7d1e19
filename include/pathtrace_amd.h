/*
 * pathtrace_amd.h -- C ABI of the MI355X-native wavefront path tracer.
 *
 * Drop-in boundary for the per-pixel rendering hot path of roxas1533/pathtrace.
 * The reference has no FFI; the seam it offers is the Rust-internal call
 *     world_clone.render_pixel(x, y, &mut rng) -> Color        (src/main.rs:55,
 *                                                                src/world.rs:293)
 * inside the rayon loop at src/main.rs:43-60, plus the two film buffers
 * World.data (RGBA8, src/world.rs:55) and World.luminance_data (linear RGB,
 * src/world.rs:57).  pt_render() replaces that whole loop: one blocking call,
 * internally asynchronous on HIP streams.
 *
 * Only plain pointers, sizes and POD cross this boundary (no trait objects, no
 * torch types).  Reals are f64 on the boundary because the reference's
 * Vector3 is f64 (src/math.rs:4-8); the device computes in f32.
 *
 * Every function returns 0 on success and a non-zero PtStatus on failure;
 * pt_last_error() returns a thread-local message.  Nothing throws or aborts
 * across the boundary (the reference panics instead: src/main.rs:59,66).
 */
#ifndef PATHTRACE_AMD_H
#define PATHTRACE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 6

typedef enum {
    PT_OK = 0,
    PT_ERR_INVALID_ARG = 1,
    PT_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime failure at init   */
    PT_ERR_HIP = 3,         /* a HIP call failed; see pt_last_error()         */
    PT_ERR_OOM = 4,
    PT_ERR_UNSUPPORTED = 5
} PtStatus;

/* ---- scene description -------------------------------------------------- */

/* = the cached fields of Camera (src/camera.rs:27-39).  Fill with
 * pt_camera_new / pt_camera_look_at, or by hand.                            */
typedef struct {
    double origin[3];
    double lower_left[3];
    double horizontal[3];
    double vertical[3];
    uint32_t width, height;
} PtCamera;

/* Shape tags: which `impl Shape` (src/objects/shape.rs:52,160). */
enum { PT_SHAPE_SPHERE = 0, PT_SHAPE_TRIANGLE = 1 };
/* Material tags: which `impl Material` (src/objects/material.rs:85,138,220;
 * src/objects/mirror.rs:178). */
enum { PT_MAT_LAMBERT = 0, PT_MAT_EMISSIVE = 1, PT_MAT_MIRROR = 2, PT_MAT_OREN_NAYAR = 3 };

/* = Object{shape: Box<dyn Shape>, material: Box<dyn Material>}
 * (src/objects/object.rs:9-14) flattened to POD.  Array order == World.objects
 * order (it decides closest-hit ties, src/world.rs:281-287).
 *   shape:  sphere   = center[3], radius            (shape.rs:38-43)
 *           triangle = v0[3], v1[3], v2[3]          (shape.rs:148-152)
 *   mat:    lambert    = albedo[3]                  (material.rs:67-69)
 *           emissive   = emission[3]                (material.rs:126-129)
 *           mirror     = roughness, color[3], metallic, ior   (mirror.rs:5-14)
 *           oren-nayar = albedo[3], roughness       (material.rs:166-174)     */
typedef struct {
    uint32_t shape_tag;
    uint32_t mat_tag;
    double shape[9];
    double mat[6];
} PtObject;

enum { PT_INTEGRATOR_MIS = 0, PT_INTEGRATOR_BRDF_ONLY = 1 };
enum { PT_ACCEL_LINEAR = 0, PT_ACCEL_BVH = 1, PT_ACCEL_AUTO = 2 };

/* Compile-time constants of the reference made runtime parameters
 * (src/world.rs:16-18, src/rendering.rs:6-10).  pt_default_params() fills the
 * reference's values.                                                        */
typedef struct {
    uint32_t spp;            /* SAMPLE_NUM (world.rs:18)                       */
    uint32_t spp_offset;     /* first sample index; film is linear in spp      */
    uint32_t min_depth;      /* MIN_DEPTH = 4 (rendering.rs:6)                 */
    uint32_t max_depth;      /* MAX_DEPTH = 50 (rendering.rs:7)                */
    uint32_t integrator;     /* PT_INTEGRATOR_*; cargo feature (Cargo.toml:6)  */
    double   t_min;          /* 0.001 (rendering.rs:41,64,105)                 */
    /* Row-band tile of the image rendered by this call: the image rows are cut
     * into bands of band_rows rows; this call renders bands b with
     * b % band_count == band_index.  band_count = 1 renders the whole image.
     * Output buffers hold only this tile's rows, ascending y, row-major.      */
    uint32_t band_rows;
    uint32_t band_index;
    uint32_t band_count;
    /* Wavefront sizing: upper bound on paths resident in HBM at once (0 = library default).  It sizes the
     * context's device buffers, which persist between renders: the default is 2^26 paths (76 B of queue + 12 B of
     * sample buffer each, only as many as the job has) and 2^28 where the level-0 launch keeps its paths in
     * registers (EVERY scene of <= 128 objects, whatever its materials: 12 B of sample buffer per path, i.e. up to 3.2 GB per context --
     * per buffer set: renders of several sample batches, or renders enqueued back to back, rotate through up to three of them --
     * for a render of >= 2^28 samples -- the 400 x 400 x 3000 default job included).  A host that shares the GPU
     * sets a smaller bound: the job is then cut into more sample batches, with the same film.                */
    uint64_t max_paths_in_flight;
    uint32_t profile;        /* 1: time every path-kernel launch with HIP events (the launches of consecutive batches / renders
                                then run strictly one after the other; otherwise one may start while its predecessor's last
                                waves run dry) */
    /* Workgroups (256 threads) of the path kernel; every wave owns one private queue
     * segment.  0 = library default (about 1024 paths per wave).  Results do not
     * depend on it.                                                           */
    uint32_t workgroups;
    /* Device arithmetic.  0 (default): hardware reciprocal / square root (1 ulp).  1: IEEE correctly
     * rounded division and sqrt -- every f32 operation is then reproducible on a host CPU, the film
     * is bit-identical to the f32 CPU oracle, and the render is ~1.3x slower.  Both modes meet the
     * FP32 tolerance against the f64 reference arithmetic.                      */
    uint32_t exact_math;
    /* How World::hit_scene (world.rs:270-290) finds the closest hit.  PT_ACCEL_LINEAR: the reference's linear
     * scan over all objects.  PT_ACCEL_BVH: traversal of a BVH over the objects' bounding boxes, built on the
     * host the first time a render asks for it (beyond the reference).  The BVH only prunes the
     * scan: the primitive tests and the winner (smallest t; among equal t the highest object index) are those of
     * the linear scan, and the film is identical -- so which one runs is a performance decision only.
     * PT_ACCEL_AUTO (default): the BVH where it is faster -- scenes of more than 128 objects whose scan costs
     * more than ~512 sphere tests (a triangle counts 2.5) --, the scan otherwise and for scenes the BVH refuses
     * (an object with a NaN/inf coordinate).                                                                */
    uint32_t accel;
    /* pt_render() only: render on the first n_devices HIP devices (pt_render_multi: row bands, one RCCL
     * gather of the film to device 0).  0 or 1: device 0 alone.  The film does not depend on it.               */
    uint32_t n_devices;
} PtRenderParams;

/* Scheduling knobs of a context (pt_context_set_tuning); results never depend on them.  0 = library default.   */
typedef struct {
    uint32_t export_below;   /* a wave hands its queue segment to the continuation launch below this many paths (64) */
    uint32_t bvh_refill;     /* accel = 1: idle lanes take new rays when fewer lanes than this are tracing (44)      */
    uint32_t bvh_leaf;       /* accel = 1: leaf primitives are tested when this many lanes wait at a leaf (20)       */
    uint32_t cont_workgroups;/* workgroups of the continuation launch that finishes the handed-over tails             */
    uint32_t level0_form;    /* level-0 launch of a large batch over a scene in LDS.  0: paths stay in registers and a
                                lane whose path ends takes the batch's next one (k_paths_regen, compiled for the scene's
                                material set); with the Mirror vertices of a wave set aside and shaded 64 at a time
                                (k_paths_regen_split) if some but at most half of the objects are Mirror (the
                                reference's own scene).  1: the queue form; 2: k_paths_regen; 3: k_paths_regen_split  */
    uint32_t regen_workgroups;/* workgroups of that regenerating launch (0: what the device holds at once)             */
    uint32_t in_order;       /* 1: the regenerating launches of consecutive batches / renders run strictly one after the other (as
                                with profile = 1); 0: the next one may start while the last waves of this one run dry            */
} PtTuning;

/* Counters of the renders enqueued on a context since they were last collected (pt_sync / pt_get_stats; pt_scene_upload
 * starts afresh): normally ONE render -- synchronise after each and these are its counters.  A caller that pipelines several
 * pt_render_device calls behind one synchronisation gets their sums; total_ms then runs from the first one's start to the
 * last one's end. */
typedef struct {
    uint64_t samples;          /* camera samples FINISHED, counted on the device where a path's radiance is written to the
                                  sample buffer.  pt_sync / pt_get_stats fail with PT_ERR_HIP when it differs from
                                  samples_expected: a render lost or repeated work and its film is not to be trusted  */
    uint64_t vertices;         /* path vertices processed (iterations of the
                                  per-vertex loop)                 */
    uint64_t shadow_rays;      /* NEE visibility scans                         */
    uint32_t bounce_launches;  /* path-kernel launches (one per sample batch)  */
    uint32_t batches;          /* sample batches                               */
    uint32_t max_depth_reached;
    uint32_t reserved;
    double   bounce_kernel_ms; /* sum of HIP-event durations of the path-kernel
                                  launches (profile=1), else 0                */
    double   total_ms;         /* HIP-event duration of the whole render      */
    /* The dominant kernel on its own: the level-0 launch of every batch (the launch that generates the
     * camera rays and traces them until its waves hand their sparse tails over; the continuation
     * launches that finish those tails are the rest of bounce_kernel_ms).                          */
    uint64_t primary_vertices; /* vertices processed by the level-0 launches                      */
    double   primary_kernel_ms;/* sum of their HIP-event durations (profile=1)                    */
    uint32_t primary_launches;
    uint32_t reserved2;
    uint64_t samples_expected; /* tile pixels * spp of the renders enqueued (host arithmetic); renders captured into a graph
                                  count by replay: `samples` may then exceed this by multiples of the captured renders' size */
} PtStats;

/* ---- helpers ------------------------------------------------------------ */

/* Camera::new (src/camera.rs:50-82): axis aligned, looks down -Z. */
int pt_camera_new(const double origin[3], uint32_t width, uint32_t height,
                  double screen_distance, double fov_degrees, PtCamera* out);
/* Camera::look_at (src/camera.rs:94-130). */
int pt_camera_look_at(const double origin[3], const double target[3], const double up[3],
                      uint32_t width, uint32_t height, double fov_degrees, PtCamera* out);
/* Reference constants: spp 3000, min_depth 4, max_depth 50, MIS, t_min 1e-3. */
void pt_default_params(PtRenderParams* out);
/* Number of image rows in the tile selected by (band_rows, band_index, band_count). */
uint32_t pt_tile_rows(uint32_t height, uint32_t band_rows, uint32_t band_index, uint32_t band_count);

/* Built-in scenes: 1 = World::new() Cornell box, verbatim
 * src/world.rs:80-211; 2 = 10-sphere diffuse Cornell; 4 = n random spheres
 * (arg = n, 0 -> 10000).  Writes up to cap objects, returns the count in *n
 * (call with objs = NULL to query).                                          */
int pt_builtin_scene(uint32_t id, uint32_t arg, PtObject* objs, uint32_t cap, uint32_t* n);

/* ---- rendering ---------------------------------------------------------- */

typedef struct PtContext PtContext;

/* One context per process per GPU.  device = HIP device ordinal.
 * Threading: a context is NOT internally synchronised -- use it from one thread at a time (the
 * reference calls render_pixel from every rayon worker; this library is called once from the render
 * thread and parallelises on the GPU).  Different contexts may be used from different threads.
 * pt_last_error() is thread-local.  pt_render() serialises its callers on one cached context.   */
int pt_context_create(int device, PtContext** out);
int pt_context_destroy(PtContext* ctx);
/* Run the library's kernels on a caller-owned hipStream_t (e.g. torch's current
 * stream) instead of the context's own (non-blocking) stream.  NULL restores the context's own
 * stream; PT_STREAM_LEGACY_DEFAULT names HIP's legacy default stream, whose handle is also 0
 * (torch's default stream): pass it when the render must be ordered against work queued there.
 * Renders already enqueued on the previous stream stay ahead: the new stream waits for it once.  */
#define PT_STREAM_LEGACY_DEFAULT ((void*)(uintptr_t)1)
int pt_context_set_stream(PtContext* ctx, void* hip_stream);
int pt_context_set_tuning(PtContext* ctx, const PtTuning* tuning);

/* Copy the scene to the device (the reference's World is immutable while
 * rendering: render_pixel(&self), src/world.rs:293).  Lights are detected as
 * in src/world.rs:214-225: objects whose emit() has non-zero length.          */
int pt_scene_upload(PtContext* ctx, const PtObject* objs, uint32_t n_objs);

/* Render the tile into DEVICE buffers (no host transfer, no host synchronisation inside):
 *   d_linear_rgb: float[tile_rows*W*3], mean linear radiance  (= luminance_data,
 *                 src/world.rs:318-319)
 *   d_rgba8:      uint8[tile_rows*W*4], sqrt-gamma + truncation (= World.data /
 *                 draw(), src/world.rs:322-341); may be NULL; 4-byte aligned (a pixel is one 32-bit store).
 * Work is enqueued on the context's stream and the call returns once the last launch is
 * enqueued; the continuation launch that finishes the sparse tails of a sample batch takes
 * its path count from device memory, so the host never waits inside.  Renders of several
 * sample batches also use a second, context-owned stream for those tails; the context's
 * stream waits for it at the end, so everything is complete when that stream is.  Once the
 * buffers of a given size exist (after the first render of that size) the call allocates
 * nothing and can be captured into a hipGraph.  pt_sync() waits.                          */
int pt_render_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params,
                     float* d_linear_rgb, uint8_t* d_rgba8);
/* The same render, the film written as ONE 16-byte record per tile pixel -- float linear RGB (12 B) + RGBA8 (4 B), row-major
 * like the planes -- into d_packed (tile_rows*W*16 bytes, 16-byte aligned): the send buffer of the multi-GPU film gather
 * straight from the film resolve, without the two planes and the pt_film_pack launch in between.  pt_film_unpack (below)
 * turns gathered records into the planes.  Asynchronous like pt_render_device.                                       */
int pt_render_device_packed(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, void* d_packed);
int pt_sync(PtContext* ctx);
int pt_get_stats(PtContext* ctx, PtStats* out);
/* Debug: the 16 raw 64-bit device-side counters behind PtStats as last collected ([0] shadow rays, [1] vertices, [2] deepest
 * vertex, [3] level-0 vertices, [7] internal error flag, [8..] timing words of measurement builds, else 0).             */
int pt_debug_raw_stats(PtContext* ctx, uint64_t* out16);
/* Debug: the entries one linear scan of the uploaded scene tests: spheres, single triangles, and triangle PAIRS (two consecutive
 * triangles with the same first vertex and plane normal, e.g. the halves of a wall of World::new(), are tested together).     */
int pt_debug_scan_layout(PtContext* ctx, uint32_t* n_spheres, uint32_t* n_triangles, uint32_t* n_pairs);
/* Debug: *out = 1 when the scan consists of one run of at most 16 spheres and nothing else (k_paths_regen<MIS, diffuse> then walks
 * it without the run records), else 0.  ctx != NULL: the flag the uploaded scene carries (objs, n unused).  ctx == NULL: what an
 * upload of objs[0 .. n) would record; host only, no device.                                                                    */
int pt_debug_spheres_only(PtContext* ctx, const PtObject* objs, uint32_t n, uint32_t* out);
/* Debug, same two forms: *out = 1 when every object is Lambertian or Emissive with a non-zero emission (a path then goes on from
 * Lambertian surfaces only: k_paths_regen<MIS, diffuse> shades a one-light scene of such spheres without the other materials'
 * arms), else 0 -- a black Emissive, an OrenNayar or a Mirror object clears it.  No object: 1.                                   */
int pt_debug_lambert_surfaces(PtContext* ctx, const PtObject* objs, uint32_t n, uint32_t* out);

/* Same render with HOST output buffers (blocking): device staging is owned by the
 * context, results are copied back over PCIe.  out_rgba8 may be NULL.          */
int pt_render_host(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params,
                   float* out_linear_rgb, uint8_t* out_rgba8);

/* Progressive preview (the reference redraws World.data every 16 ms while the rayon loop fills it,
 * src/main.rs:79-90): the same render in increments of spp_step samples.  After each increment the
 * host buffers hold the mean of the samples so far and fn is called; a non-zero return stops early.
 * The final frame is bit-identical to pt_render_host with the same parameters.                    */
typedef int (*PtProgressFn)(void* user, uint32_t spp_done, uint32_t spp_total,
                            const uint8_t* rgba8, const float* linear_rgb);
int pt_render_progressive(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params,
                          uint32_t spp_step, PtProgressFn fn, void* user,
                          float* out_linear_rgb, uint8_t* out_rgba8);

/* One-shot convenience with HOST buffers: create context on device 0 (cached),
 * upload, render, copy back.  = everything src/main.rs:43-60 does.  params->n_devices > 1
 * renders through pt_render_multi on devices 0 .. n_devices-1.  The cached contexts are freed
 * by pt_shutdown() (also registered with atexit).                              */
int pt_render(const PtCamera* cam, const PtObject* objs, uint32_t n_objs,
              const PtRenderParams* params, float* out_linear_rgb, uint8_t* out_rgba8);
void pt_shutdown(void);

/* ---- multi-GPU ------------------------------------------------
 * ONE process drives n devices: one context per device, interleaved row bands (device g renders the bands b with
 * b % n == g; pixels are independent units keyed by (x, y), src/main.rs:51, so there is no collective on the data
 * path), and ONE RCCL gather (ncclGather, rccl.h:745) of the 16 B/pixel film tiles -- written by each device's film
 * resolve straight into its send buffer -- to the first device over xGMI.  The frame is bitwise independent of n.
 * RCCL is loaded with dlopen by pt_multi_create; hosts that render on one GPU never need it.
 * pt_multi_render_device only enqueues and returns: frames posted back to back are kept apart by stream order on every
 * device, and a device's share of a frame costs the host 13-14 us, so ONE host thread (the caller's; the n gather calls inside
 * one ncclGroupStart/End) keeps eight devices fed.  pt_multi_set_threads(m, 1) gives every device its own host thread inside
 * the library instead (its render launches, its ncclGather call on its own communicator): the call then returns as soon as the
 * frame is posted, and an error of a posted frame is reported by the next pt_multi_sync / pt_multi_get_stats.  The object
 * itself is not internally synchronised: call it from one thread at a time.                                          */
typedef struct PtMulti PtMulti;
int pt_multi_create(const int* devices, uint32_t n_devices, PtMulti** out);   /* contexts + ncclCommInitAll (rccl.h:236) + one 16-byte gather that connects the ranks */
int pt_multi_destroy(PtMulti* m);
uint32_t pt_multi_device_count(const PtMulti* m);
int pt_multi_set_threads(PtMulti* m, int enabled);
/* How the tiles reach the first device.  PT_EXCHANGE_RCCL (default): one ncclGather per frame.  PT_EXCHANGE_COPY: every device
 * copies its tile into the root's receive buffer with the DMA engines (hipMemcpyPeerAsync over xGMI) and the root waits for the n
 * copies -- no kernel takes part, so the exchange never waits for wave slots beside the render (RCCL's gather kernel does, see
 * pt_multi.cpp).  Same frame bit for bit.  Exercised on one device only (a same-device copy), like everything with n > 1.   */
#define PT_EXCHANGE_RCCL 0u
#define PT_EXCHANGE_COPY 1u
int pt_multi_set_exchange(PtMulti* m, uint32_t mode);
int pt_multi_scene_upload(PtMulti* m, const PtObject* objs, uint32_t n_objs);  /* replicated on every device */
int pt_multi_set_tuning(PtMulti* m, const PtTuning* tuning);                   /* pt_context_set_tuning on every device's context */
/* Post one frame: d_linear_rgb (H*W*3 floats) / d_rgba8 (H*W*4 bytes or NULL) are buffers on the FIRST device.
 * params->band_rows = 0 picks about eight bands per device; band_index / band_count are ignored.  Asynchronous.   */
int pt_multi_render_device(PtMulti* m, const PtCamera* cam, const PtRenderParams* params,
                           float* d_linear_rgb, uint8_t* d_rgba8);
int pt_multi_sync(PtMulti* m);                       /* every posted frame is complete on every device */
int pt_multi_get_stats(PtMulti* m, PtStats* out);    /* counters of the frames since the last collection summed over the devices, times of the slowest */
int pt_multi_render_host(PtMulti* m, const PtCamera* cam, const PtRenderParams* params,
                         float* out_linear_rgb, uint8_t* out_rgba8);
/* What the object is made of -- a record of an N-device run carries these to show that N ranks took part.          */
typedef struct {
    uint32_t n_devices;
    uint32_t comm_count;      /* ncclCommCount (rccl.h) of the first device's communicator; 0: a debug object without RCCL */
    uint32_t rccl_version;    /* ncclGetVersion, e.g. 22203                                                         */
    uint32_t threaded;        /* 1: one host thread per device                                                      */
    uint64_t frames;          /* frames posted since creation                                                       */
    double   enqueue_us_sum;  /* host time spent enqueueing one frame, summed over the devices (mean per frame) ...  */
    double   enqueue_us_max;  /* ... and the slowest device's share of it: what a frame costs the host with threads  */
    uint32_t exchange;        /* PT_EXCHANGE_*                                                                      */
    uint32_t reserved_;
} PtMultiInfo;
int pt_multi_info(PtMulti* m, PtMultiInfo* out);
/* One shot with host buffers (a cached PtMulti for the device list; pt_shutdown frees it). */
int pt_render_multi(const int* devices, uint32_t n_devices, const PtCamera* cam, const PtObject* objs,
                    uint32_t n_objs, const PtRenderParams* params, float* out_linear_rgb, uint8_t* out_rgba8);

/* The two kernels pt_multi_* runs around its ncclGather, for hosts that bring their own collective (one process per GPU:
 * pathtrace_amd/dist.py over torch.distributed / RCCL, an MPI host, ...).  Both work on DEVICE memory of the calling
 * thread's current HIP device and are enqueued on hip_stream (a hipStream_t; NULL = that device's default stream).
 * The caller guarantees that hip_stream was created on that current device (hipSetDevice before the call in a
 * multi-device host): a stream of another device makes the launch fail with PT_ERR_HIP, it is not redirected.
 *   pt_film_pack:   a rank's tile (d_linear_rgb: n_pixels * 3 floats, d_rgba8: n_pixels * 4 bytes or NULL) ->
 *                   d_packed, 16 bytes per pixel (12 B linear RGB + 4 B RGBA8): both film planes in ONE gather.
 *   pt_film_unpack: the gathered tiles (rank g's tile, padded to max_rows rows, at d_gathered + g * max_rows * width *
 *                   16 bytes) -> the frame in image order (d_linear_rgb: width * height * 3 floats, d_rgba8 or NULL),
 *                   for the interleaved bands of PtRenderParams (band b belongs to rank b % n_ranks).               */
int pt_film_pack(void* hip_stream, const float* d_linear_rgb, const uint8_t* d_rgba8, uint32_t n_pixels, void* d_packed);
int pt_film_unpack(void* hip_stream, const void* d_gathered, uint32_t width, uint32_t height, uint32_t band_rows,
                   uint32_t n_ranks, uint32_t max_rows, float* d_linear_rgb, uint8_t* d_rgba8);

/* Debug / parity entry: the frame of an n_virtual-device render on ONE context (tiles rendered one after another,
 * device-to-device copies where pt_multi_* runs ncclGather): partition, packed resolve and unpack for any n on a one-GPU box. */
int pt_debug_multi_emulate(PtContext* ctx, uint32_t n_virtual, const PtCamera* cam, const PtRenderParams* params,
                           float* out_linear_rgb, uint8_t* out_rgba8);
/* Debug object: a PtMulti of n contexts that all sit on ONE device, without RCCL -- each context copies its tile into the
 * receive buffer on its own stream where the real object calls ncclGather.  Everything else is the real thing: the host
 * threads, frames posted back to back, the packed resolve, the row permutation, the statistics.  Rehearses (and times:
 * pt_multi_info) an n-device frame on a one-GPU box.                                                                */
int pt_debug_multi_create_shared(int device, uint32_t n, PtMulti** out);
/* Host-only self test of the per-device feeder threads (no GPU needed): posts n_frames jobs to each of n_workers threads
 * the way pt_multi_render_device posts frames and returns the start / end log of the jobs in order_out (2 * n_workers *
 * n_frames entries: worker << 32 | frame, bit 63 set on the end record); fail_at >= 0 makes job worker * n_frames + frame
 * fail, and the call then returns the status the drain reported.                                                     */
int pt_debug_feeder_selftest(uint32_t n_workers, uint32_t n_frames, uint32_t spin, int32_t fail_at,
                             uint64_t* order_out, uint32_t* n_out);

/* The launch scheduler of a context, host only (no GPU needed).  A render is planned by a PURE function (csrc/pt_sched.h):
 * (scheduling state of the context, job) -> the list of stream operations the render enqueues -- path-kernel launches and film
 * resolves with their stream, buffer set, lane, exchange region and counters, the event records / waits that order them, the
 * fills of counters and statistics.  pt_render_device* executes exactly such a list.  These entries run the same function on a
 * scheduling state of their own, so that a test can drive random sequences of jobs through it and check the invariants of
 * DESIGN.md 3 with a happens-before simulator (tests/test_sched_cpu.py).  Field meanings: csrc/pt_sched.h (Job, Op).         */
typedef struct {
    uint32_t n_batches, regen, split, hand_off, regen_export, profile, in_order, capturing;
    uint32_t grid, regen_grid, cont_grid, regen_capacity, fixed_grid, counter_words;
    uint64_t xchg_need;
} PtSchedJob;
typedef struct {
    uint32_t kind, stream, event, pool, set, lane, level, own_queue, ovf_par, batch, grid, seq, core, flags, zero_words, reserved;
    uint64_t xchg_off, xchg_len;
} PtSchedOp;
typedef struct PtSched PtSched;
int pt_debug_sched_create(PtSched** out);
void pt_debug_sched_destroy(PtSched* s);
/* Plans one render and advances the state.  faults: bit 0 / bit 1 switch round 4's two scheduling bugs back on (pt_sched.h:
 * Faults; for the test that shows they are caught).  fail_after < the plan's length: the operation of that index fails as a
 * HIP call would -- only the operations before it are returned, followed by the host synchronisation of the recovery, and the
 * state is what render_impl's recovery leaves.  *lanes = 1 if the render took the lanes.                                     */
int pt_debug_sched_render(PtSched* s, const PtSchedJob* job, uint32_t faults, uint32_t fail_after, PtSchedOp* ops, uint32_t cap,
                          uint32_t* n_ops, uint32_t* lanes);
int pt_debug_sched_sync(PtSched* s, uint32_t collect);        /* pt_sync: everything enqueued is complete (collect: statistics read and cleared) */
/* The launch sizing of a render, host only (no GPU needed).  What pt_render_device* derives from the scene, the parameters, the
 * tuning and the device before it allocates or enqueues anything -- the level-0 form, the batches, every grid, segment and queue
 * size, the job the scheduler plans -- is a PURE function too (csrc/pt_shape.h); this entry runs it on the caller's numbers.
 * occupancy: workgroups per CU the runtime reports for the form's regenerating kernel with the scene's LDS blob (0: unknown).
 * out->job can be handed to pt_debug_sched_render as it is; ops (optional): n_ops operations of such a plan -- launches[k]
 * receives the per-launch words of operation k where that is a launch, zeros otherwise.  A tile above the cap:
 * PT_ERR_UNSUPPORTED with out->over_cap = 1 and out->cap.  Field meanings: csrc/pt_shape.h (In, Form, Shape, Launch).          */
typedef struct {
    uint64_t np, max_paths_in_flight;
    uint32_t spp, workgroups, accel, profile, list, list_regen, inject, n_objs, blob_f4, diffuse_only, split_ok, n_cus;
    uint32_t export_below, cont_workgroups, level0_form, regen_workgroups, in_order, capturing;
    uint32_t inject_spp, reserved;   /* inject_spp: samples per pixel that given paths bring (0: one); additive, 0 = as before */
} PtShapeIn;
typedef struct {
    uint32_t lds_job, split, regen_scene, over_cap;
    uint64_t cap, n_paths_max, ovf_slots, q_slots_cont, q_slots;
    uint32_t np, spp, nb_max, n_batches, export_small, paths_per_wave, small_scene, hand_off, regen, overlap;
    uint32_t grid, nw, seg_cap, regen_per_cu, regen_capacity, regen_grid, regen_launch_grid, cont_grid, nw_cont, seg_cap_cont;
    uint32_t regen_export, reserved;
    PtSchedJob job;
} PtShapeOut;
typedef struct {
    uint32_t s0, nb, n_first, seg_cap, src_mode, export_below, regen_static, reserved;
} PtShapeLaunch;
int pt_debug_render_shape(const PtShapeIn* in, uint32_t occupancy, PtShapeOut* out, const PtSchedOp* ops, uint32_t n_ops,
                          PtShapeLaunch* launches);
/* Test hook: the n-th stream operation (0-based) of the NEXT render on this context fails as if its HIP call had (n < 0: none). */
int pt_debug_fail_after(PtContext* ctx, int64_t n);
/* Launch log: which compiled instance of the path kernels each launch took.  One code per path-kernel launch, recorded on the
 * host as the launch is enqueued: bits 0-1 family (0 k_paths, 1 k_paths_bvh, 2 k_paths_regen, 3 k_paths_regen_split), bit 2
 * MODE of k_paths (0 scene in LDS, 1 tiled scan), bit 3 MIS, bit 4 OVF (continuation launch), bits 5-6 material set (DIFFUSE
 * of k_paths / k_paths_bvh; MATS of k_paths_regen and PLAIN of k_paths_regen_split: 0 all, 1 diffuse only, 2 no Mirror),
 * bit 7 LIST (pixel list), bit 8 exact arithmetic.  pt_debug_launch_log writes the codes of the launches since its last
 * call, in launch order (up to cap; *n = codes written), and clears them.  pt_debug_path_instances writes the table of
 * every code the dispatch can record (up to cap; *n = the table's length; out may be NULL).                            */
int pt_debug_launch_log(PtContext* ctx, uint32_t* out, uint32_t cap, uint32_t* n);
int pt_debug_path_instances(uint32_t* out, uint32_t cap, uint32_t* n);

/* World::render_pixel (src/world.rs:293-333) -- the seam the reference's rayon loop calls at
 * src/main.rs:55 -- for an arbitrary list of n pixels: xy = n * (x, y), y = film row (top-down, the y
 * of the seed (y<<32)|x, main.rs:51).  Every listed pixel gets exactly the samples a full render gives
 * it (same key, same sample indices spp_offset .. spp_offset+spp-1), so out_linear_rgb[3i..] /
 * out_rgba8[4i..] are bit-identical to that pixel of the full film.  out_samples (optional,
 * n * spp * 3 floats, [pixel][sample][rgb]) receives the radiance of every camera sample =
 * RenderingStrategy::ray_color's return value (rendering.rs:34,214; what the reference's pixel
 * diagnostics print, world.rs:378-417); it needs the whole list in one sample batch
 * (n * spp <= max_paths_in_flight).  Host buffers, blocking.  band_* of params must select the
 * whole image.                                                                                */
int pt_render_pixels(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params,
                     const uint32_t* xy, uint32_t n, float* out_linear_rgb, uint8_t* out_rgba8,
                     float* out_samples);

/* Adaptive sampling: every pixel gets spp_min samples, then passes of spp_step more go to the pixels whose noise estimate has
 * not converged, up to params->spp (= spp_max; the last pass is cut to it).  The rule (pathtrace_amd/csrc/pt_adaptive.h), per
 * pixel over its samples' luminance L = 0.2126 r + 0.7152 g + 0.0722 b in f64, S1 = sum L, S2 = sum L^2, checked at
 * n = spp_min, spp_min + spp_step, ...:
 *   mean = S1 / n,  var = max(0, (S2 - S1 mean) / (n - 1)),  se = sqrt(var / n)
 *   converged  <=>  se <= rel_tol * max(mean, abs_floor)   (never with rel_tol = 0 or a non-finite sum)
 * Pixel (x, y) gets samples spp_offset .. spp_offset + n - 1 and its film is their mean through the same gamma / `as u8`
 * steps as every render: bit-identical to pt_render_pixels / pt_render_host of that pixel with spp = n.  out_spp = n,
 * out_rel_err = se / max(mean, abs_floor) at n (both optional, width * height entries).  Host buffers, blocking; the whole
 * image (band_count = 1).  PT_ERR_INVALID_ARG: spp_min < 2, spp_step = 0, params->spp < spp_min, rel_tol negative or not
 * finite, abs_floor <= 0.                                                                                               */
typedef struct {
    uint32_t spp_min;    /* samples every pixel gets first (>= 2)                                   */
    uint32_t spp_step;   /* samples per later pass, for the pixels not yet converged (>= 1)          */
    double rel_tol;      /* a pixel stops once se(L) <= rel_tol * max(mean(L), abs_floor)            */
    double abs_floor;    /* keeps dark pixels from running to spp_max (> 0)                          */
} PtAdaptive;
int pt_render_adaptive(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, const PtAdaptive* ad,
                       float* out_linear_rgb, uint8_t* out_rgba8, uint32_t* out_spp, float* out_rel_err);

/* First-hit feature buffers: one 32-byte record per image pixel, row-major, whole image, 16-byte aligned:
 *   {albedo r, g, b, emitter, normal x, y, z, depth}
 * For samples spp_offset .. spp_offset + n_samples - 1 the pass takes the primary ray the path kernels take (same key, same
 * jitter draws), finds its closest hit in [t_min, inf) with the scan or BVH params->accel selects, and maps it to a record:
 *   Lambert / OrenNayar: albedo clamped to [0, 1], emitter 0;  Mirror: color clamped to [0, 1], emitter 0;
 *   Emissive: albedo (1, 1, 1), emitter 1;  the three with the face-forwarded HitRecord normal and depth = t;
 *   miss: albedo (1, 1, 1), emitter 0, normal 0, depth 0.
 * The records are summed in sample order in f32 and each sum is divided by n_samples; params->exact_math selects the
 * arithmetic mode (exact: bit-identical to the f32 oracle's camera rays and hit records).  Asynchronous on the context's
 * stream like pt_render_device; the scratch (a bounded batch of rays and hits) is context-owned and grows on first use.
 * PT_ERR_INVALID_ARG: n_samples = 0, band_count > 1 (the pass works on the whole image only).                         */
int pt_render_features_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t n_samples,
                              float* d_features);

/* Edge-avoiding a-trous wavelet denoiser guided by variance (spatial SVGF, no temporal part).  Per pixel p, with c the
 * linear film and the feature records above:
 *   demodulate   a = max(albedo, 1e-3) per channel, u = c / a, L(u) = 0.2126 r + 0.7152 g + 0.0722 b
 *   variance     var = the 3x3 population variance of L(u); taps outside the image are skipped
 *   iteration i = 0 .. iterations-1, step h = 2^i: 5x5 taps at (dx, dy) h, B3-spline weights
 *                k = [1/16, 1/4, 3/8, 1/4, 1/16] (x) same, taps outside the image skipped;
 *                g_p = sqrt(3x3 Gaussian [1/4, 1/2, 1/4] (x) same of var, renormalised over the in-image taps);
 *                q != p:  w = k max(0, n_p.n_q)^sigma_n exp(-|L_p - L_q| / (sigma_l g_p + 1e-10)
 *                                                    -|d_p - d_q| / (sigma_d h max(d_p, 1e-3) + 1e-10)),
 *                         w = 0 when emitter_p > 0 or emitter_q > 0;  the centre tap: w = k;
 *                         w = 0 when n_p.n_q <= 0, for every sigma_n, 0 included (0^0 is not consulted: orthogonal
 *                         and opposite normals, and every miss pixel, whose normal is 0, never mix);
 *                         a tap with w = 0 by one of these cases (outside the image, an emitter, n_p.n_q <= 0) is not
 *                         read: nothing of pixel q, a NaN or an infinity included, reaches pixel p through it;
 *                u' = sum w u_q / sum w,  var' = sum w^2 var_q / (sum w)^2
 *   remodulate   c' = u a; the RGBA8 plane is c' through the sqrt-gamma / clamp / `as u8` steps of every render.
 * iterations = 0 gives u a of the input.  The device computes in f32 (the sums as u_p + sum w (u_q - u_p) / sum w).
 * pt_default_denoise: 5 iterations, sigma_l 4, sigma_n 128, sigma_d 0.025.                                            */
typedef struct {
    uint32_t iterations;
    float sigma_l;           /* luminance edge stop, in units of the local standard deviation */
    float sigma_n;           /* normal exponent                                                */
    float sigma_d;           /* depth edge stop, relative to the depth per unit step           */
} PtDenoise;
void pt_default_denoise(PtDenoise* out);
/* Device buffers: d_linear_rgb width*height*3 floats, d_features width*height*8 floats (16-byte aligned), d_out_linear
 * width*height*3 floats (not the input), d_out_rgba8 width*height*4 bytes or NULL (4-byte aligned).  Asynchronous on the
 * context's stream; two context-owned float4 planes of (u, var) grow on first use.  Needs no scene.                   */
int pt_denoise_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_linear_rgb, const float* d_features,
                      const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba8);
/* One call with HOST buffers (blocking): the render of params, then the feature pass of min(feature_samples, params->spp)
 * samples from params->spp_offset, then the filter.  out_rgba8, out_noisy_linear (the render's linear film) and out_features
 * (width*height*8 floats) may be NULL.  The whole image only (band_count = 1).                                         */
int pt_render_denoised(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                       const PtDenoise* dn, float* out_linear_rgb, uint8_t* out_rgba8, float* out_noisy_linear,
                       float* out_features);

/* The filter guided by each pixel's MEASURED variance (additive to ABI 6).  pt_render_adaptive already measures,
 * per pixel, the squared standard error of the mean luminance its stopping rule tests; the three entries below hand it to the
 * a-trous filter in place of the 3x3 guess, which mistakes texture and edges for noise and, after an adaptive render, compares
 * neighbours with different sample counts.
 *
 * pt_denoise_var_device is pt_denoise_device in every rule but "variance": per pixel, var = d_var[p] when that is finite and
 * >= 0; any other entry (NaN, +-inf, negative: "no measurement") takes the 3x3 population variance of pt_denoise_device.  With
 * every entry NaN it is bit-identical to pt_denoise_device; with iterations = 0 the plane is not read.  d_var: width*height
 * floats on the device, 4-byte aligned, in units of L(u)^2 (the DEMODULATED luminance).  Buffers, argument checks,
 * context-owned planes and asynchrony as pt_denoise_device; PT_ERR_INVALID_ARG also for a NULL d_var.  Needs no scene. */
int pt_denoise_var_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_linear_rgb, const float* d_features,
                          const float* d_var, const PtDenoise* dn, float* d_out_linear, uint8_t* d_out_rgba8);
/* The variance plane of the last pt_render_adaptive (or pt_render_adaptive_denoised) this context COMPLETED.  The context keeps
 * that render's per-pixel f64 sums (sum R, sum G, sum B, S1 = sum L, S2 = sum L^2) and sample counts n on the device until
 * the next adaptive render is asked for; one that returns an error, for whatever reason, leaves none; pt_scene_upload and
 * the other scene entries do not touch them.  Per pixel, with the albedo of its feature record (pathtrace_amd/csrc/pt_denoise_var.h, f64):
 *   mean = S1 / n,  var_c = max(0, (S2 - S1 mean) / (n - 1)) / n          (se^2 of the stopping rule)
 *   c_k = sum_k / n,  a_k = max(albedo_k, 1e-3),  L_u = 0.2126 c_0/a_0 + 0.7152 c_1/a_1 + 0.0722 c_2/a_2
 *   var_u = var_c (L_u / mean)^2
 * d_var[p] = (float)var_u when mean > 0 and L_u, var_u are finite; NaN when S1 or S2 is not finite; else 0 (a black pixel,
 * a miss; a pixel whose samples are all equal, e.g. one that sees the light directly, has var_c = 0).  The squared ratio of
 * the two mean luminances carries the film's variance to the demodulated colour the filter works on: exact for a grey
 * albedo, an approximation otherwise.  d_features as pt_render_features_device writes them (16-byte aligned), d_var
 * width*height floats (4-byte aligned).  Asynchronous on the context's stream; needs no scene.  PT_ERR_INVALID_ARG: the
 * context holds no completed adaptive render, or width x height is not that render's size.                               */
int pt_adaptive_variance_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_features, float* d_var);
/* One call with HOST buffers (blocking), the adaptive counterpart of pt_render_denoised: pt_render_adaptive(params, ad), then
 * pt_render_features_device of min(feature_samples, ad->spp_min) samples from params->spp_offset (the samples every pixel
 * has), pt_adaptive_variance_device and pt_denoise_var_device; bit-identical to calling the four.  out_linear_rgb is the
 * denoised film; out_rgba8 (of the denoised film), out_noisy_linear (the adaptive render's film), out_spp and out_rel_err
 * (as pt_render_adaptive) and out_var (the variance plane, width*height floats) may be NULL.  The whole image only.      */
int pt_render_adaptive_denoised(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, const PtAdaptive* ad,
                                uint32_t feature_samples, const PtDenoise* dn, float* out_linear_rgb, uint8_t* out_rgba8,
                                float* out_noisy_linear, uint32_t* out_spp, float* out_rel_err, float* out_var);

/* Temporal accumulation with camera reprojection in front of the a-trous filter (the temporal half of SVGF).
 * Per-frame history that the context owns.  Image W x H, film row y top-down; the frame's camera (o, l, hz, vt) =
 * PtCamera.origin / lower_left / horizontal / vertical, the history's (o', l', hz', vt'); c the linear film, the pixel's
 * feature record {albedo, emitter, normal n, depth d}; a = max(albedo, 1e-3), u_c = c / a, L_c = L(u_c) as above.
 *   1 fresh        a pixel has no history when the history is empty (after pt_temporal_reset, on first use, after a
 *                  pt_scene_upload, or when W or H changed), when d_p = 0 (a miss), or when the reprojection fails
 *   2 reprojection s = (x + 0.5)/(W - 1), t = (H - 1 - y + 0.5)/(H - 1), D = l + s hz + t vt - o, P = o + d_p D/|D|;
 *                  solve s' hz' + t' vt' - lambda (P - o') = o' - l' for (s', t', lambda): fails when singular or lambda <= 0;
 *                  x' = s'(W - 1) - 0.5, y' = H - 0.5 - t'(H - 1), d_exp = |P - o'|.  When the camera equals the history's
 *                  field by field: x' = x, y' = y, d_exp = d_p exactly.
 *   3 taps         the bilinear 2x2 taps around (x', y') with the usual weights; tap q is valid iff it lies inside the
 *                  image, d_q > 0, |d_q - d_exp| <= depth_tol d_exp, n_p.n_q >= normal_tol and (emitter_p > 0) ==
 *                  (emitter_q > 0), with d_q, n_q, emitter_q of the history's frame.  S = the sum of the valid weights;
 *                  S < 1e-2: fresh; else u_h, m1_h, m2_h, n_h = the valid-weighted means / S.  A fresh pixel has n_h = 0.
 *   4 accumulate   (f32) n = n_h + 1, alpha' = max(alpha, 1/n), u = u_h + alpha'(u_c - u_h), m1 = m1_h + alpha'(L_c - m1_h),
 *                  m2 = m2_h + alpha'(L_c^2 - m2_h); a fresh pixel: u = u_c exactly
 *   5 variance     n >= 4: var = max(0, m2 - m1^2); else the 3x3 spatial variance of pt_denoise_device
 *   6 filter       (u, var) through the a-trous iterations and the remodulation of pt_denoise_device (current albedo)
 *   7 store        the history keeps the unfiltered (u, m1, m2, n), the frame's normal, depth and emitter flag, and the camera
 * The first frame after a reset is bit-identical to pt_denoise_device.  The device computes the reprojection in f64, the
 * rest in f32.  pt_default_temporal: alpha 0.2, depth_tol 0.1, normal_tol 0.9.                                          */
typedef struct {
    float alpha;             /* least blend weight of the new frame, in [0, 1]; 0 = running mean     */
    float depth_tol;         /* relative depth tolerance of a history tap                            */
    float normal_tol;        /* least cosine between the pixel's normal and a history tap's normal   */
} PtTemporal;
void pt_default_temporal(PtTemporal* out);
/* Empties the context's history: the next frame is fresh everywhere. */
int pt_temporal_reset(PtContext* ctx);
/* Device buffers as pt_denoise_device, the image size = cam->width x cam->height (at least 2 x 2).  Asynchronous on the
 * context's stream; needs no scene.  Context-owned memory, grown on first use and freed with the context: the two (u, var)
 * planes of pt_denoise_device and two history buffers of 48 bytes per pixel (double-buffered: 96 bytes per pixel).
 * PT_ERR_INVALID_ARG as pt_denoise_device, and alpha not in [0, 1], a negative or non-finite tolerance.                 */
int pt_denoise_temporal_device(PtContext* ctx, const PtCamera* cam, const float* d_linear_rgb, const float* d_features,
                               const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear, uint8_t* d_out_rgba8);
/* One frame with HOST buffers (blocking), the temporal counterpart of pt_render_denoised: the render of params, the feature
 * pass of min(feature_samples, params->spp) samples from params->spp_offset, then pt_denoise_temporal_device.         */
int pt_render_denoised_temporal(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                                const PtDenoise* dn, const PtTemporal* tp, float* out_linear_rgb, uint8_t* out_rgba8,
                                float* out_noisy_linear, float* out_features);

/* Moving objects in the temporal denoiser (additive to ABI 6).  pt_scene_upload empties the history; these
 * entries change the scene and keep it.
 *
 * pt_scene_update makes the scene pt_scene_upload would make of the same objects (same records, same lazy BVH rebuild, same
 * restart of the statistics: a render after it is bit-identical to one after pt_scene_upload) and keeps the temporal history.
 * It needs an uploaded scene with the same n_objs and the same shape_tag at every index: otherwise PT_ERR_INVALID_ARG, and the
 * context is untouched.  The context keeps the f64 shape[9] of every object twice: of the current scene, and of the HISTORY
 * POSE, the scene as it was at the most recent temporal call (either entry) that stored a history frame.  Any number of
 * updates may lie between two temporal frames.                                                                          */
int pt_scene_update(PtContext* ctx, const PtObject* objs, uint32_t n_objs);
/* Device-side BVH refit (additive to ABI 6).
 *
 * pt_scene_refit is pt_scene_update in every respect but one: same argument checks, same records, same restart of the
 * statistics, the temporal history kept -- but a BVH the context holds is NOT dropped.  It is refitted on the device, on the
 * context's stream behind the new records: the tree keeps its topology (which objects share a leaf, which nodes are children
 * of which), and the leaf records, every child box and the quantisation grid are recomputed from the new shapes.  No tree
 * array crosses PCIe and the binned-SAH builder does not run.  Without a tree (no accel = 1 render yet, or the BVH was
 * refused or failed) the call IS pt_scene_update: the tree is built at first use.  A pose with a NaN/inf coordinate drops the
 * tree and refuses the BVH as building it would: accel = 1 then fails with PT_ERR_UNSUPPORTED, PT_ACCEL_AUTO takes the scan.
 * pt_scene_upload, pt_scene_update and pt_scene_refit may be mixed freely on one context.
 *
 * THE FILM NEVER DEPENDS ON THE REFIT.  The tree only decides which primitives a ray is tested against; every box of a
 * refitted tree encloses what is beneath it, so a render over it is bit-identical to the linear scan's, however far the
 * objects moved.  Only the traversal TIME depends on it: objects that were neighbours when the tree was built and have
 * drifted apart leave large, overlapping boxes.  pt_scene_bvh_cost measures that:
 *   cost = the sum, over every used child slot of every node, of the half-area of the child box the device traverses
 * (exact integer sums on the 16-bit grid, scaled by the grid cell in f64).  cost_now is the tree as it is (the call waits
 * for the context's stream), cost_at_build the tree as the builder left it, refits the refits since then.  A caller who sees
 * cost_now / cost_at_build grow calls pt_scene_update ONCE: the next render rebuilds the tree for the current pose.
 * Any output may be NULL.  PT_ERR_INVALID_ARG when the context holds no tree.                                            */
int pt_scene_refit(PtContext* ctx, const PtObject* objs, uint32_t n_objs);
int pt_scene_bvh_cost(PtContext* ctx, double* cost_now, double* cost_at_build, uint32_t* refits);
/* Device-side BVH build (additive to ABI 6).
 *
 * pt_scene_rebuild is pt_scene_update in every respect but one: same argument checks with the context untouched on failure,
 * same records, same restart of the statistics, the temporal history kept -- but the context afterwards HOLDS A TREE FOR THE NEW
 * POSE, built on the device, on the context's stream behind the new records, whether or not it held one before.  The tree is
 * the Morton tree of DESIGN.md 5f: the objects ordered along a Morton curve over the scene's grid (keys and a radix sort on the
 * device), four consecutive objects per leaf, and a topology that depends on the object count alone (planned on the host once
 * per count and cached on the device), filled in by the launches of the refit.  No tree array crosses PCIe, the binned-SAH
 * builder does not run, and the call adds no wait for the device of its own.  Called with the uploaded objects right after
 * pt_scene_upload it is a first build without the host builder.  A later pt_scene_refit refits this tree; cost_at_build of
 * pt_scene_bvh_cost is the cost after this build, refits restarts at 0.
 * A pose with a NaN/inf coordinate drops the tree and refuses the BVH exactly as pt_scene_refit does.  An object count for
 * which no tree fits the traversal stack (more than 2^25 objects) gives PT_ERR_UNSUPPORTED with the context untouched: use
 * pt_scene_update.  pt_scene_upload, pt_scene_update, pt_scene_refit and pt_scene_rebuild may be mixed freely.
 * THE FILM NEVER DEPENDS ON THE BUILDER.  A Morton tree is built faster and traversed somewhat slower than the host's SAH
 * tree (docs/EXPERIMENTS.md, "Device-side build"); when to refit, rebuild here or rebuild on the host is the caller's policy. */
int pt_scene_rebuild(PtContext* ctx, const PtObject* objs, uint32_t n_objs);
/* Device-side BVH build in a chosen order (additive to ABI 6).
 *
 * order = PT_BVH_ORDER_MORTON: pt_scene_rebuild, bit for bit.
 * order = PT_BVH_ORDER_MEDIAN: pt_scene_rebuild in every respect -- checks, records, statistics, kept history, refits = 0,
 * cost_at_build, the NaN/inf rule, PT_ERR_UNSUPPORTED for a count without a plan, the topology, the leaf layout and the refit
 * launches -- except the order in which the objects fill the leaf slots: instead of a sort along a Morton curve, a recursive
 * median split along the child boundaries of the count-only topology (per step: the widest axis of the objects' grid cells,
 * the range ordered by (cell on that axis, object index); ptbvh::build_median is the specification).  A node's children are
 * then boxes side by side instead of stretches of a curve, which roughly halves the tree's cost (docs/EXPERIMENTS.md,
 * "Device-side build: median order").  The split plan depends on the object count alone: planned on the host once per count
 * and kept on the device; the call adds no wait for the device.
 * Any other order: PT_ERR_INVALID_ARG, context untouched.  THE FILM NEVER DEPENDS ON THE ORDER.                            */
enum { PT_BVH_ORDER_MORTON = 0, PT_BVH_ORDER_MEDIAN = 1 };
int pt_scene_rebuild_ordered(PtContext* ctx, const PtObject* objs, uint32_t n_objs, uint32_t order);
/* The motion map of object k, x -> A x + b in f64, carries a point of the current pose to the same material point of the
 * history pose:  sphere (c, r) now, (c', r') then: A = (r'/r) I, b = c' - (r'/r) c;  triangle (v0, v1, v2) now, primed then:
 * e1 = v1 - v0, e2 = v2 - v0, n = (e1 x e2)/|e1 x e2|, E = [e1 e2 n] as columns, A = E' E^-1, b = v0' - A v0.
 * INVALID: a radius <= 0, a triangle of zero area, or a non-finite entry.  IDENTITY: the nine shape fields are bitwise equal
 * now and then (decided on the fields; then A = I, b = 0 exactly).
 * Host only, needs no GPU: out_maps n x 12 doubles (A row-major, then b), out_flags n words (bit 0 identity, bit 1 invalid). */
int pt_debug_motion_maps(const PtObject* prev_objs, const PtObject* cur_objs, uint32_t n, double* out_maps, uint32_t* out_flags);
/* One int32 per image pixel, row-major: the object index hit by the primary ray of sample params->spp_offset, -1 for a miss.
 * The ray, its key and jitter, [t_min, inf), params->accel and params->exact_math are the feature pass's (its first sample's
 * hit ids, copied out of the pass's scratch).  Whole image only; asynchronous on the context's stream.                  */
int pt_render_feature_ids_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, int32_t* d_ids);
/* pt_denoise_temporal_device plus d_ids (width*height int32, 4-byte aligned): per call the maps current pose -> history pose
 * go to a context-owned device buffer on the context's stream, out of host staging that the context owns (no wait for the stream).
 * Rules 1-3 and 7 above are amended, 4-6 are untouched:
 *   1' fresh, additionally: id_p < 0, id_p >= n_objs, or the map of id_p is invalid (the ids are the caller's: the device
 *                  checks them against n_objs before it reads a map)
 *   2' reprojection P as in 2, k = id_p, P_h = A_k P + b_k in f64; the system of 2 is solved with P_h in place of P and
 *                  d_exp = |P_h - o'|;  n_h = A_k n_p normalised in f64 and rounded to f32 (n_p when its length is 0).
 *                  Map k the identity: P_h = P and n_h = n_p exactly; the camera also equal to the history's field by
 *                  field: x' = x, y' = y, d_exp = d_p exactly (the shortcut of 2, per pixel)
 *   3' taps        the conditions of 3 with n_h in the normal gate, and the id gate: the tap's stored id is unknown, or equals
 *                  id_p, or neither the map of id_p nor the map of the tap's id is anything but the identity.  (The last
 *                  clause keeps a scene in which nothing moved bit-identical to pt_denoise_temporal_device under a moving
 *                  camera: two objects that both stand still gate each other by depth and normal alone, as there.)
 *   7' store       the history's second record is (m2, n, emitter, id_p + 1 as float); 0 = unknown, which is what
 *                  pt_denoise_temporal_device stores (the lane is read by nothing else), and what a pixel with id_p < 0 or
 *                  id_p >= n_objs stores.  The two entries may be mixed freely on one context.
 * Needs a scene (PT_ERR_INVALID_ARG without); PT_ERR_UNSUPPORTED for more than 2^24 - 2 objects (id + 1 is kept in f32).
 * Lighting that changes because an object moved is forgotten at the rate alpha, as under a moving camera -- unless the
 * caller raises alpha where it changed: the temporal gradients below.                                                     */
int pt_denoise_temporal_motion_device(PtContext* ctx, const PtCamera* cam, const float* d_linear_rgb, const float* d_features,
                                      const int32_t* d_ids, const PtDenoise* dn, const PtTemporal* tp, float* d_out_linear,
                                      uint8_t* d_out_rgba8);
/* pt_render_denoised_temporal with the ids pass and the motion entry; out_ids (width*height int32) may be NULL. */
int pt_render_denoised_motion(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                              const PtDenoise* dn, const PtTemporal* tp, float* out_linear_rgb, uint8_t* out_rgba8,
                              float* out_noisy_linear, float* out_features, int32_t* out_ids);

/* Temporal gradients: a per-pixel blend weight where the LIGHTING changed (additive to ABI 6; after the temporal
 * gradient of A-SVGF, Schied et al. 2018).  The motion entry above follows an object's geometry; the shadow it left behind, or
 * a light that was dimmed, fades at the rate alpha.  These entries measure where the radiance changed and raise alpha there.
 *
 * Samples are addressed by (pixel, sample index) and a pixel-list render is bit-identical to the same pixel of a full render,
 * so the PREVIOUS frame's sample re-traced in the CURRENT scene is one list render with the previous frame's parameters; on
 * an unchanged scene it reproduces the previous film bit for bit and the gradient is exactly 0.  The rule
 * (pathtrace_amd/csrc/pt_gradient.h, f64), image W x H:
 *   strata       3 x 3 blocks, SW = ceil(W/3) by SH = ceil(H/3), clipped at the right and bottom edges; stratum (bx, by) has
 *                one gradient pixel (min(3 bx + seed % 3, W - 1), min(3 by + (seed / 3) % 3, H - 1)); the caller advances seed
 *                per frame so that the gradient pixel walks through its block
 *   record       c_new the gradient pixel's re-traced film, c_old its film in d_prev_linear, L(c) = 0.2126 r + 0.7152 g +
 *                0.0722 b:  delta = |L_new - L_old|, N = max(L_new, L_old); not finite when either L is not
 *   per pixel    over the strata (x/3 + i, y/3 + j), |i|, |j| <= radius, inside the grid, row-major: D = sum delta, Nn = sum N;
 *                lambda = 1 when a record of the window is not finite, min(1, scale D / Nn) when Nn > 0, else 0;
 *                d_alpha[p] = (float)(alpha_min + lambda (1 - alpha_min));  D = 0 gives alpha_min exactly
 * pt_default_gradient: radius 1, scale 1.
 *
 * pt_temporal_gradient_device: d_prev_linear is the previous frame's noisy linear film (W*H*3 floats on the device, 4-byte
 * aligned), rendered with prev_params and this camera before the scene changed: the caller guarantees that prev_params holds
 * that render's spp, spp_offset, depths, integrator, t_min and exact_math (accel and the scheduling fields may differ: the film
 * never depends on them) and that the camera is the same.  Consecutive frames must use different spp_offsets (temporal
 * accumulation needs that anyway: equal samples add nothing); the re-trace then shares no sample with the current frame.
 * d_alpha: W*H floats, 4-byte aligned.  The strata's pixel list, their re-traced film and their records live in context-owned
 * buffers that grow on first use.  Asynchronous on the context's stream; needs a scene; the whole image only.
 * PT_ERR_INVALID_ARG: a null argument, a misaligned plane, band_count > 1, radius > 8, a scale that is negative or not finite,
 * alpha_min outside [0, 1], an image smaller than 2 x 2; the context is then untouched.                                     */
typedef struct {
    uint32_t radius;         /* the window: (2 radius + 1)^2 strata around the pixel's, at most 8   */
    float scale;             /* lambda = min(1, scale D / Nn); finite, >= 0                         */
} PtGradient;
void pt_default_gradient(PtGradient* out);
int pt_temporal_gradient_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* prev_params, uint32_t seed,
                                const float* d_prev_linear, const PtGradient* g, float alpha_min, float* d_alpha);
/* Debug: the strata of the last pt_temporal_gradient_device of a width x height image on this context, copied back (blocking):
 * out_xy SW*SH (x, y) pairs, out_film SW*SH*3 floats (the re-traced film), out_rec SW*SH (delta, N) pairs of doubles, stratum
 * by * SW + bx; any may be NULL.                                                                                            */
int pt_debug_gradient_strata(PtContext* ctx, uint32_t width, uint32_t height, uint32_t* out_xy, float* out_film, double* out_rec);
/* pt_denoise_temporal_motion_device with a per-pixel blend weight: d_alpha, width*height floats on the device, 4-byte aligned,
 * not NULL.  Rule 4 alone changes: alpha' = max(alpha_p, 1/n) with alpha_p = d_alpha[p] when that is finite and in [0, 1];
 * any other entry (NaN, +-inf, out of range: "no measurement") takes tp->alpha.  With every entry NaN it is bit-identical to
 * the motion entry, with a constant plane c to the motion entry called with tp->alpha = c.  The history layout is the same:
 * the three temporal entries may be mixed freely on one context.                                                           */
int pt_denoise_temporal_alpha_device(PtContext* ctx, const PtCamera* cam, const float* d_linear_rgb, const float* d_features,
                                     const int32_t* d_ids, const float* d_alpha, const PtDenoise* dn, const PtTemporal* tp,
                                     float* d_out_linear, uint8_t* d_out_rgba8);
/* One frame with HOST buffers (blocking), the counterpart of pt_render_denoised_motion: the render, the feature pass, the ids
 * pass, the alpha plane, pt_denoise_temporal_alpha_device; bit-identical to calling the parts.  The alpha plane is
 * pt_temporal_gradient_device's, with alpha_min = tp->alpha and seed = the number of frames this entry completed on the
 * context since its previous frame was last dropped, when the context holds a usable PREVIOUS FRAME; otherwise every entry is
 * NaN and the frame is bit-identical to pt_render_denoised_motion.  The context keeps every completed frame's noisy film on
 * the device (12 bytes per pixel) with its parameters and camera.  That frame is usable when the size is the same, the camera
 * is equal field by field and the temporal history is valid; pt_temporal_reset and pt_scene_upload drop it, pt_scene_update,
 * pt_scene_refit and pt_scene_rebuild keep it.  A moved camera thus drops the previous frame here; a host whose camera moves
 * calls pt_render_denoised_gradient_camera below, which keeps it.  out_alpha (width*height floats) and the outputs that may
 * be NULL there may be NULL.                                                                                                */
int pt_render_denoised_gradient(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                                const PtDenoise* dn, const PtTemporal* tp, const PtGradient* g, float* out_linear_rgb,
                                uint8_t* out_rgba8, float* out_noisy_linear, float* out_features, int32_t* out_ids,
                                float* out_alpha);

/* Temporal gradients under a MOVING CAMERA (additive to ABI 6).  A pixel-list render is bit-identical to the same
 * pixel of a full render for any camera, so the previous frame's samples re-traced in the current scene are a list render
 * through the PREVIOUS camera; and the temporal kernels already compute where a current pixel's first-hit point lay in the
 * previous image (rule 2 of PtTemporal).  The rule (pathtrace_amd/csrc/pt_gradient.h), cam and prev_cam of one size W x H:
 *   strata       as above, in the PREVIOUS frame's image: the gradient pixel of stratum (bx, by) is a pixel of that image,
 *                c_new its film through prev_cam with prev_params in the current scene, c_old d_prev_linear at that pixel
 *   lookup       pixel p = (x, y) of cam with depth d_p from d_features.  cam equal to prev_cam field by field: (xi, yi) =
 *                (x, y) for every pixel, misses included.  Otherwise d_alpha[p] = NaN ("no measurement") when d_p is not > 0
 *                or the reprojection of rule 2 fails; else xi = floor(x' + 0.5), yi = floor(y' + 0.5), and d_alpha[p] = NaN
 *                when (xi, yi) lies outside the image
 *   weight       d_alpha[p] = the per-pixel rule above around the stratum of (xi, yi)
 * The lookup uses the cameras alone, not the object motion maps: the re-trace runs in the current scene, so the stratum that
 * measured the world point a pixel sees is the one where that point projects through prev_cam in the current pose.  A NaN
 * entry is what pt_denoise_temporal_alpha_device reads as "take tp->alpha"; a pixel that falls outside the previous image is
 * fresh there anyway, and a point that was occluded in the previous view fails that kernel's tap gates.
 *
 * pt_temporal_gradient_camera_device: pt_temporal_gradient_device's arguments, checks, buffers and asynchrony, with prev_cam
 * (the camera d_prev_linear was rendered through) and d_features (the CURRENT frame's feature records of cam, 16-byte
 * aligned).  Additionally PT_ERR_INVALID_ARG for a NULL prev_cam or d_features, a misaligned d_features and a prev_cam whose
 * width or height differs from cam's; the context is then untouched.  With prev_cam equal to cam field by field d_alpha is
 * bit-identical to pt_temporal_gradient_device's.  pt_debug_gradient_strata reads its strata, xy in the previous image.    */
int pt_temporal_gradient_camera_device(PtContext* ctx, const PtCamera* cam, const PtCamera* prev_cam,
                                       const PtRenderParams* prev_params, uint32_t seed, const float* d_prev_linear,
                                       const float* d_features, const PtGradient* g, float alpha_min, float* d_alpha);
/* pt_render_denoised_gradient with one difference: the previous frame is usable when the size is the same and the temporal
 * history is valid -- the cameras need not be equal -- and the plane is pt_temporal_gradient_camera_device's with the previous
 * frame's camera.  Both entries keep the previous frame in the same context state and may be mixed freely on one context;
 * with an unmoved camera this one is bit-identical to pt_render_denoised_gradient.                                          */
int pt_render_denoised_gradient_camera(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                                       const PtDenoise* dn, const PtTemporal* tp, const PtGradient* g, float* out_linear_rgb,
                                       uint8_t* out_rgba8, float* out_noisy_linear, float* out_features, int32_t* out_ids,
                                       float* out_alpha);

/* Auto-exposure and tone mapping for display (additive to ABI 6).  Every entry above writes its RGBA8 plane with
 * the reference's transform (sqrt, clamp, `as u8`): what lies above 1 is white, and a dimmed light is a dark frame.  These
 * entries are the last stage of a frame on the device: an exposure E -- given, or metered from the film's luminance histogram
 * and adapted over frames in device memory --, a curve, a transfer.  The rule (pathtrace_amd/csrc/pt_tonemap.h), image W x H,
 * c the linear film, L(c) = (0.2126 r + 0.7152 g) + 0.0722 b in f32:
 *   histogram   258 uint32 words: [0, 256) bins, 8 per octave over [2^-16, 2^16), bin = (bits(L) >> 20) - (bits(2^-16) >> 20),
 *               L >= 2^16 in bin 255; [256] dark: L < 2^-16 (0, negatives, denormals); [257] invalid: NaN, +-inf.  Sum = W H.
 *   metering    f64.  N = the sum of the bins, lo = pct_lo N, hi = pct_hi N; bin k holds the ranks [B_k, B_k + n_k) and counts
 *               in_k = max(0, min(B_k + n_k, hi) - max(B_k, lo)) at its centre z_k = -16 + (k + 0.5) / 8;  m = sum in_k z_k /
 *               sum in_k (pct_lo == pct_hi: z_k of the first bin with n_k > 0 and B_k + n_k >= lo);
 *               target t = clamp(log2(key) - m, log2_min, log2_max); N == 0: t = the previous exposure, 0 without one
 *   adaptation  the context holds log2E on the device.  After pt_exposure_reset, at first use or when W or H changed:
 *               log2E = t; otherwise log2E += adapt (t - log2E).  E = (float)exp2(log2E).
 *   manual      mode = PT_EXPOSURE_MANUAL: E = (float)exp2(ev); no histogram, the state untouched
 *   curve       x = E c per channel, f32.  PT_CURVE_CLAMP y = x;  PT_CURVE_REINHARD Lx = L(x), y = x (1 + Lx / white^2) /
 *               (1 + Lx);  PT_CURVE_ACES x' = min(x, 2^60), y = x' (2.51 x' + 0.03) / (x' (2.43 x' + 0.59) + 0.14).
 *               A channel whose y is NaN is 0 on both planes.
 *   transfer    PT_TRANSFER_SQRT: sqrt in f64, clamp, `as u8` -- the steps of every render;  PT_TRANSFER_SRGB: the piecewise
 *               sRGB curve in f32 (0 for y <= 0, 1 for y >= 1), then clamp and `as u8`.  Alpha 255.
 * Manual mode with ev = 0, PT_CURVE_CLAMP and PT_TRANSFER_SQRT is the display transform of pt_render_device.
 * pt_default_tonemap: auto, ACES, sqrt transfer, key 0.18, percentiles 0.5 / 0.95, log2 range -8 .. 8, adapt 0.1, white 4. */
enum { PT_EXPOSURE_AUTO = 0, PT_EXPOSURE_MANUAL = 1 };
enum { PT_CURVE_CLAMP = 0, PT_CURVE_REINHARD = 1, PT_CURVE_ACES = 2 };
enum { PT_TRANSFER_SQRT = 0, PT_TRANSFER_SRGB = 1 };
typedef struct {
    uint32_t mode;           /* PT_EXPOSURE_*                                                        */
    uint32_t curve;          /* PT_CURVE_*                                                           */
    uint32_t transfer;       /* PT_TRANSFER_*                                                        */
    float ev;                /* manual mode: E = 2^ev; finite                                        */
    float key;               /* the luminance the metered part of the film is exposed to; finite, > 0 */
    float pct_lo, pct_hi;    /* the metered ranks, as fractions of the pixels: 0 <= lo <= hi <= 1     */
    float log2_min, log2_max; /* the range of the target, log2_min <= log2_max                        */
    float adapt;             /* the share of the way to the target a frame goes, in [0, 1]            */
    float white;             /* PT_CURVE_REINHARD: the luminance that maps to 1; finite, > 0          */
} PtTonemap;
void pt_default_tonemap(PtTonemap* out);
/* The histogram alone: d_linear_rgb (width*height*3 floats on the device, 4-byte aligned) -> d_hist258 (258 uint32 on the
 * device, 4-byte aligned; zeroed on the stream in front of the kernel).  Asynchronous on the context's stream; needs no scene.
 * PT_ERR_INVALID_ARG for a null argument, a misaligned plane or an image smaller than 2 x 2; the context is then untouched. */
int pt_film_histogram_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_linear_rgb, uint32_t* d_hist258);
/* One frame through the rule: d_linear_rgb -> d_out_rgba8 (width*height*4 bytes) and, when d_out_linear is not NULL, y (the
 * tone-mapped film in front of the transfer, width*height*3 floats).  d_out_linear may be d_linear_rgb (in place).  Asynchronous
 * on the context's stream (the caller's after pt_context_set_stream): the host never waits for the exposure, the metering
 * kernel leaves it in device memory and the curve kernel reads it there.  Needs no scene.  The context allocates its 258
 * histogram words and its state words at the first auto-mode call and nothing afterwards, so later calls can be captured
 * into a graph.  PT_ERR_INVALID_ARG, with the context untouched, for a null argument (d_out_linear excepted), a misaligned
 * plane, an image smaller than 2 x 2, an unknown mode, curve or transfer, an ev that is not finite, pct_lo or pct_hi outside
 * [0, 1] or pct_lo > pct_hi, a key or white that is not finite and > 0, adapt outside [0, 1], log2_min > log2_max.
 * pt_scene_upload and the other scene entries do not touch the exposure.                                                  */
int pt_tonemap_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_linear_rgb, const PtTonemap* tm,
                      float* d_out_linear, uint8_t* d_out_rgba8);
/* pt_tonemap_device with HOST planes (blocking): the film is staged in a context-owned device buffer and mapped there. */
int pt_tonemap_host(PtContext* ctx, uint32_t width, uint32_t height, const float* linear_rgb, const PtTonemap* tm,
                    float* out_linear, uint8_t* out_rgba8);
/* The next auto-mode frame takes its target as its exposure.  On the context's stream, in order with the frames around it. */
int pt_exposure_reset(PtContext* ctx);
/* Blocking: log2E of the context (0 when it has none) and, when hist258 is not NULL, the 258 words of the last auto-mode
 * frame's histogram (host memory; zeros before the first).                                                               */
int pt_exposure_get(PtContext* ctx, double* log2E, uint32_t* hist258);
/* Debug: pt_exposure_get with the device's own E (1 when there is none) and the valid word; any output may be NULL. */
int pt_debug_exposure_state(PtContext* ctx, double* log2E, float* E, uint32_t* valid, uint32_t* hist258);
/* Debug entries, host only (no GPU needed): the functions of pt_tonemap.h as the host compiler builds them.  The histogram
 * word of a luminance; the metering and adaptation of 258 words (fresh != 0: no usable previous exposure) -> the new log2E;
 * one pixel through curve and transfer under a given E -> y (3 floats) and its RGBA8 bytes.                              */
uint32_t pt_debug_tonemap_bin(float L);
double pt_debug_tonemap_meter(const uint32_t* hist258, const PtTonemap* tm, int fresh, double log2E_prev);
int pt_debug_tonemap_pixel(const PtTonemap* tm, float E, const float* rgb, float* out_y, uint8_t* out_rgba8);

/* Bloom (additive to ABI 6): the stage in front of pt_tonemap_device.  The display transform works pixel by pixel, so an
 * emitter 20 times over white ends as the same 255 as one 1.1 times over; bloom spreads the part of the linear film above a threshold
 * over its neighbourhood before the curve, and the meter then sees the bloomed film, as a camera's would.  The rule
 * (pathtrace_amd/csrc/pt_bloom.h), all of it f32 with + - * /, comparisons and selects, so that host and device agree bit for bit;
 * film c of W x H pixels:
 *   plan        level 0 is ceil(W/2) x ceil(H/2), level i is ceil(w/2) x ceil(h/2) of level i - 1 and exists while i < levels and
 *               level i - 1 is larger than 1 x 1; n levels
 *   bright      L = L(c), the tone mapper's luminance.  L or a channel NaN or +-inf, or L <= 0: b = 0.  Else d = L - T,
 *               q = min(max(d + k, 0), 2 k), soft = k > 0 ? q q / (4 k) : 0, g = min(max(max(soft, d), 0), clamp), b = max(c, 0) (g / L)
 *   reduce      film under the bright pass -> level 0, level i -> level i + 1: separable, horizontal first, weights 1/8, 3/8, 3/8, 1/8
 *               on the source indices 2 x - 1 .. 2 x + 2 clamped to the plane, summed left to right
 *   expand      up(P): separable, horizontal first; destination j takes 3/4 P[j >> 1] + 1/4 of its neighbour on the side j lies
 *               (j even: the one before, j odd: the one after), indices clamped
 *   collect     U_(n-1) = D_(n-1);  U_i = (1 - s) D_i + s up(U_(i+1))
 *   combine     a = intensity up(U_0);  out = a == 0 ? c : c + a per channel: a pixel without a bloom term is copied bit for bit,
 *               and a non-finite pixel stays what it was without touching its neighbours
 * Only pt_display_device applies bloom to an RGBA8 plane; the RGBA8 planes of the render entries carry none, and a multi-GPU render
 * has no bloom form (the caller can run these entries on the gathered film, on device 0).
 * PT_ERR_INVALID_ARG, before the context is looked at: a null argument, a plane that is not 4-byte aligned, an image smaller than
 * 2 x 2 or of more than 2^30 pixels, levels outside 1 .. 8, a field outside the range its comment gives (NaN included).
 * pt_default_bloom: 6 levels, threshold 1, knee 0.5, clamp +inf, scatter 0.7, intensity 0.05.                                    */
typedef struct {
    uint32_t levels;         /* pyramid levels asked for, 1 .. 8                                   */
    float threshold;         /* T: luminance where bloom starts; finite, >= 0                      */
    float knee;              /* k: half-width of the soft transition around T; finite, >= 0        */
    float clamp;             /* cap on a pixel's bright-pass luminance; > 0, +inf allowed          */
    float scatter;           /* s in [0, 1]: share each level takes from the coarser one           */
    float intensity;         /* finite, >= 0: weight of the bloom term added to the film           */
} PtBloom;
void pt_default_bloom(PtBloom* out);
/* d_linear_rgb (width*height*3 floats on the device) -> d_out_linear (the same size; may be d_linear_rgb: in place).  Asynchronous
 * on the context's stream (the caller's after pt_context_set_stream); needs no scene.  The context owns the pyramid buffer, which
 * grows at the first call of an image size and never afterwards.  PT_ERR_UNSUPPORTED for an image that needs 2^24 tiles or more
 * (two or three pixels wide or high and of some 2^29 pixels).                                                                       */
int pt_bloom_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_linear_rgb, const PtBloom* bloom, float* d_out_linear);
/* The rule header on the CPU, on host planes.  Needs no GPU and no context; out_linear may be linear_rgb.                          */
int pt_bloom_host(uint32_t width, uint32_t height, const float* linear_rgb, const PtBloom* bloom, float* out_linear);
/* pt_bloom_device into a context-owned full-size plane, then pt_tonemap_device from that plane, bit for bit -- the metering and the
 * exposure state included.  bloom NULL: pt_tonemap_device.  Refuses what either stage refuses, before anything is enqueued.         */
int pt_display_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_linear_rgb, const PtBloom* bloom,
                      const PtTonemap* tm, float* d_out_linear, uint8_t* d_out_rgba8);
/* pt_display_device with HOST planes (blocking), staged like pt_tonemap_host; out_linear may be NULL.                              */
int pt_display_host(PtContext* ctx, uint32_t width, uint32_t height, const float* linear_rgb, const PtBloom* bloom, const PtTonemap* tm,
                    float* out_linear, uint8_t* out_rgba8);
/* Debug entries, host only.  The plan of (width, height, levels): out_wh receives (w, h) of every level (room for 16 words), n_levels
 * their number, first_tail_level the first level of at most 32 x 32 texels (w <= 32 and h <= 32; n_levels when there is none), from
 * which on one workgroup runs the rest of the pyramid in LDS.  One pixel through the bright pass: rgb (3 floats) -> out_b (3).       */
int pt_debug_bloom_plan(uint32_t width, uint32_t height, uint32_t levels, uint32_t* out_wh, uint32_t* n_levels, uint32_t* first_tail_level);
int pt_debug_bloom_bright(const PtBloom* bloom, const float* rgb, float* out_b);
/* Debug: enable = 0 makes the context run every level with the per-level kernels instead of the one-workgroup tail kernel (same
 * bits, more launches); anything else restores the default.                                                                        */
int pt_debug_bloom_tail(PtContext* ctx, int enable);

/* Feature-guided upsampling (additive to ABI 6): paths traced on a w x h grid and first-hit features at the full
 * W x H reconstruct a full-size film -- joint bilateral upsampling in the denoiser's demodulated space.  The low camera is
 * the full camera with width / height replaced (the cached frustum fields of PtCamera do not depend on the pixel count).
 * The rule (pathtrace_amd/csrc/pt_upsample.h), for the full-size pixel p = (x, y) with record {albedo A, emitter, normal n,
 * depth d}; c, f the low film and its records, film row y top-down:
 *   position    f64, multiply then divide: X = ((x + 0.5)(w - 1)) / (W - 1) - 0.5,  Y = h - 0.5 - ((H - 1 - y + 0.5)(h - 1)) /
 *               (H - 1); X0 = floor(X), fx = X - X0, likewise Y0, fy.  w = W, h = H: X = x, Y = y exactly.
 *   taps        the low pixels (Y0, X0), (Y0, X0 + 1), (Y0 + 1, X0), (Y0 + 1, X0 + 1) in this order; bilinear weights b_q formed
 *               in f64, rounded to f32; a tap outside the low image or with b_q = 0 is skipped
 *   class       miss (depth = 0), else emitter (emitter > 0), else surface.  A tap of another class than p's: w_q = 0.  Same
 *               class: miss, emitter w_q = b_q; surface w_q = b_q max(0, n . n_q)^sigma_n exp(-|d - d_q| / (sigma_d r max(d, 1e-3)
 *               + 1e-10)), r = max((W - 1) / (w - 1), (H - 1) / (h - 1)) in f32, w_q = 0 when n . n_q is <= 0 or NaN
 *   anchor      a = the tap with the largest b_q among the taps of p's class, without one among all taps not skipped; ties
 *               go to the first in the order above
 *   value       u_q = c_q / max(albedo_q, 1e-3) per channel (f32), u = u_a + sum w_q (u_q - u_a) / (sum w_q + 1e-6) (these sums in
 *               f64, u rounded to f32): no threshold, continuous in the weights, the anchor when nothing agrees with p;
 *               c' = u max(A, 1e-3) (f32); the RGBA8 plane is c' through the sqrt / clamp / `as u8` steps of every render
 * With w = W, h = H and the same records on both sides the output is pt_denoise_device's with iterations = 0, bit for bit.
 * pt_default_upsample: the denoiser's sigma_n 128 and sigma_d 0.025.                                                       */
typedef struct {
    float sigma_n;           /* exponent of the normal weight; finite, >= 0                          */
    float sigma_d;           /* depth tolerance per low pixel, relative to the depth; finite, >= 0   */
} PtUpsample;
void pt_default_upsample(PtUpsample* out);
/* d_lo_linear (lo_width*lo_height*3 floats), d_lo_features (lo_width*lo_height*8 floats, 16-byte aligned) and d_features
 * (width*height*8 floats, 16-byte aligned) -> d_out_linear (width*height*3 floats) and, when not NULL, d_out_rgba8
 * (width*height*4 bytes); all on the device.  Asynchronous on the context's stream (the caller's after
 * pt_context_set_stream); needs no scene, allocates nothing and touches no context state: the temporal history, the exposure
 * and the adaptive sums stay as they are.  PT_ERR_INVALID_ARG, before the context is looked at, for a null pointer
 * (d_out_rgba8 excepted), a misaligned plane (16 bytes for the records, 4 for the rest), a dimension below 2, a low size above
 * the full size, an output that is one of the inputs, a sigma that is negative or not finite.                              */
int pt_upsample_device(PtContext* ctx, uint32_t lo_width, uint32_t lo_height, const float* d_lo_linear, const float* d_lo_features,
                       uint32_t width, uint32_t height, const float* d_features, const PtUpsample* up, float* d_out_linear,
                       uint8_t* d_out_rgba8);
/* The same planes in HOST memory, the same checks: the rule header run on the CPU.  Needs no device and no context. */
int pt_upsample_host(uint32_t lo_width, uint32_t lo_height, const float* lo_linear, const float* lo_features, uint32_t width,
                     uint32_t height, const float* features, const PtUpsample* up, float* out_linear, uint8_t* out_rgba8);
/* One frame (host buffers, blocking, the whole image): the render of params through the low camera, the low features,
 * pt_denoise_device on the low film, the full-size features, pt_upsample_device -- bit-identical to these five entries called
 * in this order.  Both feature passes take min(feature_samples, params->spp) samples from params->spp_offset.  out_linear_rgb
 * and out_rgba8 are the full-size film (width*height of cam); out_lo_linear the denoised low film (lo_width*lo_height*3
 * floats), out_features the full-size records; every output but out_linear_rgb may be NULL.                              */
int pt_render_denoised_upsampled(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t lo_width,
                                 uint32_t lo_height, uint32_t feature_samples, const PtDenoise* dn, const PtUpsample* up,
                                 float* out_linear_rgb, uint8_t* out_rgba8, float* out_lo_linear, float* out_features);

/* Thin-lens camera (additive to ABI 6): depth of field.  The lens travels beside PtCamera; the rule
 * (pathtrace_amd/csrc/pt_lens.h):
 *   host, f64   C = lower_left + horizontal/2 + vertical/2 - origin, D = |C|, U = horizontal/|horizontal|, V = vertical/|vertical|;
 *               inv_phi = D / focus_distance, Lu = (aperture/2) U, Lv = (aperture/2) V; the device receives them rounded to f32
 *   per sample  in the render's arithmetic, from the ONE Philox block the pinhole ray draws for (x, y, sample): words 0, 1 the
 *               pixel jitter as ever, words 2, 3 (spare until now) the lens point; `dir` the pinhole ray's direction before it
 *               is normalised.  (a, b) = 2 u01(w2) - 1, 2 u01(w3) - 1 -> (dx, dy) on the unit disc by Shirley's concentric map;
 *               l = dx Lu + dy Lv;  o' = origin + l;  d' = normalize(dir - l inv_phi)
 * aperture 0: l = 0 and every entry below is its pinhole entry bit for bit.  aperture > 0: all rays of a jittered screen point
 * meet at origin + dir / inv_phi, on the plane at focus_distance.  The path kernels do not know the lens: the rays reach them as
 * given paths (what pt_ray_color does), each traced with key (x, y) and its own sample index.
 * PT_ERR_INVALID_ARG, and the context untouched, for: a null argument, an aperture that is negative or not finite, a
 * focus_distance that is not finite or not > 0, a degenerate camera (D or an axis of length 0 or not finite), and everything the
 * pinhole entry refuses.
 * The temporal and motion entries have no lens form: their reprojection assumes a pinhole.                                  */
typedef struct {
    double aperture;         /* lens diameter in world units; finite, >= 0; 0 = pinhole                                       */
    double focus_distance;   /* distance from the origin to the plane of focus, along the view axis; finite, > 0              */
} PtLens;
void pt_default_lens(PtLens* out);   /* aperture 0, focus_distance 1 */
/* pt_render_device through the lens (asynchronous on the context's stream): the film is the mean, through the ordinary resolve
 * (f64 sums in sample order), of the lens rays' colours for samples spp_offset .. spp_offset + spp - 1.  Row bands as in
 * pt_render_device; max_paths_in_flight cuts the job into sample batches and the film does not depend on them.  The context
 * owns the planes the rays are written to: they grow at first use.                                                          */
int pt_render_lens_device(PtContext* ctx, const PtCamera* cam, const PtLens* lens, const PtRenderParams* params,
                          float* d_linear_rgb, uint8_t* d_rgba8);
/* The same into host buffers (blocking), as pt_render_host. */
int pt_render_lens_host(PtContext* ctx, const PtCamera* cam, const PtLens* lens, const PtRenderParams* params,
                        float* out_linear_rgb, uint8_t* out_rgba8);
/* pt_render_features_device with lens rays: the same records, sums and checks. */
int pt_render_features_lens_device(PtContext* ctx, const PtCamera* cam, const PtLens* lens, const PtRenderParams* params,
                                   uint32_t n_samples, float* d_features);
/* pt_render_denoised through the lens (host buffers, blocking): bit-identical to pt_render_lens_device ->
 * pt_render_features_lens_device -> pt_denoise_device.                                                                      */
int pt_render_lens_denoised(PtContext* ctx, const PtCamera* cam, const PtLens* lens, const PtRenderParams* params,
                            uint32_t feature_samples, const PtDenoise* dn, float* out_linear_rgb, uint8_t* out_rgba8,
                            float* out_noisy_linear, float* out_features);
/* Debug: the lens rays of n (x, y, sample) triples (x, y the film position, top-down) as pt_debug_camera_rays gives the
 * pinhole rays: out8 = n * (o'3, d'3, dx, dy).  Host arrays, blocking; needs no scene.                                       */
int pt_debug_lens_rays(PtContext* ctx, const PtCamera* cam, const PtLens* lens, const uint32_t* xys, uint32_t n,
                       uint32_t exact_math, float* out8);
/* Debug, host only: out7 = Lu3, Lv3, inv_phi as the device receives them.  Needs no device. */
int pt_debug_lens_setup(const PtCamera* cam, const PtLens* lens, float* out7);

/* Projections and films from the caller's rays (additive to ABI 6).  The projection travels beside PtCamera; the
 * rule (pathtrace_amd/csrc/pt_projection.h):
 *   host, f64   C = lower_left + horizontal/2 + vertical/2 - origin, Wv = C/|C|, U = horizontal/|horizontal|,
 *               V = vertical/|vertical|, aspect = |vertical|/|horizontal|; the device receives them rounded to f32
 *   per sample  in the render's arithmetic, from the ONE Philox block the pinhole ray draws for (x, y, sample): words 0, 1 the
 *               pixel jitter as ever; u, v and `dir` by the pinhole ray's own statements; a = 2u - 1, b = 2v - 1
 *     PERSPECTIVE   o = origin, d = normalize(dir): the pinhole ray, and every entry below is its pinhole entry bit for bit
 *     ORTHOGRAPHIC  o = origin + (dir - C), d = Wv: the view window is |horizontal| x |vertical| at the camera plane
 *     FISHEYE       equidistant: bb = b aspect, rho = sqrt(a a + bb bb), theta = min(rho fov/720, 1/2) revolutions off the axis,
 *                   d = normalize(cos Wv + sin (a/rho) U + sin (bb/rho) V), d = Wv at rho = 0, o = origin.  No masking: the
 *                   corners see further, to at most 180 degrees off the axis
 *     EQUIRECT      longitude a/2 revolutions, latitude b/4: d = normalize(cos(lat) (sin(lon) U + cos(lon) Wv) + sin(lat) V),
 *                   o = origin.  Column 0 looks backwards on the left, the centre column along Wv, rows from +V (top) to -V
 * The path kernels do not know the projection: the rays reach them as given paths, as the lens rays do, each traced with key
 * (x, y) and its own sample index.
 * PT_ERR_INVALID_ARG, and the context untouched, for: a null argument, an unknown kind, a reserved word that is not 0, a fisheye
 * fov_degrees that is not finite or outside (0, 360], a degenerate camera (|C| or an axis of length 0 or not finite), and
 * everything the pinhole entry refuses.
 * Out of scope: the temporal, motion and gradient entries keep assuming a pinhole, and there is no lens, cascade, filtered,
 * adaptive, progressive or multi-GPU form of the projection render.                                                          */
enum { PT_PROJ_PERSPECTIVE = 0, PT_PROJ_ORTHOGRAPHIC = 1, PT_PROJ_FISHEYE = 2, PT_PROJ_EQUIRECT = 3 };
typedef struct {
    uint32_t kind;           /* PT_PROJ_*                                                                                     */
    uint32_t reserved;       /* 0                                                                                             */
    double fov_degrees;      /* FISHEYE only: the angle the image's width spans; finite, in (0, 360]                          */
} PtProjection;
void pt_default_projection(PtProjection* out);   /* perspective, fov 180 */
/* pt_render_device under the projection (asynchronous on the context's stream), with the film, row bands, batching by
 * max_paths_in_flight and plane ownership of pt_render_lens_device.                                                          */
int pt_render_projection_device(PtContext* ctx, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* params,
                                float* d_linear_rgb, uint8_t* d_rgba8);
/* The same into host buffers (blocking), as pt_render_host. */
int pt_render_projection_host(PtContext* ctx, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* params,
                              float* out_linear_rgb, uint8_t* out_rgba8);
/* pt_render_features_device with projection rays: the same records, sums and checks. */
int pt_render_features_projection_device(PtContext* ctx, const PtCamera* cam, const PtProjection* proj,
                                         const PtRenderParams* params, uint32_t n_samples, float* d_features);
/* pt_render_denoised under the projection (host buffers, blocking): bit-identical to pt_render_projection_device ->
 * pt_render_features_projection_device -> pt_denoise_device.                                                                 */
int pt_render_projection_denoised(PtContext* ctx, const PtCamera* cam, const PtProjection* proj, const PtRenderParams* params,
                                  uint32_t feature_samples, const PtDenoise* dn, float* out_linear_rgb, uint8_t* out_rgba8,
                                  float* out_noisy_linear, float* out_features);
/* A film from the caller's own rays (asynchronous on the context's stream).  d_rays6: device float[spp][tile rows][width][6] =
 * origin3, direction3, sample-major with the pixel fastest, 8-byte aligned; the planes hold the tile's rows only (row bands as
 * in pt_render_device).  d_weights3: device float[spp][tile rows][width][3], the initial throughput of every ray, or NULL = 1.
 * The ray of plane s at (row, x) is traced as sample spp_offset + s of that pixel, key (x, image row); the film is the mean
 * through the ordinary resolve.  Directions are TAKEN AS GIVEN and not normalised, so rays this library produced come back bit
 * for bit; a direction that is not a unit vector gives what the path kernels make of it.  max_paths_in_flight cuts the job
 * into sample batches and the film does not depend on them.  The caller keeps the planes alive until the stream has passed
 * the call.  width and tile rows < 65536.  PT_ERR_INVALID_ARG, and the context untouched, for a NULL d_rays6 or context, a
 * misaligned buffer, spp = 0, and everything the pinhole entry refuses.                                                      */
int pt_render_rays_device(PtContext* ctx, uint32_t width, uint32_t height, const PtRenderParams* params, const float* d_rays6,
                          const float* d_weights3, float* d_linear_rgb, uint8_t* d_rgba8);
/* Debug: the projection's rays of n (x, y, sample) triples (x, y the film position, top-down) on the device:
 * out8 = n * (o3, d3, a, b).  Host arrays, blocking; needs no scene.                                                         */
int pt_debug_projection_rays(PtContext* ctx, const PtCamera* cam, const PtProjection* proj, const uint32_t* xys, uint32_t n,
                             uint32_t exact_math, float* out8);
/* Host only: out11 = U3, V3, Wv3, aspect, fov_degrees/720 (0 unless FISHEYE) as the device receives them.  Needs no device. */
int pt_projection_setup_host(const PtCamera* cam, const PtProjection* proj, float* out11);
/* Host only: the rule on the CPU in the render's exact arithmetic, out8 as pt_debug_projection_rays with exact_math = 1, bit
 * for bit.  Needs no device.                                                                                                 */
int pt_projection_rays_host(const PtCamera* cam, const PtProjection* proj, const uint32_t* xys, uint32_t n, float* out8);

/* Light baking (additive to ABI 6): the light that arrives at surface points (lightmaps) and at points in space
 * (irradiance probes, as spherical harmonics).  The path kernels do not know: the rays reach them as given paths, as the lens
 * and projection rays do, with the keys, film slots and resolve of a plain render.  The rule (pathtrace_amd/csrc/pt_bake.h):
 *   texel ray   one record per texel, float[H][W][6] = point3, normal3.  Sample s of texel (x, y) takes words 0 and 1 of the ONE
 *               Philox block the pinhole ray draws for the key (x, y, s): r1 = u01(w0), r2 = u01(w1); nn = normalize(normal) in
 *               f32; d = the cosine-weighted direction about nn of the materials' own sampler; o = point as it is (t_min keeps
 *               the ray off its surface, as for every continuation ray); throughput 1.  The film is the cosine-weighted mean
 *               radiance E / pi: times a Lambert albedo it is the outgoing radiance.
 *   empty texel one of its six numbers is not finite, or the f32 square of its normal's length is below 1e-36 or not finite.
 *               Its outputs are +0.0 and the RGBA8 pixel of a black film pixel, whatever the scene; the render's sample count
 *               stays W H spp.
 *   probe ray   direction r of R, the same for every probe and sample: z = 1 - (2r + 1) / R; phase = the top 24 bits of
 *               (r * 0x9E3779B9) mod 2^32, in revolutions; d = (sqrt(1 - z^2) cos, sqrt(1 - z^2) sin, z); o = the probe's
 *               position; solid-angle weight 4 pi / R.  spp > 1 repeats the direction with independent continuations.
 *   SH          real spherical harmonics through l = 2, coefficient k = l (l + 1) + m, constants 0.282095, 0.488603, 1.092548,
 *               0.315392, 0.546274: sh[p][k][c] = (4 pi / R) sum_r radiance[p][r][c] Y_k(d_r), in f64 in a fixed order (lane j
 *               of 64 sums r = j, j + 64, ..., then a pairwise tree), d_r the rule's direction in exact arithmetic.  Host and
 *               device agree bit for bit.
 *   irradiance  E(n) = sum A_l sh_lm Y_lm(n), A = (pi, 2 pi / 3, pi / 4).
 * Under PT_INTEGRATOR_MIS the path kernels carry the reference's MIS weights, which do not sum to 1; a baked
 * texel's first bounce is plain cosine sampling with emitters counted in full, so a bake differs from what a camera sees of the
 * same Lambert point by that documented bias.  Under PT_INTEGRATOR_BRDF_ONLY the two agree in expectation.
 * Every entry checks everything before its first launch.  PT_ERR_INVALID_ARG, with a message and the context untouched, for: a
 * null or misaligned plane, a zero size, rays_per_probe = 0, a size of 65536 or more, band_count > 1, and everything the pinhole
 * entry refuses.  Not there: a lens, filter, cascade, adaptive, progressive or multi-GPU form, and row bands.                 */
enum { PT_BAKE_TEXELS = 0, PT_BAKE_PROBES = 1 };
/* A lightmap (asynchronous on the context's stream).  d_texels6: device float[height][width][6], 8-byte aligned.
 * d_linear_rgb: device float[height][width][3]; d_rgba8: device uint8[height][width][4], 4-byte aligned, or NULL.
 * width, height in [1, 65535]; max_paths_in_flight cuts the job into sample batches and the film does not depend on them.     */
int pt_bake_lightmap_device(PtContext* ctx, uint32_t width, uint32_t height, const float* d_texels6, const PtRenderParams* params,
                            float* d_linear_rgb, uint8_t* d_rgba8);
/* The same from and into host buffers (blocking). */
int pt_bake_lightmap_host(PtContext* ctx, uint32_t width, uint32_t height, const float* texels6, const PtRenderParams* params,
                          float* out_linear_rgb, uint8_t* out_rgba8);
/* Probes (asynchronous on the context's stream).  d_positions3: device float[n_probes][3].  d_radiance: device
 * float[n_probes][rays_per_probe][3], the film -- a probe per row, a direction per column --, the mean over spp.  d_sh27: device
 * float[n_probes][9][3], or NULL.  n_probes, rays_per_probe in [1, 65535].                                                    */
int pt_bake_probes_device(PtContext* ctx, const float* d_positions3, uint32_t n_probes, uint32_t rays_per_probe,
                          const PtRenderParams* params, float* d_radiance, float* d_sh27);
/* The same from and into host buffers (blocking); out_sh27 may be NULL. */
int pt_bake_probes_host(PtContext* ctx, const float* positions3, uint32_t n_probes, uint32_t rays_per_probe,
                        const PtRenderParams* params, float* out_radiance, float* out_sh27);
/* The SH projection of radiance planes the caller holds on the device (asynchronous on the context's stream); needs no scene. */
int pt_sh_project_device(PtContext* ctx, uint32_t n_probes, uint32_t rays_per_probe, const float* d_radiance, float* d_sh27);
/* Host only: the same on the CPU, bit for bit.  Needs no device. */
int pt_sh_project_host(uint32_t n_probes, uint32_t rays_per_probe, const float* radiance, float* sh27);
/* Host only: the irradiance E(n) of ONE probe's coefficients sh27 = float[9][3] at n normals (normalised in f64 first; a normal
 * of length 0 gives 0): out_rgb = float[n][3].  Needs no device.                                                              */
int pt_sh_irradiance_host(const float* sh27, const float* normals3, uint32_t n, float* out_rgb);
/* Debug: the bake's rays of n (x, y, sample) triples on the device: out6 = n * (o3, d3).  kind PT_BAKE_TEXELS: width x height
 * texels, data = host float[height][width][6]; PT_BAKE_PROBES: width = rays_per_probe, height = n_probes, data = host
 * float[n_probes][3], x the direction, y the probe.  Host arrays, blocking; needs no scene.  x >= width or y >= height is
 * refused.                                                                                                                  */
int pt_debug_bake_rays(PtContext* ctx, uint32_t kind, uint32_t width, uint32_t height, const float* data, const uint32_t* xys,
                       uint32_t n, uint32_t exact_math, float* out6);
/* Host only: the rule on the CPU in the render's exact arithmetic, out6 as pt_debug_bake_rays with exact_math = 1, bit for bit.
 * Needs no device.                                                                                                           */
int pt_bake_rays_host(uint32_t kind, uint32_t width, uint32_t height, const float* data, const uint32_t* xys, uint32_t n,
                      float* out6);

/* Irradiance volume (additive to ABI 6): a regular grid of baked SH probes, sampled at every visible point -- diffuse
 * global illumination for the price of a first-hit pass.  pt_probe_grid_bake_device bakes the grid, pt_probe_shade_device turns
 * first-hit features (pt_render_features_device) and the baked coefficients into a film, pt_render_probe_lit_device does the
 * feature pass and the shading in one call.  No path kernel knows.  The rule (pathtrace_amd/csrc/pt_probe_grid.h), f64 with
 * + - * /, square root, comparisons and selects in a fixed order, so that the host and the device agree bit for bit:
 *   grid        probe (ix, iy, iz) has index (iz ny + iy) nx + ix and the position origin_a + i_a spacing_a, formed in f64 and
 *               rounded to f32 once.  Valid: no count 0, origin and spacing finite, spacing > 0 on every axis with more than one
 *               probe, at most 65535 probes.
 *   unlit       a pixel whose depth is not > 0 (a miss, NaN), whose emitter flag is > 0, whose normal, depth or albedo is not
 *               finite, whose normal has the f64 length 0, or whose point is not finite (every pixel when width or height is 1):
 *               it takes the fallback pixel bit for bit, +0.0 without a fallback plane, and reads no probe.
 *   point       s = (x + 0.5) / (W - 1), t = (H - 1 - y + 0.5) / (H - 1), D = lower_left + s horizontal + t vertical - origin,
 *               P = origin + depth (D (1 / |D|)): the temporal denoiser's reconstruction.  nn = n / |n|; Q = P + normal_bias nn.
 *   cell        per axis with more than one probe g = (Q_a - origin_a) / spacing_a, clamped to [0, count - 1] (NaN: unlit),
 *               i = min(floor(g), count - 2), f = g - i; an axis with one probe has i = 0, f = 0 and one corner for both.
 *   weights     corner j = 0..7 (bit 0 x, bit 1 y, bit 2 z): (wx wy) wz, each f or 1 - f.  PT_PROBE_WEIGHT_FACING multiplies by
 *               ((c + 1) / 2)^2 + 0.2 with c = (v . nn) / |v|, v = the corner's f32 position - P, c = 1 when |v| = 0: the backface
 *               weight of Majercik et al. 2019.  Its visibility term is not in these two weights -- with them light leaks through
 *               thin walls; the pt_probe_*_visibility entries below add it.
 *   blend       every coefficient C = C_0 + (sum_{j=1..7} w_j (C_j - C_0)) / (sum_j w_j), j ascending from 0.0: a constant field
 *               comes out exactly
 *   shade       E_c = sum_k A_l C[k][c] Y_k(nn) in pt_sh_irradiance_host's order; a negative E_c becomes 0, NaN stays;
 *               out_c = (float)((max(albedo_c, 0) E_c) / pi); the RGBA8 word through the sqrt, clamp and `as u8` of every render.
 * A Mirror surface is shaded as a diffuse one of its colour.  Every entry checks everything before its first launch.
 * PT_ERR_INVALID_ARG, with a message and the context untouched, for: a null or misaligned plane (features 16 bytes, the others
 * 4), an invalid grid, weight > 1, a normal_bias that is not finite, a zero size, band_count > 1, and everything the feature and
 * probe-bake entries refuse.                                                                                                   */
enum { PT_PROBE_WEIGHT_TRILINEAR = 0, PT_PROBE_WEIGHT_FACING = 1 };
typedef struct {
    double origin[3];        /* the position of probe (0, 0, 0); finite                         */
    double spacing[3];       /* between neighbours; finite, > 0 on an axis with more than one probe */
    uint32_t counts[3];      /* nx, ny, nz >= 1; nx ny nz <= 65535                              */
    uint32_t reserved;
} PtProbeGrid;
typedef struct {
    float normal_bias;       /* the lookup point is moved this far along the normal; finite    */
    uint32_t weight;         /* PT_PROBE_WEIGHT_*                                              */
} PtProbeShade;
/* normal_bias 0, PT_PROBE_WEIGHT_TRILINEAR */
void pt_default_probe_shade(PtProbeShade* out);
/* Host only: nx ny nz, or 0 for an invalid (or null) grid. */
uint32_t pt_probe_grid_count(const PtProbeGrid* grid);
/* Host only: the positions, float[count][3], as pt_bake_probes_* takes them.  Needs no device. */
int pt_probe_grid_positions_host(const PtProbeGrid* grid, float* out_positions3);
/* Bakes the grid (asynchronous on the context's stream): the positions are written on the device into a context-owned plane, then
 * pt_bake_probes_device runs with a context-owned radiance plane.  d_sh27: device float[count][9][3].  Bit-identical to
 * pt_bake_probes_device on the positions of pt_probe_grid_positions_host.                                                    */
int pt_probe_grid_bake_device(PtContext* ctx, const PtProbeGrid* grid, uint32_t rays_per_probe, const PtRenderParams* params,
                              float* d_sh27);
/* The shading pass (asynchronous on the context's stream; needs no scene).  cam: the camera the features were rendered with.
 * d_features: device float[height][width][8], 16-byte aligned.  d_fallback_linear: device float[height][width][3] or NULL; it may be
 * d_out_linear itself (in place).  d_out_rgba8: device uint8[height][width][4], 4-byte aligned, or NULL.                        */
int pt_probe_shade_device(PtContext* ctx, const PtCamera* cam, const PtProbeGrid* grid, const float* d_sh27, const float* d_features,
                          const float* d_fallback_linear, const PtProbeShade* shade, float* d_out_linear, uint8_t* d_out_rgba8);
/* Host only: the same rule on the CPU, host buffers (features 4-byte aligned), bit for bit.  Needs no device. */
int pt_probe_shade_host(const PtCamera* cam, const PtProbeGrid* grid, const float* sh27, const float* features,
                        const float* fallback_linear, const PtProbeShade* shade, float* out_linear, uint8_t* out_rgba8);
/* pt_render_features_device of feature_samples samples into a context-owned plane, then pt_probe_shade_device: bit-identical to
 * the two calls.  Asynchronous on the context's stream.                                                                     */
int pt_render_probe_lit_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                               const PtProbeGrid* grid, const float* d_sh27, const float* d_fallback_linear, const PtProbeShade* shade,
                               float* d_out_linear, uint8_t* d_out_rgba8);
/* The same from and into host buffers (blocking); fallback_linear and out_rgba8 may be NULL. */
int pt_render_probe_lit_host(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                             const PtProbeGrid* grid, const float* sh27, const float* fallback_linear, const PtProbeShade* shade,
                             float* out_linear, uint8_t* out_rgba8);
/* Debug: the grid's positions as the device writes them for pt_probe_grid_bake_device, copied to out_positions3 = host
 * float[count][3] (blocking; needs no scene).  The same bits as pt_probe_grid_positions_host.                               */
int pt_debug_probe_positions(PtContext* ctx, const PtProbeGrid* grid, float* out_positions3);

/* Irradiance volume, probe visibility (additive to ABI 6): every probe carries an octahedral map of the mean and the
 * mean square of the distance to the nearest surface in each direction, and a corner probe that the shaded point cannot see is
 * weighted down by a Chebyshev test -- the other half of the probe weight of Majercik et al. 2019, so that light no longer leaks
 * through walls between probes.  The rule (pathtrace_amd/csrc/pt_probe_vis.h), f64 as above, host and device bit for bit:
 *   map         T x T texels per probe, T = resolution in [2, 16]: moments float[count][T][T][2], texel (i, j) of probe p at
 *               ((p T + j) T + i) 2, 8-byte aligned.  Texel centre u = (i + 0.5) 2 / T - 1; direction oct_decode(u, v): z = 1 - |u|
 *               - |v|, (u, v, z) for z >= 0, else ((1 - |v|) sgn u, (1 - |u|) sgn v, z), normalised; oct_encode is its inverse
 *               (sgn 0 = +1).  No border is stored: a bilinear tap outside the map mirrors along the edge it crossed, (-1, j) ->
 *               (0, T-1-j), and a tap outside on both axes is the diagonally opposite corner texel.
 *   distances   float[n_probes][rays_per_probe]: the t of the first hit of probe ray r (the directions of pt_bake_probes_*), +inf
 *               for a miss.  Of PtRenderParams only t_min, accel and exact_math are read.
 *   moments     dist = t when 0 < t <= max_distance, else max_distance; per texel direction n: w = max(n . d_r, 0)^(2^sharpness_log2)
 *               with d_r the bake's direction in exact arithmetic; (m1, m2) = (sum w dist, sum w dist^2) / sum w, r ascending;
 *               (max_distance, max_distance^2) when sum w = 0.
 *   weight      the corner weight is tri F vis', with tri and F = ((c + 1) / 2)^2 + 0.2 as PT_PROBE_WEIGHT_FACING forms them,
 *               whatever PtProbeShade.weight says (it must still be a known value).  r = |Q - pos_j| from the biased point;
 *               (m1, m2) = the bilinear lookup at oct_encode((Q - pos_j) / r) in probe j's map; vis = 1 when r is 0 or not finite,
 *               a moment is not finite, or r <= m1; else vis = (var / (var + (r - m1)^2))^3, var = |m1^2 - m2|.  g = max(1e-6, F
 *               vis), g < 0.2: g = g^3 / 0.04.  The sum of the weights is > 0 always.  Maps with m1 >= r everywhere give
 *               PT_PROBE_WEIGHT_FACING's film bit for bit.
 * Everything else is pt_probe_shade_*'s.  Refused as there, and: resolution outside [2, 16], sharpness_log2 > 8, a max_distance
 * that is not finite or not > 0, a moments plane that is null or not 8-byte aligned, n_probes or rays_per_probe outside
 * [1, 65535].  Not there: probe relocation, a multi-GPU form (temporal hysteresis: the update entries below).                 */
typedef struct {
    uint32_t resolution;     /* T: texels per side of a probe's map, 2 .. 16                    */
    uint32_t sharpness_log2; /* k: the cosine lobe's exponent is 2^k, k <= 8                    */
    float max_distance;      /* distances are clamped to it; finite, > 0                        */
    uint32_t reserved;
} PtProbeVisibility;
/* resolution 8, sharpness_log2 5, max_distance = 1.5 x the diagonal of a grid cell over the axes with more than one probe (1 for
 * a NULL or invalid grid, or one without such an axis)                                                                     */
void pt_default_probe_visibility(const PtProbeGrid* grid, PtProbeVisibility* out);
/* The distances of n_probes x rays_per_probe probe rays (asynchronous on the context's stream): chunks of whole probes through the
 * feature pass's scratch; no path kernel.  d_positions3: device float[n_probes][3]; d_distances: device float[n_probes][rays_per_probe]. */
int pt_probe_distances_device(PtContext* ctx, const float* d_positions3, uint32_t n_probes, uint32_t rays_per_probe,
                              const PtRenderParams* params, float* d_distances);
/* The same from and into host buffers (blocking). */
int pt_probe_distances_host(PtContext* ctx, const float* positions3, uint32_t n_probes, uint32_t rays_per_probe,
                            const PtRenderParams* params, float* out_distances);
/* Distances -> moment maps (asynchronous on the context's stream; needs no scene). */
int pt_probe_moments_device(PtContext* ctx, const float* d_distances, uint32_t n_probes, uint32_t rays_per_probe,
                            const PtProbeVisibility* vis, float* d_moments);
/* Host only: the same rule on the CPU, bit for bit.  Needs no device. */
int pt_probe_moments_host(const float* distances, uint32_t n_probes, uint32_t rays_per_probe, const PtProbeVisibility* vis,
                          float* out_moments);
/* The maps of a grid: the positions into a context-owned plane, pt_probe_distances_device into a context-owned plane,
 * pt_probe_moments_device.  Bit-identical to the separate calls.  Asynchronous on the context's stream.                     */
int pt_probe_grid_visibility_device(PtContext* ctx, const PtProbeGrid* grid, uint32_t rays_per_probe, const PtRenderParams* params,
                                    const PtProbeVisibility* vis, float* d_moments);
/* pt_probe_shade_device with the visibility term; d_moments: the maps of the grid's probes at vis->resolution. */
int pt_probe_shade_visibility_device(PtContext* ctx, const PtCamera* cam, const PtProbeGrid* grid, const float* d_sh27,
                                     const float* d_moments, const PtProbeVisibility* vis, const float* d_features,
                                     const float* d_fallback_linear, const PtProbeShade* shade, float* d_out_linear, uint8_t* d_out_rgba8);
/* Host only: the same rule on the CPU, bit for bit.  Needs no device. */
int pt_probe_shade_visibility_host(const PtCamera* cam, const PtProbeGrid* grid, const float* sh27, const float* moments,
                                   const PtProbeVisibility* vis, const float* features, const float* fallback_linear,
                                   const PtProbeShade* shade, float* out_linear, uint8_t* out_rgba8);
/* pt_render_features_device, then pt_probe_shade_visibility_device: bit-identical to the two calls. */
int pt_render_probe_lit_visibility_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                                          const PtProbeGrid* grid, const float* d_sh27, const float* d_moments,
                                          const PtProbeVisibility* vis, const float* d_fallback_linear, const PtProbeShade* shade,
                                          float* d_out_linear, uint8_t* d_out_rgba8);
/* The same from and into host buffers (blocking); fallback_linear and out_rgba8 may be NULL. */
int pt_render_probe_lit_visibility_host(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, uint32_t feature_samples,
                                        const PtProbeGrid* grid, const float* sh27, const float* moments, const PtProbeVisibility* vis,
                                        const float* fallback_linear, const PtProbeShade* shade, float* out_linear, uint8_t* out_rgba8);

/* Irradiance volume, updates over frames (additive to ABI 6): the temporal half of Majercik et al. 2019.  After a
 * scene change the volume need not be baked again: each call re-traces a SUBSET of the probes with FEW rays along a freshly rotated
 * direction set and blends the result into the stored coefficients and moment maps with a per-probe hysteresis, so the quadrature
 * error of a small direction set averages away over frames.  The rule (pathtrace_amd/csrc/pt_probe_update.h), host and device bit
 * for bit:
 *   slots       a call updates the probes p = first + k stride < count, k = 0, 1, ...; slot k is probe first + k stride, n_upd =
 *               ceil((count - first) / stride).  The planes of a call's new data are slot-indexed: radiance float[n_upd][R][3],
 *               distances float[n_upd][R].
 *   ray         of slot k, direction r of R: the probe's position by the grid rule; d = the bake's direction r of R in the render's
 *               arithmetic; d'_a = fma(M[a][2], d_2, fma(M[a][1], d_1, M[a][0] d_0)) in f32, not normalised again; a rotation that is
 *               bit for bit the identity leaves d as it is (a select).  spp > 1 repeats a direction with independent continuations.
 *   new values  the SH projection of pt_sh_project_* and the moments of pt_probe_moments_* with the rotated direction in exact
 *               arithmetic in the place of the bake's.
 *   blend       per probe with age = d_age[p] (uint32): alpha = 1 when age = 0, else max(1 - hysteresis, 1 / (age + 1)) in f64 -- a
 *               plain running mean until the floor is reached.  Per SH coefficient and moment component: out = (float)(old + alpha
 *               (new - old)) in f64; out = new when age = 0 or old is not finite (old is never multiplied: a NaN of a plane that was
 *               never written does not survive); when new is not finite, out = old (age > 0) or +0.0 (age = 0).  age' = min(age + 1,
 *               65535).
 *   change gate change_threshold > 0 and age > 0: L0 = 0.2126 C[0][0] + 0.7152 C[0][1] + 0.0722 C[0][2] of the old and the new
 *               coefficients; both finite and |L0_new - L0_old| > change_threshold max(L0_old, L0_new, 0): alpha = max(alpha,
 *               change_alpha) for every coefficient and moment of that probe.
 *   untouched   probes that are not a slot of the call keep sh27, moments and age bit for bit.
 * Refused (PT_ERR_INVALID_ARG, before the first launch, the context untouched): what the probe-grid and visibility entries refuse of
 * the grid, the visibility struct and the planes; rays_per_probe outside [1, 65535]; stride = 0 or first >= count; a hysteresis
 * outside [0, 1) or not finite; a change_threshold that is negative or not finite; a change_alpha outside [0, 1] or not finite; a
 * rotation that is not finite, with max |M M^T - I| > 1e-5 or with a determinant <= 0; a NULL or misaligned d_age (4 bytes);
 * band_count > 1.  stride may be anything from 1 to 2^32 - 1 (a stride past the grid leaves the one slot `first`).  Not there:
 * probe relocation and classification, a multi-GPU form, lens, filter or cascade forms.                                          */
typedef struct {
    uint32_t rays_per_probe;   /* R, 1 .. 65535                                                                              */
    uint32_t first, stride;    /* this call updates probes p = first + k stride < P, k = 0, 1, ...; stride >= 1, first < P    */
    float    hysteresis;       /* h in [0, 1): the floor of the blend weight is 1 - h                                         */
    float    change_threshold; /* 0: off; else see "change gate"; finite, >= 0                                                */
    float    change_alpha;     /* in [0, 1]                                                                                   */
    float    rotation[9];      /* row-major M; finite, max |M M^T - I| <= 1e-5, det > 0                                       */
    uint32_t reserved;
} PtProbeUpdate;
/* Host only: the rotation of a frame, row-major.  Frame 0 is the identity exactly; otherwise u_i = (((frame c_i) mod 2^32) >> 8)
 * 2^-24 with c = 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, Shoemake's uniform quaternion (sqrt(1 - u0) sin 2 pi u1, sqrt(1 - u0) cos 2 pi
 * u1, sqrt(u0) sin 2 pi u2, sqrt(u0) cos 2 pi u2) = (x, y, z, w) in f64, the matrix in f64, rounded to f32 once.                  */
void pt_probe_rotation(uint32_t frame, float* out9);
/* Host only: rays_per_probe 64, first = frame % stride (stride 0 counts as 1), hysteresis 0.9375, the change gate off
 * (change_threshold 0, change_alpha 1), pt_probe_rotation(frame).                                                                */
void pt_default_probe_update(uint32_t frame, uint32_t stride, PtProbeUpdate* out);
/* Host only: the ray rule on the CPU in exact arithmetic.  xys = n x (direction r, slot, sample) inside the update's film of
 * rays_per_probe x n_upd; out6 = n x (o3, d3).                                                                                   */
int pt_probe_update_rays_host(const PtProbeGrid* grid, const PtProbeUpdate* upd, const uint32_t* xys, uint32_t n, float* out6);
/* The same rays from the device's debug-ray form (blocking; needs no scene).  In exact arithmetic the same bits. */
int pt_debug_probe_update_rays(PtContext* ctx, const PtProbeGrid* grid, const PtProbeUpdate* upd, const uint32_t* xys, uint32_t n,
                               uint32_t exact_math, float* out6);
/* The blend on planes the caller holds (k_probe_update; asynchronous on the context's stream; needs no scene).  d_radiance: device
 * float[n_upd][R][3]; vis may be NULL: no moments, and d_distances and d_moments are not read; else d_distances: device
 * float[n_upd][R], d_moments: device float[n_probes][T][T][2], 8-byte aligned.  d_sh27: device float[n_probes][9][3]; d_age: device
 * uint32[n_probes].  sh27, moments and age are updated in place.                                                                 */
int pt_probe_blend_device(PtContext* ctx, uint32_t n_probes, const PtProbeUpdate* upd, const PtProbeVisibility* vis,
                          const float* d_radiance, const float* d_distances, float* d_sh27, float* d_moments, uint32_t* d_age);
/* Host only: the same rule on the CPU, bit for bit, in place on host planes.  Needs no device. */
int pt_probe_blend_host(uint32_t n_probes, const PtProbeUpdate* upd, const PtProbeVisibility* vis, const float* radiance,
                        const float* distances, float* sh27, float* moments, uint32_t* age);
/* The whole update of a grid (asynchronous on the context's stream): the slots' rays through the path kernels into a context-owned
 * radiance plane (the fifth user of the injected-path driver), with vis their first-hit distances into a context-owned plane, then
 * pt_probe_blend_device.  Bit-identical to tracing and then blending.  params->spp_offset is the caller's means to draw fresh
 * continuations per frame.  vis may be NULL (d_moments is then not read).                                                         */
int pt_probe_grid_update_device(PtContext* ctx, const PtProbeGrid* grid, const PtRenderParams* params, const PtProbeVisibility* vis,
                                const PtProbeUpdate* upd, float* d_sh27, float* d_moments, uint32_t* d_age);
/* The same from and into host planes (blocking): sh27 float[count][9][3], moments float[count][T][T][2] (not read when vis is NULL)
 * and age uint32[count] go through the context's staging and come back updated; the same bits as the device entry.            */
int pt_probe_grid_update_host(PtContext* ctx, const PtProbeGrid* grid, const PtRenderParams* params, const PtProbeVisibility* vis,
                              const PtProbeUpdate* upd, float* sh27, float* moments, uint32_t* age);

/* Brightness cascade (additive to ABI 6): a firefly-robust film.  The samples of a render are averaged into the film
 * by an estimator that knows which of them are outliers -- the re-weighting of Zirr, Hanika and Dachsbacher (2018): every sample
 * is split between two layers of a per-pixel cascade by its luminance, and a layer keeps its energy in full only where enough
 * samples of that brightness landed in the pixel or its 3 x 3 neighbourhood.  The estimator is consistent: with more samples a
 * legitimate rare event reaches the count and is kept.  No path kernel knows the cascade: k_resolve_cascade stands in for the
 * ordinary resolve, k_cascade_reweight follows it.  The rule (pathtrace_amd/csrc/pt_cascade.h), all of it f64 with + - * /,
 * comparisons and selects only, so that the host and the device agree bit for bit:
 *   levels      B_0 = start, B_{j+1} = B_j base, K = layers of them (formed on the host by repeated multiplication)
 *   split       per sample v (f32), L = 0.2126 r + 0.7152 g + 0.0722 b in f64: j = the largest index in [0, K-2] with B_j <= L,
 *               0 when there is none (L < B_0, NaN).  !(L > B_j): w_lo = 1, w_hi = 0 (NaN, negatives, L <= B_0); else L < B_{j+1}:
 *               q = B_j / B_{j+1}, w_lo = (B_j / L - q) / (1 - q), w_hi = 1 - w_lo; else (L >= B_{K-1}, +inf) w_lo = 0, w_hi = 1.
 *               S_j += w_lo v and S_{j+1} += w_hi v per channel, each only when its weight is not exactly 0 (a select, not a
 *               multiplication by zero: an infinite sample puts no NaN into the lower layer); beside them the plain sums P += v,
 *               exactly as the ordinary resolve forms them.  Samples in sample order; the sums carry over sample batches.
 *   count       lum_j = 0.2126 S_j.r + 0.7152 S_j.g + 0.0722 S_j.b;  T_j = lum_{j-1} + lum_j + lum_{j+1} added left to right, an
 *               absent layer 0;  cnt_j = T_j / B_j
 *   re-weight   wide_j(p) = the sum of cnt_j over the in-image taps of the 3 x 3 block around p, row-major from 0, divided by the
 *               number of those taps;  r = cnt_j(p) > wide_j(p) ? cnt_j(p) : wide_j(p) (NaN when either is);  w_j(p) = 1 when
 *               j = 0, kappa = 0, r is NaN or r >= kappa, else r / kappa
 *   film        m = (sum over j ascending, from 0, of w_j(p) S_j(p)) / n per channel with n the samples per pixel; the linear
 *               plane is (float)m, the RGBA8 plane m through the sqrt, clamp and `as u8` steps of every render (which start from
 *               the f64 mean); the plain film is P / n, bit-identical to pt_render_device's
 * Whole image only (band_count = 1): the re-weighting reads neighbours.  params->exact_math changes the path kernels only; the
 * cascade kernels have no f32 arithmetic.  The lens, adaptive, progressive and multi-GPU renders have no cascade form, and the
 * layers are not fed to the denoiser: the cascade film is an ordinary linear film and pt_denoise_device takes it as it is.
 * PT_ERR_INVALID_ARG, with the context untouched, for: a null required argument, layers outside [2, 8], a start that is not
 * finite and > 0, a base that is not finite and >= 2, a kappa that is not finite and >= 0, a level table that overflows, an
 * image smaller than 2 x 2, band_count > 1, n = 0, a plane that is not 4-byte aligned, an output that shares memory with the
 * samples or with another output.
 * pt_default_cascade: 6 layers, start 1, base 8, kappa 1 (docs/EXPERIMENTS.md "Brightness cascade").                          */
typedef struct {
    uint32_t layers;         /* K, in [2, 8]                                                          */
    float start;             /* B_0: luminances up to it are never re-weighted; finite, > 0           */
    float base;              /* the ratio of consecutive levels; finite, >= 2                         */
    float kappa;             /* the count a layer needs to be kept in full; finite, >= 0; 0 = keep all */
} PtCascade;
void pt_default_cascade(PtCascade* out);
/* pt_render_device with the cascade resolve in place of the ordinary one, then the re-weighting pass: d_linear_rgb (width*height*3
 * floats) the cascade film, d_rgba8 (width*height*4 bytes, may be NULL) its display plane, d_plain_linear (width*height*3 floats,
 * may be NULL) the plain film.  Asynchronous on the context's stream.  The context owns the cascade state -- 3 (K + 1) doubles
 * per pixel for the sums and K doubles per pixel for the counts --, which grows at first use and is freed with the context; once
 * it is there the call allocates nothing beyond what pt_render_device does.  max_paths_in_flight cuts the job into sample batches
 * and the film does not depend on them.                                                                                      */
int pt_render_cascade_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, const PtCascade* cs,
                             float* d_linear_rgb, uint8_t* d_rgba8, float* d_plain_linear);
/* The same into host buffers (blocking).  Optional outputs (NULL: not wanted): out_plain_linear; out_layers, the layer sums
 * S_j, K*width*height*3 doubles, layer-major; out_weights, w_j(p) rounded to f32, K*width*height floats, layer-major.         */
int pt_render_cascade_host(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, const PtCascade* cs,
                           float* out_linear_rgb, uint8_t* out_rgba8, float* out_plain_linear, double* out_layers,
                           float* out_weights);
/* The two kernels on GIVEN samples: d_samples = n * width*height RGB records of 12 bytes on the device in the renders' own
 * sample-buffer layout, sample-major ([s * width*height + p]).  Needs no scene.  batch: the samples a launch of the resolve
 * kernel takes, so that n is cut into ceil(n / batch) launches that hand the sums on (0: all n in one); the film does not
 * depend on it.  Outputs as pt_render_cascade_device's.  Asynchronous on the context's stream.                               */
int pt_cascade_samples_device(PtContext* ctx, const PtCascade* cs, uint32_t width, uint32_t height, uint32_t n, uint32_t batch,
                              const float* d_samples, float* d_linear_rgb, uint8_t* d_rgba8, float* d_plain_linear);
/* The same samples in HOST memory through the rule header on the CPU, with the optional outputs of pt_render_cascade_host.
 * Needs no device and no context.                                                                                             */
int pt_cascade_host(const PtCascade* cs, uint32_t width, uint32_t height, uint32_t n, const float* samples, float* out_linear,
                    uint8_t* out_rgba8, float* out_plain, double* out_layers, float* out_weights);
/* Debug, host only: the split of one luminance -> the lower layer j and the two weights.                                      */
int pt_debug_cascade_split(const PtCascade* cs, double L, uint32_t* j, double* w_lo, double* w_hi);

/* Reconstruction filters (additive to ABI 6): the first stage behind the path kernel.  Every render resolves the film
 * as World::render_pixel does -- a pixel is the plain mean of the samples that started inside it, a box filter of radius 0.5; that
 * stays the default.  Here a pixel also takes the samples of its neighbours, each weighted by a separable filter of the distance
 * between the sample's position on the film and the pixel's centre.  No path kernel stores that position: sample s of pixel (x, y)
 * takes its jitter from words 0 and 1 of the Philox block (x, y, s, 0xFFFFFFFF; key 0) -- part of the ABI --, and k_resolve_filter,
 * which stands in for the ordinary resolve, recomputes it.  The rule (pathtrace_amd/csrc/pt_filter.h), all of it f64 with + - * /,
 * comparisons and selects only, so that the host and the device agree bit for bit:
 *   jitter      ox = (2 (w0 >> 9) + 1) / 2^24, oy the same of w1; y = film row, top-down; s counts from spp_offset
 *   position    the sample lies at (x + ox, y - oy) in pixel pitches, the centre of pixel q at (qx + 0.5, qy - 0.5)
 *   offsets     a sample of pixel p seen from q: tx = (px - qx) + (ox - 0.5), ty = (py - qy) - (oy - 0.5)
 *   weight      w = f(|tx|) f(|ty|); R = radius; f(t) = 0 for t >= R, else box 1; tent 1 - t / R; gaussian g(t) - g(R) with
 *               g(t) = exp_neg(alpha (t t)); mitchell with (B, C) and z = (2 t) / R the two cubic pieces in Horner form, / 6.
 *               exp_neg(e), e in [0, 100]: x = e / 256, the degree-15 Taylor polynomial of exp(-x) in Horner form with the
 *               coefficients (-1)^i (1 / i!), squared eight times; + and * only, no libm
 *   taps        m = the largest integer < R + 0.5 (0, 1 or 2); q takes the samples of the in-image pixels p with |px - qx| <= m
 *               and |py - qy| <= m
 *   sums        A_c += w v_c (the product rounded, then added) and Wt += w, only when w is not exactly 0 (a select: an infinite
 *               sample outside the support puts no NaN in); the plain sums P_c += v_c of the pixel's own samples beside them.
 *               Samples ascending, inside a sample py - qy ascending, then px - qx.  The sums carry over sample batches.
 *   film        Wt > 0: m_c = A_c / Wt, else m_c = P_c / n.  The linear plane is (float)m_c: under Mitchell it may be NEGATIVE
 *               and is kept; the RGBA8 plane is m_c through the sqrt, clamp and `as u8` steps of every render (negative -> 0);
 *               the plain film is P / n, bit-identical to pt_render_device's
 * Box with radius 0.5 is pt_render_device bit for bit, film and RGBA8.  params->exact_math changes the path kernels only.
 * No filtered form: row bands (band_count > 1), the lens, adaptive, progressive and multi-GPU renders, and the brightness cascade
 * together with a filter.
 * PT_ERR_INVALID_ARG, before the context is looked at: a null required argument, an unknown kind, a radius that is not finite or
 * outside [0.5, 2.5], a Gaussian alpha not finite or outside (0, 16], a Mitchell B or C not finite or outside [0, 1], an image
 * smaller than 2 x 2, band_count > 1, n = 0, a plane that is not 4-byte aligned (the weight sums: 8-byte), an output that shares
 * memory with the samples or with another output.
 * pt_default_filter: Gaussian, radius 1.5, alpha 2.                                                                              */
enum { PT_FILTER_BOX = 0, PT_FILTER_TENT = 1, PT_FILTER_GAUSSIAN = 2, PT_FILTER_MITCHELL = 3 };
typedef struct {
    uint32_t kind;           /* PT_FILTER_*                                                  */
    float radius;            /* R in pixel pitches, in [0.5, 2.5]                            */
    float a;                 /* gaussian: alpha in (0, 16]; mitchell: B in [0, 1]; else ignored */
    float b;                 /* mitchell: C in [0, 1]; else ignored                          */
} PtFilter;
void pt_default_filter(PtFilter* out);
/* pt_render_device with k_resolve_filter in place of the ordinary resolve: d_linear_rgb (width*height*3 floats) the filtered film,
 * d_rgba8 (width*height*4 bytes, may be NULL) its display plane, d_plain_linear (width*height*3 floats, may be NULL) the plain film.
 * Asynchronous on the context's stream.  The context owns the filter state -- 7 doubles per pixel --, which grows at first use and
 * is freed with the context; once it is there the call allocates nothing beyond what pt_render_device does.  max_paths_in_flight
 * cuts the job into sample batches and the film does not depend on them.                                                      */
int pt_render_filtered_device(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, const PtFilter* flt,
                              float* d_linear_rgb, uint8_t* d_rgba8, float* d_plain_linear);
/* The same into host buffers (blocking).  Optional outputs (NULL: not wanted): out_rgba8, out_plain_linear; out_weight_sum, Wt of
 * every pixel, width*height doubles.                                                                                            */
int pt_render_filtered_host(PtContext* ctx, const PtCamera* cam, const PtRenderParams* params, const PtFilter* flt,
                            float* out_linear_rgb, uint8_t* out_rgba8, float* out_plain_linear, double* out_weight_sum);
/* The kernel on GIVEN samples: d_samples = n * width*height RGB records of 12 bytes on the device in the renders' own sample-buffer
 * layout, sample-major ([s * width*height + y * width + x]); sample s has the sample index first_sample + s.  Needs no scene: the
 * jitter depends on (x, y, sample index) alone.  batch: the samples a launch takes, so that n is cut into ceil(n / batch) launches
 * that hand the sums on (0: all n in one); the film does not depend on it.  d_rgba8, d_plain_linear and d_weight_sum (width*height
 * doubles) may be NULL.  Asynchronous on the context's stream.                                                                   */
int pt_filter_samples_device(PtContext* ctx, const PtFilter* flt, uint32_t width, uint32_t height, uint32_t n, uint32_t first_sample,
                             uint32_t batch, const float* d_samples, float* d_linear_rgb, uint8_t* d_rgba8, float* d_plain_linear,
                             double* d_weight_sum);
/* The same samples in HOST memory through the rule header on the CPU.  Needs no device and no context.                          */
int pt_filter_host(const PtFilter* flt, uint32_t width, uint32_t height, uint32_t n, uint32_t first_sample, const float* samples,
                   float* out_linear, uint8_t* out_rgba8, float* out_plain, double* out_weight_sum);
/* Debug, host only: f(|t|) of the filter; the jitter (ox, oy) of sample `sample` of pixel (x, y); exp_neg(e) for e in [0, 100].  */
int pt_debug_filter_weight(const PtFilter* flt, double t, double* f);
int pt_debug_filter_offsets(uint32_t x, uint32_t y, uint32_t sample, double* ox, double* oy);
int pt_debug_filter_exp_neg(double e, double* out);

/* RenderingStrategy::ray_color(world, ray, depth = 0, rng, throughput = 1) (src/rendering.rs:34-142,
 * 214-265) for n arbitrary rays: rays = n * (origin3, direction3), the direction is normalised on
 * entry like Ray::new (camera.rs:10-16); xy = n * (x, y) = the RNG key of each ray's stream, and the
 * sample index of every stream is params->spp_offset.  out_rgb = n * 3 floats.  Host buffers,
 * blocking; the paths run through the same kernels as a render.                               */
int pt_ray_color(PtContext* ctx, const PtRenderParams* params, const double* rays,
                 const uint32_t* xy, uint32_t n, float* out_rgb);

/* Debug/parity entry: closest-hit scan of World::hit_scene (src/world.rs:270-290)
 * on the device for n arbitrary rays (host arrays; rays = n*6 doubles o,d; the
 * direction is normalised on entry like Ray::new, src/camera.rs:10-16).
 * out_id[i] = object index or -1, out_t[i] = hit distance.                   */
int pt_debug_hit_scene(PtContext* ctx, const double* rays, uint32_t n,
                       double t_min, double t_max, uint32_t exact_math, uint32_t accel,
                       int32_t* out_id, float* out_t);

/* The same with the HitRecord of every hit (src/objects/base.rs:6-33): out_rec = n * 8 floats
 * (t, point3, face-forwarded normal3, front_face as 0/1); zeros for a miss.   */
int pt_debug_hit_records(PtContext* ctx, const double* rays, uint32_t n,
                         double t_min, double t_max, uint32_t exact_math, uint32_t accel,
                         int32_t* out_id, float* out_rec);

/* Function-level parity entries: the per-vertex device functions of the path kernels on
 * arbitrary inputs, one item per thread.  `obj` = index of an object of the uploaded scene.  Host arrays.
 *   pt_debug_bsdf_eval     Material::bsdf_pdf (material.rs:86-91, 139-148, 221-265; mirror.rs:179-198)
 *                          in = n * (ray dir3, wo3, normal3, ray.eta_ratio) -> out = n * (f3, pdf)
 *   pt_debug_bsdf_sample   Material::bsdf_pdf_sample (material.rs:29-40; mirror.rs:200-305)
 *                          in = n * (ray dir3, normal3, eta_ratio), words = n * 4 raw RNG words (r1, r2, lobe u, -)
 *                          -> out = n * (wo3, f3, pdf, cos)
 *   pt_debug_shape_sample  Shape::sample_surface_from_point (shape.rs:91-145, 200-242) of object obj from
 *                          from3[i]; target3 != NULL: the look-ahead form (point given, no draws), else r12 =
 *                          n * (r1, r2) uniforms -> out = n * (point3, pdf_omega, light_dir3, distance)
 *   pt_debug_light_point   World::sample_light_point (world.rs:251-267) from from3[i]; words = n * 4
 *                          (light-index word, r1 word, r2 word, -) -> out = n * (point3, emission3, pdf, light object)
 *   pt_debug_camera_rays   Camera::get_ray_with_offset with the sample's own jitter draws (camera.rs:139-147,
 *                          world.rs:299); xys = n * (x, y film row, sample) -> out = n * (origin3, direction3, ox, oy) */
int pt_debug_bsdf_eval(PtContext* ctx, uint32_t obj, const double* in10, uint32_t n, uint32_t exact_math, float* out4);
int pt_debug_bsdf_sample(PtContext* ctx, uint32_t obj, const double* in7, const uint32_t* words4, uint32_t n,
                         uint32_t exact_math, float* out8);
int pt_debug_shape_sample(PtContext* ctx, uint32_t obj, const double* from3, const double* target3, const double* r12,
                          uint32_t n, uint32_t exact_math, float* out8);
int pt_debug_light_point(PtContext* ctx, const double* from3, const uint32_t* words4, uint32_t n, uint32_t exact_math,
                         float* out8);
int pt_debug_camera_rays(PtContext* ctx, const PtCamera* cam, const uint32_t* xys, uint32_t n, uint32_t exact_math,
                         float* out8);

/* Debug/parity entry: the two-ray scan of the regenerating path kernel (a visibility ray and a path ray from one origin
 * through the scene records in one pass) beside the two single-ray scans it stands for.  Scenes that live in LDS only
 * (PT_ERR_UNSUPPORTED otherwise).  rays10 = n * (origin3, dir_a3, dir_b3, t_max_a); directions are taken as given (not
 * normalised).  out6 = n * 6 raw 32-bit words: joint scan (hit on ray a as 0/1, object on ray b or -1, bound of ray b
 * after the scan as f32), then the same three from the separate any-hit and closest-hit scans.  Equal words = equal
 * results.                                                                                                            */
int pt_debug_joint_scan(PtContext* ctx, const double* rays10, uint32_t n, double t_min, double t_max_b,
                        uint32_t exact_math, float* out6);

/* Debug entry, host only (no GPU needed): build the accel = 1 BVH of a scene and verify it -- every object in
 * exactly one leaf slot with its scan record, every child box encloses the boxes beneath it, depth within the
 * traversal stack.  Returns PT_OK and the tree's size, or PT_ERR_UNSUPPORTED with the violated invariant in
 * pt_last_error().  Any of the three outputs may be NULL.                                                    */
int pt_debug_bvh_check(const PtObject* objs, uint32_t n_objs, uint32_t* depth, uint32_t* n_nodes,
                       uint32_t* n_leaf_slots);

/* Debug entry, host only (no GPU needed): build the tree of prev_objs, refit it to cur_objs on the host (the specification of
 * the device-side refit) and run the invariants of pt_debug_bvh_check on the result against cur_objs -- every object in one
 * slot with its CURRENT scan record, every child box encloses what is beneath it --, and that child codes and leaf ids are
 * the build's.  Both poses have the same n_objs and shape tags (PT_ERR_INVALID_ARG otherwise); PT_ERR_UNSUPPORTED for a
 * NaN/inf coordinate or a violated invariant.  refit = 0 skips the refit: the tree as built from prev_objs, verified against
 * prev_objs (what a refit to the pose of the build must reproduce bit for bit).  Optional outputs, the tree: out_qnodes (16 words per node, up to
 * cap_nodes nodes), out_leaf_rec (12 floats per leaf slot), out_leaf_lead (4 per slot), out_leaf_ids (1 per slot; up to
 * cap_slots slots), the counts, out_grid = grid_min[3], grid_cell[3], scene_abs, the root's child code, and the three cost
 * sums (dx dy, dy dz, dz dx in grid units) now and at build.                                                          */
int pt_debug_bvh_refit_check(const PtObject* prev_objs, const PtObject* cur_objs, uint32_t n_objs, uint32_t refit,
                             uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead, uint32_t* out_leaf_ids,
                             uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid, uint32_t* root,
                             uint64_t* cost_now, uint64_t* cost_at_build);
/* Debug entry, host only (no GPU needed): build the Morton tree of objs on the host (ptbvh::build_morton, the specification of
 * the device-side build) and run the invariants of pt_debug_bvh_check on it, and that the slots hold the objects in ascending
 * (key, index) order.  refit_objs (optional; same n_objs and shape tags): the tree of objs is then refitted to that pose by the
 * host refit and verified against it -- what pt_scene_refit after pt_scene_rebuild must reproduce; keys and order stay those
 * of objs.  PT_ERR_UNSUPPORTED for a NaN/inf coordinate, a violated invariant or an object count without a plan.
 * Optional outputs: the tree as pt_debug_bvh_refit_check returns it, and per object (up to cap_objs) its 30-bit key and the
 * sorted order (out_order[p] = object at sorted position p).                                                             */
int pt_debug_bvh_morton_check(const PtObject* objs, const PtObject* refit_objs, uint32_t n_objs, uint32_t* out_qnodes,
                              uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead, uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots,
                              float* out_grid, uint32_t* root, uint64_t* cost_now, uint32_t* out_keys, uint32_t* out_order,
                              uint32_t cap_objs);
/* Debug entry, host only: the topology of the Morton tree over n_objs objects, which depends on the count alone.
 * Optional outputs: per node (up to cap_nodes) its four child codes, its height and the node order by height; the first
 * position of every height in that order (n_heights entries, the last one the node count); the counts, the root's child code,
 * the stack entries a traversal can need and the deepest leaf.  PT_ERR_UNSUPPORTED when no tree fits the traversal stack.  */
int pt_debug_bvh_morton_topology(uint32_t n_objs, uint32_t* out_codes, uint32_t* out_height, uint32_t* out_order, uint32_t cap_nodes,
                                 uint32_t* out_height_first, uint32_t cap_heights, uint32_t* n_nodes, uint32_t* n_heights,
                                 uint32_t* n_slots, uint32_t* root, uint32_t* stack_need, uint32_t* depth);
/* pt_debug_bvh_morton_check for the median order (ptbvh::build_median, the specification of pt_scene_rebuild_ordered with
 * PT_BVH_ORDER_MEDIAN): the same invariants, outputs and errors, except that out_keys holds the three grid cells g of every
 * object (3 words per object, up to cap_objs objects) and that the order check is "the slots hold the order the rule gives",
 * by a second evaluation of the steps.                                                                                   */
int pt_debug_bvh_median_check(const PtObject* objs, const PtObject* refit_objs, uint32_t n_objs, uint32_t* out_qnodes,
                              uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead, uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots,
                              float* out_grid, uint32_t* root, uint64_t* cost_now, uint32_t* out_keys, uint32_t* out_order,
                              uint32_t cap_objs);
/* Debug entry, host only: the split plan of the median order over n_objs objects, which depends on the count alone.  Optional
 * outputs: the steps, four words each (level, P, Q, cut), ascending by (level, P), up to cap_steps; their number; and T, the
 * largest step the device runs inside one workgroup.  PT_ERR_UNSUPPORTED when no tree fits the traversal stack.          */
int pt_debug_bvh_median_plan(uint32_t n_objs, uint32_t* out_steps, uint32_t cap_steps, uint32_t* n_steps, uint32_t* tile);
/* The context's device tree copied back into the same outputs (blocking).  PT_ERR_INVALID_ARG when it holds no tree. */
int pt_debug_bvh_read(PtContext* ctx, uint32_t* out_qnodes, uint32_t cap_nodes, float* out_leaf_rec, float* out_leaf_lead,
                      uint32_t* out_leaf_ids, uint32_t cap_slots, uint32_t* n_nodes, uint32_t* n_slots, float* out_grid,
                      uint32_t* root, uint64_t* cost_now);

const char* pt_last_error(void);
uint32_t pt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PATHTRACE_AMD_H */
