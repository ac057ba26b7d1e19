// pt_context.h -- what the host files of the library share (internal to csrc/): the error channel, the owners of GPU
// resources, struct PtContext (its device BVH: struct DeviceBvh, pt_scene_bvh.h) and the few functions that cross files.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pathtrace_amd.h"
#include "pt_kernels.h"
#include "pt_sched.h"

// ---- the error channel (pt_host.cpp): the message pt_last_error returns, per thread
extern thread_local std::string g_err;
int pt_internal_fail(int code, const char* fmt, ...);
static constexpr auto& fail = pt_internal_fail;

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? PT_ERR_OOM : PT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                     \
    } while (0)

// ---- owners: each frees what it holds in its destructor; move-constructible, not copyable
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        if (n <= cap) return PT_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        HIP_TRY(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return PT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(bool timing) { return timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    operator hipEvent_t() const { return e; }
};
struct Stream {   // non-blocking
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
    operator hipStream_t() const { return s; }
};
template <class T> struct Pinned {   // host words the device can reach; dev: the device's address of a mapped allocation
    T* p = nullptr;
    T* dev = nullptr;
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : p(std::exchange(o.p, nullptr)), dev(std::exchange(o.dev, nullptr)) {}
    ~Pinned() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t n) { return hipHostMalloc((void**)&p, n * sizeof(T)); }
    hipError_t alloc_mapped(size_t n) {
        const hipError_t e = hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocMapped);
        return e != hipSuccess ? e : hipHostGetDevicePointer((void**)&dev, p, 0);
    }
};

struct TonemapState {   // pt_tonemap_device: the last histogram (258 words) and the exposure state, allocated and zeroed at first use
    DevBuf<uint32_t> hist;
    DevBuf<ptk::ExposureState> state;
    DevBuf<float> lin;            // pt_tonemap_host: device staging of the film (in place) and of the RGBA8 plane
    DevBuf<uint8_t> rgba;
    int ensure(hipStream_t st);   // pt_tonemap.cpp
};

#include "pt_scene_bvh.h"   // struct DeviceBvh, made of the owners above

// lanes, buffer sets and the core size of overlapping launches: pt_sched.h (the scheduler's constants)
using ptsched::kLanes;
using ptsched::kSets;
constexpr uint32_t kStatsWords = 32;            // 16 x u64 at the front of the counter buffer: 8 render statistics, 8 words for measurement builds (PT_DRAIN_TIMING)

struct PtContext {
    int device = 0;
    uint32_t n_cus = 256;             // compute units of the device (grid of the regenerating level-0 launch)
    Stream own_stream;
    hipStream_t stream = nullptr;     // the caller's (pt_context_set_stream) or own_stream
    PtTuning tuning{};                // pt_context_set_tuning; 0 = library default
    // scene
    DevBuf<float4> scan, shape, mat, blob;
    DevBuf<float4> shape_x, mat_x, blob_x;   // the exact_math = 1 copies: the records carry per-object constants evaluated in that mode (k_scene_setup)
    DevBuf<ptk::Run> runs;
    DevBuf<uint32_t> lights;
    ptk::SceneView view{};
    bool has_scene = false;
    bool split_ok = false;            // a minority of the objects is Mirror: the regenerating form that batches their vertices pays
    uint32_t scan_counts[3] = {0, 0, 0};   // entries of the scan array by kind: spheres, single triangles, triangle pairs (pt_debug_scan_layout)
    uint32_t regen_occ[2][2][2] = {};  // cached occupancy query [exact_math][integrator][split] of this scene (0: not asked yet)
    // BVH (PtRenderParams.accel): the host copy of the shape records the first build reads, the shape tags on the device (uploaded
    // with the scene; no later call can change them) for the device builds, and the device tree itself -- one object with its
    // invariants and operations (pt_scene_bvh.h); no other file reads or writes its state
    std::vector<float4> h_shape;
    std::vector<uint32_t> h_shape_tag;
    DevBuf<uint32_t> shape_tag;
    bool auto_bvh = false;            // PT_ACCEL_AUTO would take the BVH for this scene (ptscene::kAutoBvhWeight)
    DeviceBvh tree;
    // wavefront state
    DevBuf<float4> xchg;              // k_paths_regen_split: exchange stacks of every wave, one region per lane (stride: sched.xchg_stride)
    DevBuf<float4> queue[4];
    DevBuf<float4> bvh_aux, bvh_sray[2];   // accel = 1: per-slot scratch of the staged passes (k_paths_bvh)
    DevBuf<float4> ovf[2][4];         // overflow queues of the tail hand-off: [batch parity][plane]
    DevBuf<uint32_t> ovf_count;       // per batch parity: leftover count, chunk counters (kCountStride)
    DevBuf<double> film;
    // scheduling
    // multi-batch renders: the continuation launches and the film resolve of batch k run on side_stream while the
    // level-0 launch of batch k + 1 runs on the caller's stream (their own queue and a second sample buffer)
    Stream side_stream;
    DevBuf<float4> cqueue[4];
    DevBuf<float4> caux, csray[2];    // ... and, for accel = 1, its own staged-pass scratch
    Event ev_l0[2], ev_resolved[2];
    // regenerating launches: kLanes LANES (streams of their own) taken in turn by consecutive sample batches -- of one render or
    // of renders enqueued back to back --, so that the launches of batches k + 1 and k + 2 fill the device while the last waves
    // of batch k run dry; the resolves stay in order on the caller's stream
    Stream lane_stream[kLanes];
    Event lane_done[kLanes], lane_begun[kLanes], ev_pre, ev_switch;
    Pinned<uint32_t> h_posted;        // host memory the device reads: number of the last lanes launch enqueued (BounceArgs.posted = h_posted.dev)
    // ... and kSets buffer sets (sample buffer + launch counters) taken in turn: a resolve gets few wave slots beside resident
    // regenerating launches (146 us of work take ~0.9 ms: measured), so the launch of batch k + kSets is the first to wait for
    // the resolve of batch k
    Event set_free[kSets];
    DevBuf<ptk::Rgb> lsamp[kSets];    // by set number (renders without lanes: sets 0 and 1; pt_render_pixels reads set 0)
    // Which lane / buffer set comes next, which events have been recorded, which device-side words are known to be zero: the
    // scheduling state.  render_impl plans on a copy (ptsched::plan, pure) and commits it after the last operation was enqueued.
    ptsched::State sched;
    int64_t debug_fail_at = -1;       // pt_debug_fail_after: the stream operation of the next render that fails (test hook)
    std::vector<uint32_t> launch_log;  // pt_debug_launch_log: instance code of every path-kernel launch enqueued since it was last read
    // statistics
    uint64_t expected_samples = 0;    // tile pixels x spp of the renders enqueued since the statistics were last collected (pt_sync compares)
    uint64_t capture_gcd = 0;         // gcd of the sample counts of the renders captured into graphs (replays add multiples of them)
    Pinned<unsigned long long> h_dstats;
    std::vector<Event> ev_pool;
    Event ev_begin, ev_end;
    PtStats stats{};
    std::vector<uint32_t> primary_events;      // slots of the level-0 launches
    // staging and scratch of the entries
    DevBuf<float> host_lin;       // device staging of pt_render_host
    DevBuf<uint8_t> host_rgba;
    Pinned<uint32_t> h_ovf;           // pinned read-back of one counter
    // pixel-list entries (pt_render_pixels, pt_ray_color)
    DevBuf<uint2> pixel_list;
    DevBuf<float4> inject[4];
    DevBuf<float> fn_in, fn_out;               // pt_debug_* function entries
    DevBuf<uint32_t> fn_words;
    // pt_render_adaptive: image-indexed per-pixel state (ptk::AdaptiveFilm), the active lists of two consecutive passes,
    // and [survivor count | per-workgroup counts of k_adaptive_select]
    DevBuf<double> ad_sums;
    DevBuf<uint32_t> ad_count, ad_conv, ad_words;
    DevBuf<float> ad_err;
    DevBuf<uint2> ad_list[2];
    // ... which stays behind a completed render for pt_adaptive_variance_device: ad_valid with that render's image size
    bool ad_valid = false;
    uint32_t ad_width = 0, ad_height = 0;
    // pt_render_features_device: one batch of rays, their hits (ids, records) and the BVH scratch of launch_debug_hit;
    // pt_denoise_device: the two (u, var) ping-pong planes; pt_render_denoised: device staging of the features and the output
    DevBuf<float> ft_rays, ft_t, ft_rec;      // (launch_debug_hit writes t for every ray: ft_t)
    DevBuf<int32_t> ft_ids;
    DevBuf<float4> ft_scratch, dn_plane[2], dn_feat;
    DevBuf<float> dn_lin;
    DevBuf<float> dn_var;                     // pt_render_adaptive_denoised: device staging of the variance plane
    DevBuf<int32_t> dn_ids;                   // pt_render_denoised_motion: device staging of the ids
    DevBuf<float4> up_feat;                   // pt_render_denoised_upsampled: device staging of the full-size features and film
    DevBuf<float> up_lin;
    // pt_denoise_temporal_device: two history buffers of 3 float4 per pixel (ptk::TemporalArgs), tm_hist[tm_cur] holds the
    // last frame's when tm_valid; the camera and size of that frame
    DevBuf<float4> tm_hist[2];
    uint32_t tm_cur = 0;
    bool tm_valid = false;
    PtCamera tm_cam{};
    // pt_scene_update / pt_denoise_temporal_motion_device: the f64 shape fields (9 per object) of the current scene and of the
    // HISTORY POSE, the scene as it was when a temporal entry last stored a history frame; pose_gen counts the scene changes,
    // tm_pose_gen is its value at that snapshot, and mo_key names the pair of poses the device maps were computed from
    std::vector<double> pose, tm_pose;
    uint64_t pose_gen = 0, tm_pose_gen = 0, mo_key[2] = {~0ull, ~0ull};
    // two host staging vectors, used in turn: mo_staged[k] is recorded behind the copy out of h_maps[k], so a new set of maps
    // waits only for the copy of two sets ago, not for the stream
    std::vector<ptk::MotionMap> h_maps[2];
    Event mo_staged[2];
    uint32_t mo_slot = 0;
    DevBuf<ptk::MotionMap> mo_maps;
    // pt_temporal_gradient_device: the strata's pixel list, their re-traced film (3 floats per stratum) and records (2 doubles)
    DevBuf<uint2> gr_list;
    DevBuf<float> gr_film;
    DevBuf<double> gr_rec;
    // pt_render_denoised_gradient: device staging of the alpha plane, and the previous frame -- the noisy film of the last
    // frame this entry completed (gr_prev, 12 B per pixel) with its parameters and camera, held while gr_valid
    // (pt_scene_upload and pt_temporal_reset drop it); gr_frame counts the frames completed since it was last dropped (the
    // seed of the strata)
    DevBuf<float> gr_alpha, gr_prev;
    bool gr_valid = false;
    PtRenderParams gr_params{};
    PtCamera gr_cam{};
    uint32_t gr_frame = 0;
    // pt_tonemap_device: the exposure lives on the device; no scene entry touches it
    TonemapState tone;
    // pt_render_cascade_device / pt_cascade_samples_device: the layer sums and plain sums of every pixel ((3 K + 3)
    // planes of doubles) and the K count planes; they grow at first use.  pt_render_cascade_host: device staging of the plain film
    // and of the weight planes
    DevBuf<double> cas_state, cas_cnt;
    DevBuf<float> cas_plain, cas_weights;
    // pt_render_filtered_device / pt_filter_samples_device: the weighted sums, the weight sum and the plain sums of
    // every pixel (7 planes of doubles); grows at first use.  pt_render_filtered_host: device staging of the plain film
    DevBuf<double> flt_state;
    DevBuf<float> flt_plain;
    // pt_bloom_device: the pyramid, every level three planes of floats; pt_display_device: the bloomed film between
    // the two stages.  Both grow at the first call of a size and never afterwards.  bloom_no_tail: pt_debug_bloom_tail switched
    // k_bloom_tail off (the per-level kernels run every level; same bits)
    DevBuf<float> bloom_pyr, bloom_lin;
    bool bloom_no_tail = false;
    // pt_bake_*_host: device staging of the texel records or probe positions and of the SH coefficients (the film
    // goes through host_lin / host_rgba)
    DevBuf<float> bake_in, bake_sh;
    // pt_probe_grid_bake_device: the grid's positions and the radiance plane of its bake; pt_render_probe_lit_device:
    // the feature plane (pt_render_probe_lit_host stages the coefficients in bake_sh and the film in host_lin / host_rgba)
    DevBuf<float> pg_pos, pg_rad;
    DevBuf<float4> pg_feat;
    // pt_probe_grid_visibility_device: the distance plane of the grid's probe rays; pt_probe_distances_host: device
    // staging of its output (the positions go through bake_in); pt_render_probe_lit_visibility_host: device staging of the moment maps
    DevBuf<float> pv_dist, pv_out;
    DevBuf<float2> pv_mom;
    // pt_probe_grid_update_device: the radiance and the distance plane of the call's slots; pt_probe_grid_update_host:
    // device staging of the ages (the coefficients go through bake_sh, the maps through pv_mom)
    DevBuf<float> pu_rad, pu_dist;
    DevBuf<uint32_t> pu_age;
};

// What a render does with the f64 film sums (pt_render_progressive carries them across calls).
struct FilmState {
    bool load = false;        // start from the sums in c->film
    bool store = false;       // keep the sums (more samples follow in a later call)
    uint32_t div = 0;         // samples the mean is taken over (0: this call's spp)
};
// Pixel-list render: film slot i <-> image pixel d_pixels[i]; inject: the paths are given (pt_ray_color) instead of
// generated by the camera.
struct ListRender {
    const uint2* d_pixels = nullptr;
    uint32_t n = 0;
    const float4* inject[4] = {nullptr, nullptr, nullptr, nullptr};
    bool regen = false;       // the list may take the regenerating level-0 kernel (pt_render_adaptive's passes)
    // inject only (pt_render_lens_device): the given paths are those of the camera's TILE -- film slot = (tile row, x), RNG key
    // (x, image row), bands as in a plain render, no pixel list (d_pixels and n unused) --, inject_spp samples of every pixel,
    // state s_local * np + tile pixel (0: one sample)
    bool tile = false;
    uint32_t inject_spp = 0;
    // tile only (the bakes): the film is no camera's image -- no camera ray is ever generated for it, so a width or height of 1
    // is as good as any
    bool no_camera = false;
};
// A pass of pt_render_adaptive: the film resolve is k_resolve_adaptive into the image-indexed state instead of k_resolve.
struct AdaptivePass {
    ptk::AdaptiveFilm f{};
    bool load = false;        // the pixels already have samples (every pass after the first)
    uint32_t n_total = 0;     // samples per pixel of the pass's pixels once it is done
};

// A cascade render (pt_render_cascade_device): the film resolve is k_resolve_cascade into the context's cascade state instead of
// k_resolve; the caller launches k_cascade_reweight behind the render.
struct CascadePass {
    ptk::CascadeResolveArgs r{};   // the levels and the state planes; the launch fills in its batch
};

// A filtered render (pt_render_filtered_device): the film resolve is k_resolve_filter into the context's filter state instead of
// k_resolve; its finalising launch writes the planes.
struct FilterPass {
    ptk::FilterResolveArgs r{};    // the rule, the state and the output planes; the launch fills in its batch
};

// ---- functions that cross files
int render_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const FilmState& fs, const ListRender* list,
                float* d_linear, uint8_t* d_rgba, void* d_packed = nullptr, const AdaptivePass* ad = nullptr,
                const CascadePass* cas = nullptr, const FilterPass* flt = nullptr);   // pt_api.cpp
int render_adaptive_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtAdaptive* ad);   // pt_api.cpp
// The source of a frame's first rays as an entry receives it: a lens, a projection, or neither (the pinhole camera).
struct FrameSource {
    const PtLens* lens = nullptr;
    const PtProjection* proj = nullptr;
};
// The source and the camera's frame checked (a check answers in the entry's name, who), the kernels' words.  No context.  (pt_api.cpp)
int source_setup(const char* who, const PtCamera* cam, const FrameSource& src, ptk::RaySourceF* out);
// The driver of every render of injected camera paths (pt_api.cpp): per sample batch it launches the source's paths form into the
// context's inject planes and renders them.  The caller has checked what is its own.  no_camera: ListRender::no_camera (the bakes)
int render_injected_impl(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const ptk::RaySourceF& src, float* d_linear,
                         uint8_t* d_rgba, bool no_camera = false);
// pt_render_lens_device and pt_render_projection_device in the name `who` (pt_api.cpp): src holds the lens or the projection
int render_source_impl(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm, float* d_linear,
                       uint8_t* d_rgba);
// the words of xys = n * (x, y, sample) through the source's debug form into out = n * stride floats; blocking (pt_debug.cpp)
int debug_source_rays(PtContext* c, const ptk::RaySourceF& src, const uint32_t* xys, uint32_t n, uint32_t exact_math, uint32_t stride, float* out);
int lens_setup(const char* who, const PtCamera* cam, const PtLens* lens, ptk::LensF* out);                  // pt_lens.cpp
int projection_setup(const char* who, const PtCamera* cam, const PtProjection* proj, ptk::ProjF* out);      // pt_projection.cpp
ptk::CameraF camera_f32(const PtCamera* cam);                                                               // pt_lens.cpp
// the bake as a ray source: a film of width x height texels, or directions x probes, over the device records d_data (pt_bake.cpp)
ptk::RaySourceF bake_source(uint32_t kind, uint32_t width, uint32_t height, const float* d_data);
// The lens and projection forms of pt_render_features_device and pt_render_denoised (pt_denoise.cpp; their entries: pt_lens.cpp,
// pt_projection.cpp), src not empty
int features_source_device(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm,
                           uint32_t n_samples, float* d_features);
int render_source_denoised_host(const char* who, PtContext* c, const PtCamera* cam, const FrameSource& src, const PtRenderParams* prm,
                                uint32_t feature_samples, const PtDenoise* dn, float* out_linear, uint8_t* out_rgba, float* out_noisy,
                                float* out_features);
int denoised_frame_device(const char* who, PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples,
                          const PtDenoise* dn, PtRenderParams* p);   // pt_denoise.cpp
int tonemap_check_args(const char* who, uint32_t width, uint32_t height, const float* d_linear, const PtTonemap* tm, const float* d_out_linear,
                       const uint8_t* d_out_rgba);                  // pt_tonemap.cpp
ptk::SceneView view_for(const PtContext* c, uint32_t exact_math);   // pt_scene.cpp
int ensure_bvh(PtContext* c);                                       // pt_scene.cpp
hipStream_t pt_internal_stream(PtContext* c);                       // pt_context.cpp
void pt_internal_register_atexit(void);                             // pt_context.cpp
void pt_internal_multi_shutdown(void);                              // pt_multi.cpp
