//! Raw declarations of `include/pathtrace_amd.h` (ABI version 6).  Field order, types and names follow the
//! header exactly; `tests/test_rust_binding.py` checks that.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const PT_ABI_VERSION: u32 = 6;

pub const PT_OK: c_int = 0;
pub const PT_ERR_INVALID_ARG: c_int = 1;
pub const PT_ERR_NO_DEVICE: c_int = 2;
pub const PT_ERR_HIP: c_int = 3;
pub const PT_ERR_OOM: c_int = 4;
pub const PT_ERR_UNSUPPORTED: c_int = 5;

pub const PT_SHAPE_SPHERE: u32 = 0;
pub const PT_SHAPE_TRIANGLE: u32 = 1;
pub const PT_MAT_LAMBERT: u32 = 0;
pub const PT_MAT_EMISSIVE: u32 = 1;
pub const PT_MAT_MIRROR: u32 = 2;
pub const PT_MAT_OREN_NAYAR: u32 = 3;
pub const PT_INTEGRATOR_MIS: u32 = 0;
pub const PT_INTEGRATOR_BRDF_ONLY: u32 = 1;
pub const PT_ACCEL_LINEAR: u32 = 0;
pub const PT_ACCEL_BVH: u32 = 1;
pub const PT_ACCEL_AUTO: u32 = 2;
pub const PT_BVH_ORDER_MORTON: u32 = 0;
pub const PT_BVH_ORDER_MEDIAN: u32 = 1;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtCamera {
    pub origin: [f64; 3],
    pub lower_left: [f64; 3],
    pub horizontal: [f64; 3],
    pub vertical: [f64; 3],
    pub width: u32,
    pub height: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PtObject {
    pub shape_tag: u32,
    pub mat_tag: u32,
    pub shape: [f64; 9],
    pub mat: [f64; 6],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PtRenderParams {
    pub spp: u32,
    pub spp_offset: u32,
    pub min_depth: u32,
    pub max_depth: u32,
    pub integrator: u32,
    pub t_min: f64,
    pub band_rows: u32,
    pub band_index: u32,
    pub band_count: u32,
    pub max_paths_in_flight: u64,
    pub profile: u32,
    pub workgroups: u32,
    pub exact_math: u32,
    pub accel: u32,
    pub n_devices: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtTuning {
    pub export_below: u32,
    pub bvh_refill: u32,
    pub bvh_leaf: u32,
    pub cont_workgroups: u32,
    pub level0_form: u32,
    pub regen_workgroups: u32,
    pub in_order: u32,
}

/// pt_render_adaptive: the stopping rule's parameters (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtAdaptive {
    pub spp_min: u32,
    pub spp_step: u32,
    pub rel_tol: f64,
    pub abs_floor: f64,
}

/// pt_denoise_device: the edge-avoiding a-trous filter's parameters (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtDenoise {
    pub iterations: u32,
    pub sigma_l: f32,
    pub sigma_n: f32,
    pub sigma_d: f32,
}

/// pt_denoise_temporal_device: temporal accumulation with camera reprojection (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtTemporal {
    pub alpha: f32,
    pub depth_tol: f32,
    pub normal_tol: f32,
}

/// pt_temporal_gradient_device: the window and gain of the temporal gradient (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtGradient {
    pub radius: u32,
    pub scale: f32,
}

/// pt_tonemap_device: exposure, curve and transfer of the display transform (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtTonemap {
    pub mode: u32,
    pub curve: u32,
    pub transfer: u32,
    pub ev: f32,
    pub key: f32,
    pub pct_lo: f32,
    pub pct_hi: f32,
    pub log2_min: f32,
    pub log2_max: f32,
    pub adapt: f32,
    pub white: f32,
}
pub const PT_EXPOSURE_AUTO: u32 = 0;
pub const PT_EXPOSURE_MANUAL: u32 = 1;
pub const PT_CURVE_CLAMP: u32 = 0;
pub const PT_CURVE_REINHARD: u32 = 1;
pub const PT_CURVE_ACES: u32 = 2;
pub const PT_TRANSFER_SQRT: u32 = 0;
pub const PT_TRANSFER_SRGB: u32 = 1;

/// pt_render_projection_device: the projection beside the camera (include/pathtrace_amd.h); kind = PT_PROJ_*.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtProjection {
    pub kind: u32,
    pub reserved: u32,
    pub fov_degrees: f64,
}
pub const PT_PROJ_PERSPECTIVE: u32 = 0;
pub const PT_PROJ_ORTHOGRAPHIC: u32 = 1;
pub const PT_PROJ_FISHEYE: u32 = 2;
pub const PT_PROJ_EQUIRECT: u32 = 3;
/// pt_debug_bake_rays / pt_bake_rays_host: what the film of a bake holds
pub const PT_BAKE_TEXELS: u32 = 0;
pub const PT_BAKE_PROBES: u32 = 1;

/// A regular grid of SH probes (the irradiance volume): probe (ix, iy, iz) has index (iz ny + iy) nx + ix
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtProbeGrid {
    pub origin: [f64; 3],
    pub spacing: [f64; 3],
    pub counts: [u32; 3],
    pub reserved: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtProbeShade {
    pub normal_bias: f32,
    pub weight: u32,
}
pub const PT_PROBE_WEIGHT_TRILINEAR: u32 = 0;
pub const PT_PROBE_WEIGHT_FACING: u32 = 1;
/// pt_probe_moments_*, pt_probe_shade_visibility_*: the probes' octahedral distance-moment maps (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtProbeVisibility {
    pub resolution: u32,
    pub sharpness_log2: u32,
    pub max_distance: f32,
    pub reserved: u32,
}
/// pt_probe_grid_update_device, pt_probe_blend_*: one update of the irradiance volume over frames (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtProbeUpdate {
    pub rays_per_probe: u32,
    pub first: u32,
    pub stride: u32,
    pub hysteresis: f32,
    pub change_threshold: f32,
    pub change_alpha: f32,
    pub rotation: [f32; 9],
    pub reserved: u32,
}

/// pt_render_lens_device: the thin lens beside the camera (include/pathtrace_amd.h); aperture 0 = pinhole.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtLens {
    pub aperture: f64,
    pub focus_distance: f64,
}

/// pt_upsample_device: the edge-stopping weights of feature-guided upsampling (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtUpsample {
    pub sigma_n: f32,
    pub sigma_d: f32,
}

/// pt_render_cascade_device: the brightness cascade of the firefly-robust film (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtCascade {
    pub layers: u32,
    pub start: f32,
    pub base: f32,
    pub kappa: f32,
}

/// pt_bloom_device / pt_display_device: the bloom stage in front of the tone mapper (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtBloom {
    pub levels: u32,
    pub threshold: f32,
    pub knee: f32,
    pub clamp: f32,
    pub scatter: f32,
    pub intensity: f32,
}

/// pt_render_filtered_device: the reconstruction filter of the film (include/pathtrace_amd.h).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtFilter {
    pub kind: u32,
    pub radius: f32,
    pub a: f32,
    pub b: f32,
}
pub const PT_FILTER_BOX: u32 = 0;
pub const PT_FILTER_TENT: u32 = 1;
pub const PT_FILTER_GAUSSIAN: u32 = 2;
pub const PT_FILTER_MITCHELL: u32 = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtStats {
    pub samples: u64,
    pub vertices: u64,
    pub shadow_rays: u64,
    pub bounce_launches: u32,
    pub batches: u32,
    pub max_depth_reached: u32,
    pub reserved: u32,
    pub bounce_kernel_ms: f64,
    pub total_ms: f64,
    pub primary_vertices: u64,
    pub primary_kernel_ms: f64,
    pub primary_launches: u32,
    pub reserved2: u32,
    pub samples_expected: u64,
}

/// `pt_multi_info`: what a multi-device object is made of.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtMultiInfo {
    pub n_devices: u32,
    pub comm_count: u32,
    pub rccl_version: u32,
    pub threaded: u32,
    pub frames: u64,
    pub enqueue_us_sum: f64,
    pub enqueue_us_max: f64,
    pub exchange: u32,
    pub reserved_: u32,
}
pub const PT_EXCHANGE_RCCL: u32 = 0;
pub const PT_EXCHANGE_COPY: u32 = 1;

#[repr(C)]
pub struct PtContext {
    _private: [u8; 0],
}
#[repr(C)]
pub struct PtMulti {
    _private: [u8; 0],
}
/// The launch scheduler on a state of its own (host only; `pt_debug_sched_*`, tests).
#[repr(C)]
pub struct PtSched {
    _private: [u8; 0],
}
/// A render as the scheduler sees it (`csrc/pt_sched.h`: `Job`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtSchedJob {
    pub n_batches: u32,
    pub regen: u32,
    pub split: u32,
    pub hand_off: u32,
    pub regen_export: u32,
    pub profile: u32,
    pub in_order: u32,
    pub capturing: u32,
    pub grid: u32,
    pub regen_grid: u32,
    pub cont_grid: u32,
    pub regen_capacity: u32,
    pub fixed_grid: u32,
    pub counter_words: u32,
    pub xchg_need: u64,
}
/// One stream operation of a planned render (`csrc/pt_sched.h`: `Op`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtSchedOp {
    pub kind: u32,
    pub stream: u32,
    pub event: u32,
    pub pool: u32,
    pub set: u32,
    pub lane: u32,
    pub level: u32,
    pub own_queue: u32,
    pub ovf_par: u32,
    pub batch: u32,
    pub grid: u32,
    pub seq: u32,
    pub core: u32,
    pub flags: u32,
    pub zero_words: u32,
    pub reserved: u32,
    pub xchg_off: u64,
    pub xchg_len: u64,
}
/// What the launch sizing reads (`csrc/pt_shape.h`: `In`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtShapeIn {
    pub np: u64,
    pub max_paths_in_flight: u64,
    pub spp: u32,
    pub workgroups: u32,
    pub accel: u32,
    pub profile: u32,
    pub list: u32,
    pub list_regen: u32,
    pub inject: u32,
    pub n_objs: u32,
    pub blob_f4: u32,
    pub diffuse_only: u32,
    pub split_ok: u32,
    pub n_cus: u32,
    pub export_below: u32,
    pub cont_workgroups: u32,
    pub level0_form: u32,
    pub regen_workgroups: u32,
    pub in_order: u32,
    pub capturing: u32,
    pub inject_spp: u32,
    pub reserved: u32,
}
/// The sizing of a render (`csrc/pt_shape.h`: `Form`, `Shape`); `job` goes to `pt_debug_sched_render` as it is.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtShapeOut {
    pub lds_job: u32,
    pub split: u32,
    pub regen_scene: u32,
    pub over_cap: u32,
    pub cap: u64,
    pub n_paths_max: u64,
    pub ovf_slots: u64,
    pub q_slots_cont: u64,
    pub q_slots: u64,
    pub np: u32,
    pub spp: u32,
    pub nb_max: u32,
    pub n_batches: u32,
    pub export_small: u32,
    pub paths_per_wave: u32,
    pub small_scene: u32,
    pub hand_off: u32,
    pub regen: u32,
    pub overlap: u32,
    pub grid: u32,
    pub nw: u32,
    pub seg_cap: u32,
    pub regen_per_cu: u32,
    pub regen_capacity: u32,
    pub regen_grid: u32,
    pub regen_launch_grid: u32,
    pub cont_grid: u32,
    pub nw_cont: u32,
    pub seg_cap_cont: u32,
    pub regen_export: u32,
    pub reserved: u32,
    pub job: PtSchedJob,
}
/// The per-launch words of a planned launch (`csrc/pt_shape.h`: `Launch`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PtShapeLaunch {
    pub s0: u32,
    pub nb: u32,
    pub n_first: u32,
    pub seg_cap: u32,
    pub src_mode: u32,
    pub export_below: u32,
    pub regen_static: u32,
    pub reserved: u32,
}

/// `pt_context_set_stream`: HIP's legacy default stream (its handle, 0, means "the context's own stream").
pub const PT_STREAM_LEGACY_DEFAULT: usize = 1;

pub type PtProgressFn = Option<
    unsafe extern "C" fn(user: *mut c_void, spp_done: u32, spp_total: u32, rgba8: *const u8, linear_rgb: *const f32) -> c_int,
>;

extern "C" {
    pub fn pt_camera_new(origin: *const f64, width: u32, height: u32, screen_distance: f64, fov_degrees: f64, out: *mut PtCamera) -> c_int;
    pub fn pt_camera_look_at(origin: *const f64, target: *const f64, up: *const f64, width: u32, height: u32, fov_degrees: f64, out: *mut PtCamera) -> c_int;
    pub fn pt_default_params(out: *mut PtRenderParams);
    pub fn pt_tile_rows(height: u32, band_rows: u32, band_index: u32, band_count: u32) -> u32;
    pub fn pt_builtin_scene(id: u32, arg: u32, objs: *mut PtObject, cap: u32, n: *mut u32) -> c_int;
    pub fn pt_context_create(device: c_int, out: *mut *mut PtContext) -> c_int;
    pub fn pt_context_destroy(ctx: *mut PtContext) -> c_int;
    pub fn pt_context_set_stream(ctx: *mut PtContext, hip_stream: *mut c_void) -> c_int;
    pub fn pt_context_set_tuning(ctx: *mut PtContext, tuning: *const PtTuning) -> c_int;
    pub fn pt_scene_upload(ctx: *mut PtContext, objs: *const PtObject, n_objs: u32) -> c_int;
    pub fn pt_render_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_render_device_packed(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, d_packed: *mut c_void) -> c_int;
    pub fn pt_sync(ctx: *mut PtContext) -> c_int;
    pub fn pt_get_stats(ctx: *mut PtContext, out: *mut PtStats) -> c_int;
    pub fn pt_debug_raw_stats(ctx: *mut PtContext, out16: *mut u64) -> c_int;
    pub fn pt_debug_scan_layout(ctx: *mut PtContext, n_spheres: *mut u32, n_triangles: *mut u32, n_pairs: *mut u32) -> c_int;
    pub fn pt_debug_spheres_only(ctx: *mut PtContext, objs: *const PtObject, n: u32, out: *mut u32) -> c_int;
    pub fn pt_debug_lambert_surfaces(ctx: *mut PtContext, objs: *const PtObject, n: u32, out: *mut u32) -> c_int;
    pub fn pt_render_host(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_progressive(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, spp_step: u32, f: PtProgressFn, user: *mut c_void, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render(cam: *const PtCamera, objs: *const PtObject, n_objs: u32, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_shutdown();
    pub fn pt_multi_create(devices: *const c_int, n_devices: u32, out: *mut *mut PtMulti) -> c_int;
    pub fn pt_multi_destroy(m: *mut PtMulti) -> c_int;
    pub fn pt_multi_device_count(m: *const PtMulti) -> u32;
    pub fn pt_multi_set_threads(m: *mut PtMulti, enabled: c_int) -> c_int;
    pub fn pt_multi_set_exchange(m: *mut PtMulti, mode: u32) -> c_int;
    pub fn pt_multi_info(m: *mut PtMulti, out: *mut PtMultiInfo) -> c_int;
    pub fn pt_debug_multi_create_shared(device: c_int, n: u32, out: *mut *mut PtMulti) -> c_int;
    pub fn pt_debug_feeder_selftest(n_workers: u32, n_frames: u32, spin: u32, fail_at: i32, order_out: *mut u64, n_out: *mut u32) -> c_int;
    pub fn pt_debug_sched_create(out: *mut *mut PtSched) -> c_int;
    pub fn pt_debug_sched_destroy(s: *mut PtSched);
    pub fn pt_debug_sched_render(s: *mut PtSched, job: *const PtSchedJob, faults: u32, fail_after: u32, ops: *mut PtSchedOp, cap: u32, n_ops: *mut u32, lanes: *mut u32) -> c_int;
    pub fn pt_debug_sched_sync(s: *mut PtSched, collect: u32) -> c_int;
    pub fn pt_debug_render_shape(input: *const PtShapeIn, occupancy: u32, out: *mut PtShapeOut, ops: *const PtSchedOp, n_ops: u32, launches: *mut PtShapeLaunch) -> c_int;
    pub fn pt_debug_fail_after(ctx: *mut PtContext, n: i64) -> c_int;
    pub fn pt_debug_launch_log(ctx: *mut PtContext, out: *mut u32, cap: u32, n: *mut u32) -> c_int;
    pub fn pt_debug_path_instances(out: *mut u32, cap: u32, n: *mut u32) -> c_int;
    pub fn pt_multi_scene_upload(m: *mut PtMulti, objs: *const PtObject, n_objs: u32) -> c_int;
    pub fn pt_multi_set_tuning(m: *mut PtMulti, tuning: *const PtTuning) -> c_int;
    pub fn pt_multi_render_device(m: *mut PtMulti, cam: *const PtCamera, params: *const PtRenderParams, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_multi_sync(m: *mut PtMulti) -> c_int;
    pub fn pt_multi_get_stats(m: *mut PtMulti, out: *mut PtStats) -> c_int;
    pub fn pt_multi_render_host(m: *mut PtMulti, cam: *const PtCamera, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_multi(devices: *const c_int, n_devices: u32, cam: *const PtCamera, objs: *const PtObject, n_objs: u32, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_film_pack(hip_stream: *mut c_void, d_linear_rgb: *const f32, d_rgba8: *const u8, n_pixels: u32, d_packed: *mut c_void) -> c_int;
    pub fn pt_film_unpack(hip_stream: *mut c_void, d_gathered: *const c_void, width: u32, height: u32, band_rows: u32, n_ranks: u32, max_rows: u32, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_debug_multi_emulate(ctx: *mut PtContext, n_virtual: u32, cam: *const PtCamera, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_pixels(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, xy: *const u32, n: u32, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_samples: *mut f32) -> c_int;
    pub fn pt_render_adaptive(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, ad: *const PtAdaptive, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_spp: *mut u32, out_rel_err: *mut f32) -> c_int;
    pub fn pt_render_features_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, n_samples: u32, d_features: *mut f32) -> c_int;
    pub fn pt_default_denoise(out: *mut PtDenoise);
    pub fn pt_denoise_device(ctx: *mut PtContext, width: u32, height: u32, d_linear_rgb: *const f32, d_features: *const f32, dn: *const PtDenoise, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_denoised(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32) -> c_int;
    pub fn pt_denoise_var_device(ctx: *mut PtContext, width: u32, height: u32, d_linear_rgb: *const f32, d_features: *const f32, d_var: *const f32, dn: *const PtDenoise, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_adaptive_variance_device(ctx: *mut PtContext, width: u32, height: u32, d_features: *const f32, d_var: *mut f32) -> c_int;
    pub fn pt_render_adaptive_denoised(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, ad: *const PtAdaptive, feature_samples: u32, dn: *const PtDenoise, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_spp: *mut u32, out_rel_err: *mut f32, out_var: *mut f32) -> c_int;
    pub fn pt_default_temporal(out: *mut PtTemporal);
    pub fn pt_temporal_reset(ctx: *mut PtContext) -> c_int;
    pub fn pt_denoise_temporal_device(ctx: *mut PtContext, cam: *const PtCamera, d_linear_rgb: *const f32, d_features: *const f32, dn: *const PtDenoise, tp: *const PtTemporal, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_denoised_temporal(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, tp: *const PtTemporal, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32) -> c_int;
    pub fn pt_scene_update(ctx: *mut PtContext, objs: *const PtObject, n_objs: u32) -> c_int;
    pub fn pt_scene_refit(ctx: *mut PtContext, objs: *const PtObject, n_objs: u32) -> c_int;
    pub fn pt_scene_bvh_cost(ctx: *mut PtContext, cost_now: *mut f64, cost_at_build: *mut f64, refits: *mut u32) -> c_int;
    pub fn pt_scene_rebuild(ctx: *mut PtContext, objs: *const PtObject, n_objs: u32) -> c_int;
    pub fn pt_scene_rebuild_ordered(ctx: *mut PtContext, objs: *const PtObject, n_objs: u32, order: u32) -> c_int;
    pub fn pt_debug_motion_maps(prev_objs: *const PtObject, cur_objs: *const PtObject, n: u32, out_maps: *mut f64, out_flags: *mut u32) -> c_int;
    pub fn pt_render_feature_ids_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, d_ids: *mut i32) -> c_int;
    pub fn pt_denoise_temporal_motion_device(ctx: *mut PtContext, cam: *const PtCamera, d_linear_rgb: *const f32, d_features: *const f32, d_ids: *const i32, dn: *const PtDenoise, tp: *const PtTemporal, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_denoised_motion(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, tp: *const PtTemporal, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32, out_ids: *mut i32) -> c_int;
    pub fn pt_default_tonemap(out: *mut PtTonemap);
    pub fn pt_film_histogram_device(ctx: *mut PtContext, width: u32, height: u32, d_linear_rgb: *const f32, d_hist258: *mut u32) -> c_int;
    pub fn pt_tonemap_device(ctx: *mut PtContext, width: u32, height: u32, d_linear_rgb: *const f32, tm: *const PtTonemap, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_tonemap_host(ctx: *mut PtContext, width: u32, height: u32, linear_rgb: *const f32, tm: *const PtTonemap, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_exposure_reset(ctx: *mut PtContext) -> c_int;
    pub fn pt_exposure_get(ctx: *mut PtContext, log2e: *mut f64, hist258: *mut u32) -> c_int;
    pub fn pt_debug_exposure_state(ctx: *mut PtContext, log2e: *mut f64, e: *mut f32, valid: *mut u32, hist258: *mut u32) -> c_int;
    pub fn pt_debug_tonemap_bin(lum: f32) -> u32;
    pub fn pt_debug_tonemap_meter(hist258: *const u32, tm: *const PtTonemap, fresh: c_int, log2e_prev: f64) -> f64;
    pub fn pt_debug_tonemap_pixel(tm: *const PtTonemap, e: f32, rgb: *const f32, out_y: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_default_upsample(out: *mut PtUpsample);
    pub fn pt_upsample_device(ctx: *mut PtContext, lo_width: u32, lo_height: u32, d_lo_linear: *const f32, d_lo_features: *const f32, width: u32, height: u32, d_features: *const f32, up: *const PtUpsample, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_upsample_host(lo_width: u32, lo_height: u32, lo_linear: *const f32, lo_features: *const f32, width: u32, height: u32, features: *const f32, up: *const PtUpsample, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_denoised_upsampled(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, lo_width: u32, lo_height: u32, feature_samples: u32, dn: *const PtDenoise, up: *const PtUpsample, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_lo_linear: *mut f32, out_features: *mut f32) -> c_int;
    pub fn pt_default_lens(out: *mut PtLens);
    pub fn pt_render_lens_device(ctx: *mut PtContext, cam: *const PtCamera, lens: *const PtLens, params: *const PtRenderParams, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_render_lens_host(ctx: *mut PtContext, cam: *const PtCamera, lens: *const PtLens, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_features_lens_device(ctx: *mut PtContext, cam: *const PtCamera, lens: *const PtLens, params: *const PtRenderParams, n_samples: u32, d_features: *mut f32) -> c_int;
    pub fn pt_render_lens_denoised(ctx: *mut PtContext, cam: *const PtCamera, lens: *const PtLens, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32) -> c_int;
    pub fn pt_debug_lens_rays(ctx: *mut PtContext, cam: *const PtCamera, lens: *const PtLens, xys: *const u32, n: u32, exact_math: u32, out8: *mut f32) -> c_int;
    pub fn pt_debug_lens_setup(cam: *const PtCamera, lens: *const PtLens, out7: *mut f32) -> c_int;
    pub fn pt_default_projection(out: *mut PtProjection);
    pub fn pt_render_projection_device(ctx: *mut PtContext, cam: *const PtCamera, proj: *const PtProjection, params: *const PtRenderParams, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_render_projection_host(ctx: *mut PtContext, cam: *const PtCamera, proj: *const PtProjection, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_features_projection_device(ctx: *mut PtContext, cam: *const PtCamera, proj: *const PtProjection, params: *const PtRenderParams, n_samples: u32, d_features: *mut f32) -> c_int;
    pub fn pt_render_projection_denoised(ctx: *mut PtContext, cam: *const PtCamera, proj: *const PtProjection, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32) -> c_int;
    pub fn pt_render_rays_device(ctx: *mut PtContext, width: u32, height: u32, params: *const PtRenderParams, d_rays6: *const f32, d_weights3: *const f32, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_debug_projection_rays(ctx: *mut PtContext, cam: *const PtCamera, proj: *const PtProjection, xys: *const u32, n: u32, exact_math: u32, out8: *mut f32) -> c_int;
    pub fn pt_projection_setup_host(cam: *const PtCamera, proj: *const PtProjection, out11: *mut f32) -> c_int;
    pub fn pt_projection_rays_host(cam: *const PtCamera, proj: *const PtProjection, xys: *const u32, n: u32, out8: *mut f32) -> c_int;
    pub fn pt_bake_lightmap_device(ctx: *mut PtContext, width: u32, height: u32, d_texels6: *const f32, params: *const PtRenderParams, d_linear_rgb: *mut f32, d_rgba8: *mut u8) -> c_int;
    pub fn pt_bake_lightmap_host(ctx: *mut PtContext, width: u32, height: u32, texels6: *const f32, params: *const PtRenderParams, out_linear_rgb: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_bake_probes_device(ctx: *mut PtContext, d_positions3: *const f32, n_probes: u32, rays_per_probe: u32, params: *const PtRenderParams, d_radiance: *mut f32, d_sh27: *mut f32) -> c_int;
    pub fn pt_bake_probes_host(ctx: *mut PtContext, positions3: *const f32, n_probes: u32, rays_per_probe: u32, params: *const PtRenderParams, out_radiance: *mut f32, out_sh27: *mut f32) -> c_int;
    pub fn pt_sh_project_device(ctx: *mut PtContext, n_probes: u32, rays_per_probe: u32, d_radiance: *const f32, d_sh27: *mut f32) -> c_int;
    pub fn pt_sh_project_host(n_probes: u32, rays_per_probe: u32, radiance: *const f32, sh27: *mut f32) -> c_int;
    pub fn pt_sh_irradiance_host(sh27: *const f32, normals3: *const f32, n: u32, out_rgb: *mut f32) -> c_int;
    pub fn pt_debug_bake_rays(ctx: *mut PtContext, kind: u32, width: u32, height: u32, data: *const f32, xys: *const u32, n: u32, exact_math: u32, out6: *mut f32) -> c_int;
    pub fn pt_bake_rays_host(kind: u32, width: u32, height: u32, data: *const f32, xys: *const u32, n: u32, out6: *mut f32) -> c_int;
    pub fn pt_default_probe_shade(out: *mut PtProbeShade);
    pub fn pt_probe_grid_count(grid: *const PtProbeGrid) -> u32;
    pub fn pt_probe_grid_positions_host(grid: *const PtProbeGrid, out_positions3: *mut f32) -> c_int;
    pub fn pt_probe_grid_bake_device(ctx: *mut PtContext, grid: *const PtProbeGrid, rays_per_probe: u32, params: *const PtRenderParams, d_sh27: *mut f32) -> c_int;
    pub fn pt_probe_shade_device(ctx: *mut PtContext, cam: *const PtCamera, grid: *const PtProbeGrid, d_sh27: *const f32, d_features: *const f32, d_fallback_linear: *const f32, shade: *const PtProbeShade, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_probe_shade_host(cam: *const PtCamera, grid: *const PtProbeGrid, sh27: *const f32, features: *const f32, fallback_linear: *const f32, shade: *const PtProbeShade, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_probe_lit_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, grid: *const PtProbeGrid, d_sh27: *const f32, d_fallback_linear: *const f32, shade: *const PtProbeShade, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_probe_lit_host(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, grid: *const PtProbeGrid, sh27: *const f32, fallback_linear: *const f32, shade: *const PtProbeShade, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_debug_probe_positions(ctx: *mut PtContext, grid: *const PtProbeGrid, out_positions3: *mut f32) -> c_int;
    pub fn pt_default_probe_visibility(grid: *const PtProbeGrid, out: *mut PtProbeVisibility);
    pub fn pt_probe_distances_device(ctx: *mut PtContext, d_positions3: *const f32, n_probes: u32, rays_per_probe: u32, params: *const PtRenderParams, d_distances: *mut f32) -> c_int;
    pub fn pt_probe_distances_host(ctx: *mut PtContext, positions3: *const f32, n_probes: u32, rays_per_probe: u32, params: *const PtRenderParams, out_distances: *mut f32) -> c_int;
    pub fn pt_probe_moments_device(ctx: *mut PtContext, d_distances: *const f32, n_probes: u32, rays_per_probe: u32, vis: *const PtProbeVisibility, d_moments: *mut f32) -> c_int;
    pub fn pt_probe_moments_host(distances: *const f32, n_probes: u32, rays_per_probe: u32, vis: *const PtProbeVisibility, out_moments: *mut f32) -> c_int;
    pub fn pt_probe_grid_visibility_device(ctx: *mut PtContext, grid: *const PtProbeGrid, rays_per_probe: u32, params: *const PtRenderParams, vis: *const PtProbeVisibility, d_moments: *mut f32) -> c_int;
    pub fn pt_probe_shade_visibility_device(ctx: *mut PtContext, cam: *const PtCamera, grid: *const PtProbeGrid, d_sh27: *const f32, d_moments: *const f32, vis: *const PtProbeVisibility, d_features: *const f32, d_fallback_linear: *const f32, shade: *const PtProbeShade, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_probe_shade_visibility_host(cam: *const PtCamera, grid: *const PtProbeGrid, sh27: *const f32, moments: *const f32, vis: *const PtProbeVisibility, features: *const f32, fallback_linear: *const f32, shade: *const PtProbeShade, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_probe_lit_visibility_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, grid: *const PtProbeGrid, d_sh27: *const f32, d_moments: *const f32, vis: *const PtProbeVisibility, d_fallback_linear: *const f32, shade: *const PtProbeShade, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_probe_lit_visibility_host(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, grid: *const PtProbeGrid, sh27: *const f32, moments: *const f32, vis: *const PtProbeVisibility, fallback_linear: *const f32, shade: *const PtProbeShade, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_probe_rotation(frame: u32, out9: *mut f32);
    pub fn pt_default_probe_update(frame: u32, stride: u32, out: *mut PtProbeUpdate);
    pub fn pt_probe_update_rays_host(grid: *const PtProbeGrid, upd: *const PtProbeUpdate, xys: *const u32, n: u32, out6: *mut f32) -> c_int;
    pub fn pt_debug_probe_update_rays(ctx: *mut PtContext, grid: *const PtProbeGrid, upd: *const PtProbeUpdate, xys: *const u32, n: u32, exact_math: u32, out6: *mut f32) -> c_int;
    pub fn pt_probe_blend_device(ctx: *mut PtContext, n_probes: u32, upd: *const PtProbeUpdate, vis: *const PtProbeVisibility, d_radiance: *const f32, d_distances: *const f32, d_sh27: *mut f32, d_moments: *mut f32, d_age: *mut u32) -> c_int;
    pub fn pt_probe_blend_host(n_probes: u32, upd: *const PtProbeUpdate, vis: *const PtProbeVisibility, radiance: *const f32, distances: *const f32, sh27: *mut f32, moments: *mut f32, age: *mut u32) -> c_int;
    pub fn pt_probe_grid_update_device(ctx: *mut PtContext, grid: *const PtProbeGrid, params: *const PtRenderParams, vis: *const PtProbeVisibility, upd: *const PtProbeUpdate, d_sh27: *mut f32, d_moments: *mut f32, d_age: *mut u32) -> c_int;
    pub fn pt_probe_grid_update_host(ctx: *mut PtContext, grid: *const PtProbeGrid, params: *const PtRenderParams, vis: *const PtProbeVisibility, upd: *const PtProbeUpdate, sh27: *mut f32, moments: *mut f32, age: *mut u32) -> c_int;
    pub fn pt_default_cascade(out: *mut PtCascade);
    pub fn pt_render_cascade_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, cs: *const PtCascade, d_linear_rgb: *mut f32, d_rgba8: *mut u8, d_plain_linear: *mut f32) -> c_int;
    pub fn pt_render_cascade_host(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, cs: *const PtCascade, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_plain_linear: *mut f32, out_layers: *mut f64, out_weights: *mut f32) -> c_int;
    pub fn pt_cascade_samples_device(ctx: *mut PtContext, cs: *const PtCascade, width: u32, height: u32, n: u32, batch: u32, d_samples: *const f32, d_linear_rgb: *mut f32, d_rgba8: *mut u8, d_plain_linear: *mut f32) -> c_int;
    pub fn pt_cascade_host(cs: *const PtCascade, width: u32, height: u32, n: u32, samples: *const f32, out_linear: *mut f32, out_rgba8: *mut u8, out_plain: *mut f32, out_layers: *mut f64, out_weights: *mut f32) -> c_int;
    pub fn pt_debug_cascade_split(cs: *const PtCascade, l: f64, j: *mut u32, w_lo: *mut f64, w_hi: *mut f64) -> c_int;
    pub fn pt_default_bloom(out: *mut PtBloom);
    pub fn pt_bloom_device(ctx: *mut PtContext, width: u32, height: u32, d_linear_rgb: *const f32, bloom: *const PtBloom, d_out_linear: *mut f32) -> c_int;
    pub fn pt_bloom_host(width: u32, height: u32, linear_rgb: *const f32, bloom: *const PtBloom, out_linear: *mut f32) -> c_int;
    pub fn pt_display_device(ctx: *mut PtContext, width: u32, height: u32, d_linear_rgb: *const f32, bloom: *const PtBloom, tm: *const PtTonemap, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_display_host(ctx: *mut PtContext, width: u32, height: u32, linear_rgb: *const f32, bloom: *const PtBloom, tm: *const PtTonemap, out_linear: *mut f32, out_rgba8: *mut u8) -> c_int;
    pub fn pt_debug_bloom_plan(width: u32, height: u32, levels: u32, out_wh: *mut u32, n_levels: *mut u32, first_tail_level: *mut u32) -> c_int;
    pub fn pt_debug_bloom_bright(bloom: *const PtBloom, rgb: *const f32, out_b: *mut f32) -> c_int;
    pub fn pt_debug_bloom_tail(ctx: *mut PtContext, enable: c_int) -> c_int;
    pub fn pt_default_filter(out: *mut PtFilter);
    pub fn pt_render_filtered_device(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, flt: *const PtFilter, d_linear_rgb: *mut f32, d_rgba8: *mut u8, d_plain_linear: *mut f32) -> c_int;
    pub fn pt_render_filtered_host(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, flt: *const PtFilter, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_plain_linear: *mut f32, out_weight_sum: *mut f64) -> c_int;
    pub fn pt_filter_samples_device(ctx: *mut PtContext, flt: *const PtFilter, width: u32, height: u32, n: u32, first_sample: u32, batch: u32, d_samples: *const f32, d_linear_rgb: *mut f32, d_rgba8: *mut u8, d_plain_linear: *mut f32, d_weight_sum: *mut f64) -> c_int;
    pub fn pt_filter_host(flt: *const PtFilter, width: u32, height: u32, n: u32, first_sample: u32, samples: *const f32, out_linear: *mut f32, out_rgba8: *mut u8, out_plain: *mut f32, out_weight_sum: *mut f64) -> c_int;
    pub fn pt_debug_filter_weight(flt: *const PtFilter, t: f64, f: *mut f64) -> c_int;
    pub fn pt_debug_filter_offsets(x: u32, y: u32, sample: u32, ox: *mut f64, oy: *mut f64) -> c_int;
    pub fn pt_debug_filter_exp_neg(e: f64, out: *mut f64) -> c_int;
    pub fn pt_default_gradient(out: *mut PtGradient);
    pub fn pt_temporal_gradient_device(ctx: *mut PtContext, cam: *const PtCamera, prev_params: *const PtRenderParams, seed: u32, d_prev_linear: *const f32, g: *const PtGradient, alpha_min: f32, d_alpha: *mut f32) -> c_int;
    pub fn pt_debug_gradient_strata(ctx: *mut PtContext, width: u32, height: u32, out_xy: *mut u32, out_film: *mut f32, out_rec: *mut f64) -> c_int;
    pub fn pt_denoise_temporal_alpha_device(ctx: *mut PtContext, cam: *const PtCamera, d_linear_rgb: *const f32, d_features: *const f32, d_ids: *const i32, d_alpha: *const f32, dn: *const PtDenoise, tp: *const PtTemporal, d_out_linear: *mut f32, d_out_rgba8: *mut u8) -> c_int;
    pub fn pt_render_denoised_gradient(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, tp: *const PtTemporal, g: *const PtGradient, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32, out_ids: *mut i32, out_alpha: *mut f32) -> c_int;
    pub fn pt_temporal_gradient_camera_device(ctx: *mut PtContext, cam: *const PtCamera, prev_cam: *const PtCamera, prev_params: *const PtRenderParams, seed: u32, d_prev_linear: *const f32, d_features: *const f32, g: *const PtGradient, alpha_min: f32, d_alpha: *mut f32) -> c_int;
    pub fn pt_render_denoised_gradient_camera(ctx: *mut PtContext, cam: *const PtCamera, params: *const PtRenderParams, feature_samples: u32, dn: *const PtDenoise, tp: *const PtTemporal, g: *const PtGradient, out_linear_rgb: *mut f32, out_rgba8: *mut u8, out_noisy_linear: *mut f32, out_features: *mut f32, out_ids: *mut i32, out_alpha: *mut f32) -> c_int;
    pub fn pt_ray_color(ctx: *mut PtContext, params: *const PtRenderParams, rays: *const f64, xy: *const u32, n: u32, out_rgb: *mut f32) -> c_int;
    pub fn pt_debug_hit_scene(ctx: *mut PtContext, rays: *const f64, n: u32, t_min: f64, t_max: f64, exact_math: u32, accel: u32, out_id: *mut i32, out_t: *mut f32) -> c_int;
    pub fn pt_debug_hit_records(ctx: *mut PtContext, rays: *const f64, n: u32, t_min: f64, t_max: f64, exact_math: u32, accel: u32, out_id: *mut i32, out_rec: *mut f32) -> c_int;
    pub fn pt_debug_bsdf_eval(ctx: *mut PtContext, obj: u32, in10: *const f64, n: u32, exact_math: u32, out4: *mut f32) -> c_int;
    pub fn pt_debug_bsdf_sample(ctx: *mut PtContext, obj: u32, in7: *const f64, words4: *const u32, n: u32, exact_math: u32, out8: *mut f32) -> c_int;
    pub fn pt_debug_shape_sample(ctx: *mut PtContext, obj: u32, from3: *const f64, target3: *const f64, r12: *const f64, n: u32, exact_math: u32, out8: *mut f32) -> c_int;
    pub fn pt_debug_light_point(ctx: *mut PtContext, from3: *const f64, words4: *const u32, n: u32, exact_math: u32, out8: *mut f32) -> c_int;
    pub fn pt_debug_camera_rays(ctx: *mut PtContext, cam: *const PtCamera, xys: *const u32, n: u32, exact_math: u32, out8: *mut f32) -> c_int;
    pub fn pt_debug_joint_scan(ctx: *mut PtContext, rays10: *const f64, n: u32, t_min: f64, t_max_b: f64, exact_math: u32, out6: *mut f32) -> c_int;
    pub fn pt_debug_bvh_check(objs: *const PtObject, n_objs: u32, depth: *mut u32, n_nodes: *mut u32, n_leaf_slots: *mut u32) -> c_int;
    pub fn pt_debug_bvh_refit_check(prev_objs: *const PtObject, cur_objs: *const PtObject, n_objs: u32, refit: u32, out_qnodes: *mut u32, cap_nodes: u32, out_leaf_rec: *mut f32, out_leaf_lead: *mut f32, out_leaf_ids: *mut u32, cap_slots: u32, n_nodes: *mut u32, n_slots: *mut u32, out_grid: *mut f32, root: *mut u32, cost_now: *mut u64, cost_at_build: *mut u64) -> c_int;
    pub fn pt_debug_bvh_morton_check(objs: *const PtObject, refit_objs: *const PtObject, n_objs: u32, out_qnodes: *mut u32, cap_nodes: u32, out_leaf_rec: *mut f32, out_leaf_lead: *mut f32, out_leaf_ids: *mut u32, cap_slots: u32, n_nodes: *mut u32, n_slots: *mut u32, out_grid: *mut f32, root: *mut u32, cost_now: *mut u64, out_keys: *mut u32, out_order: *mut u32, cap_objs: u32) -> c_int;
    pub fn pt_debug_bvh_median_check(objs: *const PtObject, refit_objs: *const PtObject, n_objs: u32, out_qnodes: *mut u32, cap_nodes: u32, out_leaf_rec: *mut f32, out_leaf_lead: *mut f32, out_leaf_ids: *mut u32, cap_slots: u32, n_nodes: *mut u32, n_slots: *mut u32, out_grid: *mut f32, root: *mut u32, cost_now: *mut u64, out_keys: *mut u32, out_order: *mut u32, cap_objs: u32) -> c_int;
    pub fn pt_debug_bvh_median_plan(n_objs: u32, out_steps: *mut u32, cap_steps: u32, n_steps: *mut u32, tile: *mut u32) -> c_int;
    pub fn pt_debug_bvh_morton_topology(n_objs: u32, out_codes: *mut u32, out_height: *mut u32, out_order: *mut u32, cap_nodes: u32, out_height_first: *mut u32, cap_heights: u32, n_nodes: *mut u32, n_heights: *mut u32, n_slots: *mut u32, root: *mut u32, stack_need: *mut u32, depth: *mut u32) -> c_int;
    pub fn pt_debug_bvh_read(ctx: *mut PtContext, out_qnodes: *mut u32, cap_nodes: u32, out_leaf_rec: *mut f32, out_leaf_lead: *mut f32, out_leaf_ids: *mut u32, cap_slots: u32, n_nodes: *mut u32, n_slots: *mut u32, out_grid: *mut f32, root: *mut u32, cost_now: *mut u64) -> c_int;
    pub fn pt_last_error() -> *const c_char;
    pub fn pt_abi_version() -> u32;
}
