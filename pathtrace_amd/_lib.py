"""ctypes binding of the C ABI declared in include/pathtrace_amd.h.

This is the same binding a foreign-language host would write (see INTEGRATION.md
for the Rust `extern "C"` form).  Loading fails loudly when the shared library is
missing: there is no Python or CPU fallback for the rendering path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PATHTRACE_AMD_LIB: alternative build of the same library (A/B experiments of kernel variants)
LIB_PATH = os.environ.get("PATHTRACE_AMD_LIB") or os.path.join(_HERE, "libpathtrace_amd.so")


class PtCamera(C.Structure):
    _fields_ = [
        ("origin", C.c_double * 3),
        ("lower_left", C.c_double * 3),
        ("horizontal", C.c_double * 3),
        ("vertical", C.c_double * 3),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
    ]


class PtObject(C.Structure):
    _fields_ = [
        ("shape_tag", C.c_uint32),
        ("mat_tag", C.c_uint32),
        ("shape", C.c_double * 9),
        ("mat", C.c_double * 6),
    ]


class PtRenderParams(C.Structure):
    _fields_ = [
        ("spp", C.c_uint32),
        ("spp_offset", C.c_uint32),
        ("min_depth", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("integrator", C.c_uint32),
        ("t_min", C.c_double),
        ("band_rows", C.c_uint32),
        ("band_index", C.c_uint32),
        ("band_count", C.c_uint32),
        ("max_paths_in_flight", C.c_uint64),
        ("profile", C.c_uint32),
        ("workgroups", C.c_uint32),
        ("exact_math", C.c_uint32),
        ("accel", C.c_uint32),
        ("n_devices", C.c_uint32),
    ]


class PtTuning(C.Structure):
    _fields_ = [
        ("export_below", C.c_uint32),
        ("bvh_refill", C.c_uint32),
        ("bvh_leaf", C.c_uint32),
        ("cont_workgroups", C.c_uint32),
        ("level0_form", C.c_uint32),
        ("regen_workgroups", C.c_uint32),
        ("in_order", C.c_uint32),
    ]


class PtStats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64),
        ("vertices", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("bounce_launches", C.c_uint32),
        ("batches", C.c_uint32),
        ("max_depth_reached", C.c_uint32),
        ("reserved", C.c_uint32),
        ("bounce_kernel_ms", C.c_double),
        ("total_ms", C.c_double),
        ("primary_vertices", C.c_uint64),
        ("primary_kernel_ms", C.c_double),
        ("primary_launches", C.c_uint32),
        ("reserved2", C.c_uint32),
        ("samples_expected", C.c_uint64),
    ]


class PtAdaptive(C.Structure):
    _fields_ = [
        ("spp_min", C.c_uint32),
        ("spp_step", C.c_uint32),
        ("rel_tol", C.c_double),
        ("abs_floor", C.c_double),
    ]


class PtDenoise(C.Structure):
    _fields_ = [
        ("iterations", C.c_uint32),
        ("sigma_l", C.c_float),
        ("sigma_n", C.c_float),
        ("sigma_d", C.c_float),
    ]


class PtTemporal(C.Structure):
    _fields_ = [
        ("alpha", C.c_float),
        ("depth_tol", C.c_float),
        ("normal_tol", C.c_float),
    ]


class PtGradient(C.Structure):
    _fields_ = [
        ("radius", C.c_uint32),
        ("scale", C.c_float),
    ]


class PtTonemap(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32),
        ("curve", C.c_uint32),
        ("transfer", C.c_uint32),
        ("ev", C.c_float),
        ("key", C.c_float),
        ("pct_lo", C.c_float),
        ("pct_hi", C.c_float),
        ("log2_min", C.c_float),
        ("log2_max", C.c_float),
        ("adapt", C.c_float),
        ("white", C.c_float),
    ]


class PtBloom(C.Structure):
    _fields_ = [
        ("levels", C.c_uint32),
        ("threshold", C.c_float),
        ("knee", C.c_float),
        ("clamp", C.c_float),
        ("scatter", C.c_float),
        ("intensity", C.c_float),
    ]


class PtUpsample(C.Structure):
    _fields_ = [
        ("sigma_n", C.c_float),
        ("sigma_d", C.c_float),
    ]


class PtLens(C.Structure):
    _fields_ = [
        ("aperture", C.c_double),
        ("focus_distance", C.c_double),
    ]


class PtProjection(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("reserved", C.c_uint32),
        ("fov_degrees", C.c_double),
    ]


PT_PROJ_PERSPECTIVE, PT_PROJ_ORTHOGRAPHIC, PT_PROJ_FISHEYE, PT_PROJ_EQUIRECT = 0, 1, 2, 3
PT_BAKE_TEXELS, PT_BAKE_PROBES = 0, 1


class PtProbeGrid(C.Structure):
    _fields_ = [
        ("origin", C.c_double * 3),
        ("spacing", C.c_double * 3),
        ("counts", C.c_uint32 * 3),
        ("reserved", C.c_uint32),
    ]


class PtProbeShade(C.Structure):
    _fields_ = [
        ("normal_bias", C.c_float),
        ("weight", C.c_uint32),
    ]


PT_PROBE_WEIGHT_TRILINEAR, PT_PROBE_WEIGHT_FACING = 0, 1


class PtProbeVisibility(C.Structure):
    _fields_ = [
        ("resolution", C.c_uint32),
        ("sharpness_log2", C.c_uint32),
        ("max_distance", C.c_float),
        ("reserved", C.c_uint32),
    ]


class PtProbeUpdate(C.Structure):
    _fields_ = [
        ("rays_per_probe", C.c_uint32),
        ("first", C.c_uint32),
        ("stride", C.c_uint32),
        ("hysteresis", C.c_float),
        ("change_threshold", C.c_float),
        ("change_alpha", C.c_float),
        ("rotation", C.c_float * 9),
        ("reserved", C.c_uint32),
    ]


class PtCascade(C.Structure):
    _fields_ = [
        ("layers", C.c_uint32),
        ("start", C.c_float),
        ("base", C.c_float),
        ("kappa", C.c_float),
    ]


class PtFilter(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("radius", C.c_float),
        ("a", C.c_float),
        ("b", C.c_float),
    ]


FILTER_BOX, FILTER_TENT, FILTER_GAUSSIAN, FILTER_MITCHELL = 0, 1, 2, 3


class PtSchedJob(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_batches", "regen", "split", "hand_off", "regen_export", "profile", "in_order", "capturing",
                                          "grid", "regen_grid", "cont_grid", "regen_capacity", "fixed_grid", "counter_words")] + [("xchg_need", C.c_uint64)]


class PtSchedOp(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("kind", "stream", "event", "pool", "set", "lane", "level", "own_queue", "ovf_par", "batch", "grid",
                                          "seq", "core", "flags", "zero_words", "reserved")] + [("xchg_off", C.c_uint64), ("xchg_len", C.c_uint64)]


class PtShapeIn(C.Structure):
    _fields_ = [("np", C.c_uint64), ("max_paths_in_flight", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "spp", "workgroups", "accel", "profile", "list", "list_regen", "inject", "n_objs", "blob_f4", "diffuse_only", "split_ok", "n_cus",
        "export_below", "cont_workgroups", "level0_form", "regen_workgroups", "in_order", "capturing", "inject_spp", "reserved")]


class PtShapeOut(C.Structure):
    _fields_ = ([(n, C.c_uint32) for n in ("lds_job", "split", "regen_scene", "over_cap")] +
                [(n, C.c_uint64) for n in ("cap", "n_paths_max", "ovf_slots", "q_slots_cont", "q_slots")] +
                [(n, C.c_uint32) for n in ("np", "spp", "nb_max", "n_batches", "export_small", "paths_per_wave", "small_scene", "hand_off", "regen",
                                           "overlap", "grid", "nw", "seg_cap", "regen_per_cu", "regen_capacity", "regen_grid", "regen_launch_grid",
                                           "cont_grid", "nw_cont", "seg_cap_cont", "regen_export", "reserved")] + [("job", PtSchedJob)])


class PtShapeLaunch(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("s0", "nb", "n_first", "seg_cap", "src_mode", "export_below", "regen_static", "reserved")]


class PtMultiInfo(C.Structure):
    _fields_ = [
        ("n_devices", C.c_uint32),
        ("comm_count", C.c_uint32),
        ("rccl_version", C.c_uint32),
        ("threaded", C.c_uint32),
        ("frames", C.c_uint64),
        ("enqueue_us_sum", C.c_double),
        ("enqueue_us_max", C.c_double),
        ("exchange", C.c_uint32),
        ("reserved_", C.c_uint32),
    ]


PT_EXCHANGE_RCCL, PT_EXCHANGE_COPY = 0, 1
PT_SHAPE_SPHERE, PT_SHAPE_TRIANGLE = 0, 1
PT_MAT_LAMBERT, PT_MAT_EMISSIVE, PT_MAT_MIRROR, PT_MAT_OREN_NAYAR = 0, 1, 2, 3
PT_INTEGRATOR_MIS, PT_INTEGRATOR_BRDF_ONLY = 0, 1
PT_EXPOSURE_AUTO, PT_EXPOSURE_MANUAL = 0, 1
PT_CURVE_CLAMP, PT_CURVE_REINHARD, PT_CURVE_ACES = 0, 1, 2
PT_TRANSFER_SQRT, PT_TRANSFER_SRGB = 0, 1
PT_STREAM_LEGACY_DEFAULT = 1      # pt_context_set_stream: HIP's legacy default stream (handle 0 means "the context's own")

# every symbol include/pathtrace_amd.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "pt_camera_new": (C.c_int, [_P(C.c_double), C.c_uint32, C.c_uint32, C.c_double, C.c_double, _P(PtCamera)]),
    "pt_camera_look_at": (C.c_int, [_P(C.c_double), _P(C.c_double), _P(C.c_double), C.c_uint32, C.c_uint32,
                                    C.c_double, _P(PtCamera)]),
    "pt_default_params": (None, [_P(PtRenderParams)]),
    "pt_tile_rows": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "pt_builtin_scene": (C.c_int, [C.c_uint32, C.c_uint32, _P(PtObject), C.c_uint32, _P(C.c_uint32)]),
    "pt_context_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "pt_context_destroy": (C.c_int, [C.c_void_p]),
    "pt_context_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pt_context_set_tuning": (C.c_int, [C.c_void_p, _P(PtTuning)]),
    "pt_scene_upload": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32]),
    "pt_render_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_device_packed": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_void_p]),
    "pt_sync": (C.c_int, [C.c_void_p]),
    "pt_get_stats": (C.c_int, [C.c_void_p, _P(PtStats)]),
    "pt_debug_raw_stats": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "pt_debug_scan_layout": (C.c_int, [C.c_void_p, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_debug_spheres_only": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32, _P(C.c_uint32)]),
    "pt_debug_lambert_surfaces": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32, _P(C.c_uint32)]),
    "pt_render_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_progressive": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_render": (C.c_int, [_P(PtCamera), _P(PtObject), C.c_uint32, _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_debug_hit_scene": (C.c_int, [C.c_void_p, _P(C.c_double), C.c_uint32, C.c_double, C.c_double, C.c_uint32,
                                     C.c_uint32, _P(C.c_int32), _P(C.c_float)]),
    "pt_debug_hit_records": (C.c_int, [C.c_void_p, _P(C.c_double), C.c_uint32, C.c_double, C.c_double, C.c_uint32,
                                       C.c_uint32, _P(C.c_int32), _P(C.c_float)]),
    "pt_debug_bsdf_eval": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_double), C.c_uint32, C.c_uint32, _P(C.c_float)]),
    "pt_debug_bsdf_sample": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_double), _P(C.c_uint32), C.c_uint32, C.c_uint32,
                                       _P(C.c_float)]),
    "pt_debug_shape_sample": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_double), _P(C.c_double), _P(C.c_double), C.c_uint32,
                                        C.c_uint32, _P(C.c_float)]),
    "pt_debug_light_point": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_uint32), C.c_uint32, C.c_uint32, _P(C.c_float)]),
    "pt_debug_camera_rays": (C.c_int, [C.c_void_p, _P(PtCamera), _P(C.c_uint32), C.c_uint32, C.c_uint32, _P(C.c_float)]),
    "pt_debug_joint_scan": (C.c_int, [C.c_void_p, _P(C.c_double), C.c_uint32, C.c_double, C.c_double, C.c_uint32, _P(C.c_float)]),
    "pt_debug_bvh_check": (C.c_int, [_P(PtObject), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_render_pixels": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(C.c_uint32), C.c_uint32, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "pt_render_adaptive": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(PtAdaptive), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "pt_render_features_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, C.c_void_p]),
    "pt_default_denoise": (None, [_P(PtDenoise)]),
    "pt_denoise_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, _P(PtDenoise), C.c_void_p, C.c_void_p]),
    "pt_render_denoised": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "pt_denoise_var_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, _P(PtDenoise), C.c_void_p,
                                        C.c_void_p]),
    "pt_adaptive_variance_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pt_render_adaptive_denoised": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(PtAdaptive), C.c_uint32, _P(PtDenoise),
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_default_temporal": (None, [_P(PtTemporal)]),
    "pt_temporal_reset": (C.c_int, [C.c_void_p]),
    "pt_denoise_temporal_device": (C.c_int, [C.c_void_p, _P(PtCamera), C.c_void_p, C.c_void_p, _P(PtDenoise), _P(PtTemporal), C.c_void_p,
                                             C.c_void_p]),
    "pt_render_denoised_temporal": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), _P(PtTemporal),
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_scene_update": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32]),
    "pt_scene_refit": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32]),
    "pt_scene_bvh_cost": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_double), _P(C.c_uint32)]),
    "pt_scene_rebuild": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32]),
    "pt_scene_rebuild_ordered": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32, C.c_uint32]),
    "pt_debug_bvh_median_check": (C.c_int, [_P(PtObject), _P(PtObject), C.c_uint32, _P(C.c_uint32), C.c_uint32, _P(C.c_float), _P(C.c_float), _P(C.c_uint32),
                                            C.c_uint32, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_float), _P(C.c_uint32), _P(C.c_uint64),
                                            _P(C.c_uint32), _P(C.c_uint32), C.c_uint32]),
    "pt_debug_bvh_median_plan": (C.c_int, [C.c_uint32, _P(C.c_uint32), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_debug_bvh_morton_check": (C.c_int, [_P(PtObject), _P(PtObject), C.c_uint32, _P(C.c_uint32), C.c_uint32, _P(C.c_float), _P(C.c_float), _P(C.c_uint32),
                                            C.c_uint32, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_float), _P(C.c_uint32), _P(C.c_uint64),
                                            _P(C.c_uint32), _P(C.c_uint32), C.c_uint32]),
    "pt_debug_bvh_morton_topology": (C.c_int, [C.c_uint32, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), C.c_uint32, _P(C.c_uint32), C.c_uint32,
                                               _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_debug_bvh_refit_check": (C.c_int, [_P(PtObject), _P(PtObject), C.c_uint32, C.c_uint32, _P(C.c_uint32), C.c_uint32, _P(C.c_float), _P(C.c_float),
                                           _P(C.c_uint32), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_float), _P(C.c_uint32),
                                           _P(C.c_uint64), _P(C.c_uint64)]),
    "pt_debug_bvh_read": (C.c_int, [C.c_void_p, _P(C.c_uint32), C.c_uint32, _P(C.c_float), _P(C.c_float), _P(C.c_uint32), C.c_uint32,
                                    _P(C.c_uint32), _P(C.c_uint32), _P(C.c_float), _P(C.c_uint32), _P(C.c_uint64)]),
    "pt_debug_motion_maps": (C.c_int, [_P(PtObject), _P(PtObject), C.c_uint32, _P(C.c_double), _P(C.c_uint32)]),
    "pt_render_feature_ids_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_void_p]),
    "pt_denoise_temporal_motion_device": (C.c_int, [C.c_void_p, _P(PtCamera), C.c_void_p, C.c_void_p, C.c_void_p, _P(PtDenoise),
                                                    _P(PtTemporal), C.c_void_p, C.c_void_p]),
    "pt_render_denoised_motion": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), _P(PtTemporal),
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_default_gradient": (None, [_P(PtGradient)]),
    "pt_temporal_gradient_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, C.c_void_p, _P(PtGradient), C.c_float,
                                              C.c_void_p]),
    "pt_debug_gradient_strata": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_denoise_temporal_alpha_device": (C.c_int, [C.c_void_p, _P(PtCamera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(PtDenoise),
                                                   _P(PtTemporal), C.c_void_p, C.c_void_p]),
    "pt_render_denoised_gradient": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), _P(PtTemporal),
                                              _P(PtGradient), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_temporal_gradient_camera_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtCamera), _P(PtRenderParams), C.c_uint32, C.c_void_p,
                                                     C.c_void_p, _P(PtGradient), C.c_float, C.c_void_p]),
    "pt_render_denoised_gradient_camera": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), _P(PtTemporal),
                                                     _P(PtGradient), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_default_tonemap": (None, [_P(PtTonemap)]),
    "pt_film_histogram_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pt_tonemap_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtTonemap), C.c_void_p, C.c_void_p]),
    "pt_tonemap_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtTonemap), C.c_void_p, C.c_void_p]),
    "pt_exposure_reset": (C.c_int, [C.c_void_p]),
    "pt_exposure_get": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_uint32)]),
    "pt_debug_exposure_state": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_float), _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_debug_tonemap_bin": (C.c_uint32, [C.c_float]),
    "pt_debug_tonemap_meter": (C.c_double, [_P(C.c_uint32), _P(PtTonemap), C.c_int, C.c_double]),
    "pt_debug_tonemap_pixel": (C.c_int, [_P(PtTonemap), C.c_float, _P(C.c_float), _P(C.c_float), _P(C.c_uint8)]),
    "pt_default_lens": (None, [_P(PtLens)]),
    "pt_render_lens_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtLens), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_lens_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtLens), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_features_lens_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtLens), _P(PtRenderParams), C.c_uint32, C.c_void_p]),
    "pt_render_lens_denoised": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtLens), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_debug_lens_rays": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtLens), _P(C.c_uint32), C.c_uint32, C.c_uint32, _P(C.c_float)]),
    "pt_debug_lens_setup": (C.c_int, [_P(PtCamera), _P(PtLens), _P(C.c_float)]),
    "pt_default_projection": (None, [_P(PtProjection)]),
    "pt_render_projection_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProjection), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_projection_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProjection), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_features_projection_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProjection), _P(PtRenderParams), C.c_uint32, C.c_void_p]),
    "pt_render_projection_denoised": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProjection), _P(PtRenderParams), C.c_uint32, _P(PtDenoise), C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_render_rays_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(PtRenderParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_debug_projection_rays": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProjection), _P(C.c_uint32), C.c_uint32, C.c_uint32, _P(C.c_float)]),
    "pt_projection_setup_host": (C.c_int, [_P(PtCamera), _P(PtProjection), _P(C.c_float)]),
    "pt_projection_rays_host": (C.c_int, [_P(PtCamera), _P(PtProjection), _P(C.c_uint32), C.c_uint32, _P(C.c_float)]),
    "pt_bake_lightmap_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_bake_lightmap_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_bake_probes_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_bake_probes_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_sh_project_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pt_sh_project_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pt_sh_irradiance_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pt_debug_bake_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_void_p]),
    "pt_bake_rays_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _P(C.c_uint32), C.c_uint32, C.c_void_p]),
    "pt_default_probe_shade": (None, [_P(PtProbeShade)]),
    "pt_probe_grid_count": (C.c_uint32, [_P(PtProbeGrid)]),
    "pt_probe_grid_positions_host": (C.c_int, [_P(PtProbeGrid), C.c_void_p]),
    "pt_probe_grid_bake_device": (C.c_int, [C.c_void_p, _P(PtProbeGrid), C.c_uint32, _P(PtRenderParams), C.c_void_p]),
    "pt_probe_shade_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, _P(PtProbeShade), C.c_void_p,
                                        C.c_void_p]),
    "pt_probe_shade_host": (C.c_int, [_P(PtCamera), _P(PtProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_render_probe_lit_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtProbeGrid), C.c_void_p, C.c_void_p,
                                             _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_render_probe_lit_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtProbeGrid), C.c_void_p, C.c_void_p,
                                           _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_debug_probe_positions": (C.c_int, [C.c_void_p, _P(PtProbeGrid), C.c_void_p]),
    "pt_default_probe_visibility": (None, [_P(PtProbeGrid), _P(PtProbeVisibility)]),
    "pt_probe_distances_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(PtRenderParams), C.c_void_p]),
    "pt_probe_distances_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(PtRenderParams), C.c_void_p]),
    "pt_probe_moments_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, _P(PtProbeVisibility), C.c_void_p]),
    "pt_probe_moments_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(PtProbeVisibility), C.c_void_p]),
    "pt_probe_grid_visibility_device": (C.c_int, [C.c_void_p, _P(PtProbeGrid), C.c_uint32, _P(PtRenderParams), _P(PtProbeVisibility), C.c_void_p]),
    "pt_probe_shade_visibility_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtProbeGrid), C.c_void_p, C.c_void_p, _P(PtProbeVisibility),
                                                   C.c_void_p, C.c_void_p, _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_probe_shade_visibility_host": (C.c_int, [_P(PtCamera), _P(PtProbeGrid), C.c_void_p, C.c_void_p, _P(PtProbeVisibility), C.c_void_p,
                                                 C.c_void_p, _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_render_probe_lit_visibility_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtProbeGrid), C.c_void_p,
                                                        C.c_void_p, _P(PtProbeVisibility), C.c_void_p, _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_render_probe_lit_visibility_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, _P(PtProbeGrid), C.c_void_p,
                                                      C.c_void_p, _P(PtProbeVisibility), C.c_void_p, _P(PtProbeShade), C.c_void_p, C.c_void_p]),
    "pt_probe_rotation": (None, [C.c_uint32, C.c_void_p]),
    "pt_default_probe_update": (None, [C.c_uint32, C.c_uint32, _P(PtProbeUpdate)]),
    "pt_probe_update_rays_host": (C.c_int, [_P(PtProbeGrid), _P(PtProbeUpdate), C.c_void_p, C.c_uint32, C.c_void_p]),
    "pt_debug_probe_update_rays": (C.c_int, [C.c_void_p, _P(PtProbeGrid), _P(PtProbeUpdate), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "pt_probe_blend_device": (C.c_int, [C.c_void_p, C.c_uint32, _P(PtProbeUpdate), _P(PtProbeVisibility), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "pt_probe_blend_host": (C.c_int, [C.c_uint32, _P(PtProbeUpdate), _P(PtProbeVisibility), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "pt_probe_grid_update_device": (C.c_int, [C.c_void_p, _P(PtProbeGrid), _P(PtRenderParams), _P(PtProbeVisibility), _P(PtProbeUpdate),
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_probe_grid_update_host": (C.c_int, [C.c_void_p, _P(PtProbeGrid), _P(PtRenderParams), _P(PtProbeVisibility), _P(PtProbeUpdate),
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_default_upsample": (None, [_P(PtUpsample)]),
    "pt_upsample_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                     _P(PtUpsample), C.c_void_p, C.c_void_p]),
    "pt_upsample_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtUpsample),
                                   C.c_void_p, C.c_void_p]),
    "pt_render_denoised_upsampled": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_uint32, C.c_uint32, C.c_uint32, _P(PtDenoise),
                                               _P(PtUpsample), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_default_cascade": (None, [_P(PtCascade)]),
    "pt_render_cascade_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(PtCascade), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_render_cascade_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(PtCascade), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "pt_cascade_samples_device": (C.c_int, [C.c_void_p, _P(PtCascade), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "pt_cascade_host": (C.c_int, [_P(PtCascade), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "pt_debug_cascade_split": (C.c_int, [_P(PtCascade), C.c_double, _P(C.c_uint32), _P(C.c_double), _P(C.c_double)]),
    "pt_default_bloom": (None, [_P(PtBloom)]),
    "pt_bloom_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtBloom), C.c_void_p]),
    "pt_bloom_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, _P(PtBloom), C.c_void_p]),
    "pt_display_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtBloom), _P(PtTonemap), C.c_void_p, C.c_void_p]),
    "pt_display_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, _P(PtBloom), _P(PtTonemap), C.c_void_p, C.c_void_p]),
    "pt_debug_bloom_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_debug_bloom_bright": (C.c_int, [_P(PtBloom), C.c_void_p, C.c_void_p]),
    "pt_debug_bloom_tail": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_default_filter": (None, [_P(PtFilter)]),
    "pt_render_filtered_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(PtFilter), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_render_filtered_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), _P(PtFilter), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "pt_filter_samples_device": (C.c_int, [C.c_void_p, _P(PtFilter), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pt_filter_host": (C.c_int, [_P(PtFilter), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "pt_debug_filter_weight": (C.c_int, [_P(PtFilter), C.c_double, _P(C.c_double)]),
    "pt_debug_filter_offsets": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_double), _P(C.c_double)]),
    "pt_debug_filter_exp_neg": (C.c_int, [C.c_double, _P(C.c_double)]),
    "pt_ray_color": (C.c_int, [C.c_void_p, _P(PtRenderParams), _P(C.c_double), _P(C.c_uint32), C.c_uint32, C.c_void_p]),
    "pt_shutdown": (None, []),
    "pt_multi_create": (C.c_int, [_P(C.c_int), C.c_uint32, _P(C.c_void_p)]),
    "pt_multi_destroy": (C.c_int, [C.c_void_p]),
    "pt_multi_device_count": (C.c_uint32, [C.c_void_p]),
    "pt_multi_set_threads": (C.c_int, [C.c_void_p, C.c_int]),
    "pt_multi_set_exchange": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pt_multi_info": (C.c_int, [C.c_void_p, _P(PtMultiInfo)]),
    "pt_debug_multi_create_shared": (C.c_int, [C.c_int, C.c_uint32, _P(C.c_void_p)]),
    "pt_debug_feeder_selftest": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, _P(C.c_uint64), _P(C.c_uint32)]),
    "pt_debug_sched_create": (C.c_int, [_P(C.c_void_p)]),
    "pt_debug_sched_destroy": (None, [C.c_void_p]),
    "pt_debug_sched_render": (C.c_int, [C.c_void_p, _P(PtSchedJob), C.c_uint32, C.c_uint32, _P(PtSchedOp), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "pt_debug_sched_sync": (C.c_int, [C.c_void_p, C.c_uint32]),
    "pt_debug_render_shape": (C.c_int, [_P(PtShapeIn), C.c_uint32, _P(PtShapeOut), _P(PtSchedOp), C.c_uint32, _P(PtShapeLaunch)]),
    "pt_debug_fail_after": (C.c_int, [C.c_void_p, C.c_int64]),
    "pt_debug_launch_log": (C.c_int, [C.c_void_p, _P(C.c_uint32), C.c_uint32, _P(C.c_uint32)]),
    "pt_debug_path_instances": (C.c_int, [_P(C.c_uint32), C.c_uint32, _P(C.c_uint32)]),
    "pt_multi_scene_upload": (C.c_int, [C.c_void_p, _P(PtObject), C.c_uint32]),
    "pt_multi_set_tuning": (C.c_int, [C.c_void_p, _P(PtTuning)]),
    "pt_multi_render_device": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_multi_sync": (C.c_int, [C.c_void_p]),
    "pt_multi_get_stats": (C.c_int, [C.c_void_p, _P(PtStats)]),
    "pt_multi_render_host": (C.c_int, [C.c_void_p, _P(PtCamera), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_film_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "pt_film_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "pt_debug_multi_emulate": (C.c_int, [C.c_void_p, C.c_uint32, _P(PtCamera), _P(PtRenderParams), C.c_void_p, C.c_void_p]),
    "pt_render_multi": (C.c_int, [_P(C.c_int), C.c_uint32, _P(PtCamera), _P(PtObject), C.c_uint32, _P(PtRenderParams),
                                  C.c_void_p, C.c_void_p]),
    "pt_last_error": (C.c_char_p, []),
    "pt_abi_version": (C.c_uint32, []),
}

PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.POINTER(C.c_float))

_lib = None


def lib():
    """Load libpathtrace_amd.so (built by `__graft_entry__.build()` / csrc/Makefile)."""
    global _lib
    if _lib is None:
        # torch ships its own libamdhip64.so with the same SONAME as /opt/rocm's.  A process must
        # run ONE HIP runtime: load torch's first so that this library binds to it too (device
        # pointers and streams are exchanged with torch).  Without torch the system runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP library first "
                "(python -c 'import __graft_entry__ as g; g.build()').  There is no fallback path.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(h, name)   # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pathtrace_amd error {code}: {msg}")
        self.code = code


def check(code):
    if code != 0:
        raise PtError(code, lib().pt_last_error().decode("utf-8", "replace"))
