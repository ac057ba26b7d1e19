"""pathtrace_amd -- MI355X-native wavefront path tracer behind a C ABI.

Drop-in for the per-pixel rendering hot path of roxas1533/pathtrace
(src/rendering.rs and what it calls).  The product is libpathtrace_amd.so
(pathtrace_amd/csrc); this package is the ctypes harness tests and bench use.
"""
from . import _lib, api  # noqa: F401
from .api import (Context, Multi, bake_rays_host, probe_directions, sh_irradiance, sh_project_host, bloom_bright, bloom_host, bloom_plan, builtin_scene, default_bloom, bvh_check, bvh_cost_value, bvh_median_check, bvh_median_plan, bvh_morton_check, bvh_morton_topology, bvh_refit_check, camera_look_at, camera_new, cascade_host, cascade_split, default_cascade, default_denoise, default_filter, default_gradient, default_lens, default_params, default_projection, default_temporal, default_tonemap, default_upsample, make_objects, motion_maps,  # noqa: F401
                  filter_exp_neg, filter_host, filter_offsets, filter_weight, lens_setup, projection_rays_host, projection_setup, path_instance, path_instances, default_probe_shade, probe_grid, probe_grid_count, probe_grid_positions, probe_shade_host, default_probe_visibility, probe_moments_host, probe_shade_visibility_host, default_probe_update, probe_blend_host, probe_rotation, probe_update_rays_host, probe_update_slots, render_host, render_multi, scene_lambert_surfaces, scene_spheres_only, tile_rows, tile_row_indices, upsample_host)
