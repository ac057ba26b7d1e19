// pt_kernels_unit.h -- the first include of every kernel translation unit (pt_kernels_*.hip).
//
// The kernels are built as one translation unit per group, each with the compiler options its kernels measured best with
// (Makefile: KFLAGS_*; profiles/r05/ab_noslp.txt, ab_bvh_slp.txt, ab_compiler_flags2.txt), and each but the last once per
// arithmetic mode (PT_MATH_EXACT, pt_device.h):
//   pt_kernels_main.hip   k_paths, k_paths_regen, the debug / setup kernels               -fno-slp-vectorize (C2 launch -2.6 %)
//   pt_kernels_rays.hip   the ray sources beside the pinhole camera (k_source_paths,      the main unit's options
//                         k_source_feature_rays, k_debug_source_rays), k_feature_resolve
//   pt_kernels_split.hip  k_paths_regen_split                                             -fno-slp-vectorize, scheduling strategy max-ilp (C1 -1.2 %; C2 would pay 1.6 %)
//   pt_kernels_bvh.hip    the BVH form (k_paths_bvh, k_debug_hit_bvh)                     with the SLP vectoriser (its 4-wide box tests pack well: +2 % without)
//   pt_kernels_film.hip   the kernels on the film and the device-side BVH refit / builds  the main unit's options
//                         (fast mode only), one header per concern: pt_film_exchange.h, _adaptive.h, _denoise.h, _temporal.h
//                         (accumulation and gradients), _bvh.h, _tonemap.h, _upsample.h, _cascade.h, _filter.h, _bloom.h,
//                         _bake.h, _probe.h (k_probe_positions, k_probe_shade), _probe_vis.h (k_probe_distances, k_probe_moments, k_probe_shade_vis),
//                         _probe_update.h (k_probe_update)
// Shared device code: pt_kernels_scan.h (primitive tests, scene staging, scans), pt_kernels_vertex.h (one path vertex).
// Kernel templates are instantiated where their launcher is; the launchers that cross units are declared in pt_kernels.h.
#pragma once
#include "pt_device.h"
#include "pt_kernels.h"

using namespace PTD_NS;
using namespace ptk;

// namespace of a unit's kernels and the suffix of its launchers: one copy of every kernel per arithmetic mode
#if PT_MATH_EXACT
#define PTK_IMPL ptk_exact_impl
#define PT_LAUNCH(name) name##_exact
#else
#define PTK_IMPL ptk_fast_impl
#define PT_LAUNCH(name) name##_fast
#endif
namespace PTK_IMPL {
// (the instance codes the launchers return carry the mode: pt_kernels.h)
constexpr bool kExactMath = PT_MATH_EXACT != 0;
}  // namespace PTK_IMPL
