// pt_kernels_film.hip -- the kernels that work on the film or the scene's arrays, not on paths; one header per concern, in the
// order of their kernels in the code object:
//   pt_film_exchange.h   multi-GPU film exchange
//   pt_film_adaptive.h   adaptive sampling
//   pt_film_denoise.h    the a-trous denoiser
//   pt_film_temporal.h   its temporal accumulation (one body, three entries) and the temporal gradients
//   pt_film_bvh.h        device-side BVH refit and builds (Morton order, median order)
//   pt_film_tonemap.h    auto-exposure and tone mapping
//   pt_film_upsample.h   feature-guided upsampling of a low-resolution film
//   pt_film_cascade.h    the brightness cascade: a firefly-robust resolve and its re-weighting pass
//   pt_film_filter.h     reconstruction filters: a resolve that gathers the neighbours' samples under tent, Gaussian or Mitchell weights
//   pt_film_bloom.h      bloom: the bright part of the film through an image pyramid (LDS-tiled reduce and expand, an in-LDS tail)
//   pt_film_bake.h       light baking: the mask of a lightmap's empty texels, the per-probe spherical-harmonics reduction
//   pt_film_probe.h      irradiance volume: the positions of a probe grid, first-hit pixels shaded from its SH coefficients
//   pt_film_probe_vis.h  its probe visibility: ray distances, per-probe octahedral moment maps, the shading pass that reads them
//   pt_film_probe_update.h  its updates over frames: the fused projection, moments and hysteresis blend of the re-traced probes
// None of them has a division or square root whose result depends on the arithmetic mode, so the unit is compiled once, in
// fast mode (its kernels live in ptk_fast_impl), and serves both modes.
#include "pt_kernels_scan.h"
#if PT_MATH_EXACT
#error "pt_kernels_film.hip is built once, with -DPT_MATH_EXACT=0"
#endif
#include "pt_film_exchange.h"
#include "pt_film_adaptive.h"
#include "pt_film_denoise.h"
#include "pt_film_temporal.h"
#include "pt_film_bvh.h"
#include "pt_film_tonemap.h"
#include "pt_film_upsample.h"
#include "pt_film_cascade.h"
#include "pt_film_filter.h"
#include "pt_film_bloom.h"
#include "pt_film_bake.h"
#include "pt_film_probe.h"
#include "pt_film_probe_vis.h"
#include "pt_film_probe_update.h"
