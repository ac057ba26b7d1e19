// pt_probe_entry.h -- what the two host files of the irradiance volume share (internal to csrc/): the checks and passes of
// pt_probe_grid.cpp that the probe-visibility entries of pt_probe_vis.cpp run with their moment maps, and the checks and the
// distance pass of pt_probe_vis.cpp that the update entries of pt_probe_update.cpp run with their own ray source.
#pragma once
#include "pt_entry.h"
#include "pt_probe_grid.h"

namespace ptprobe {

// The moment maps of a shading pass with the visibility term; none: the pass without it
struct Maps { const float* moments = nullptr; const PtProbeVisibility* vis = nullptr; };

// the public grid as the rule and the kernels take it: the one conversion
ptgrid::Grid rule_grid(const PtProbeGrid* g);
int check_grid(const char* who, const PtProbeGrid* g);
// the 1..65535 rows and columns of a probe film
int check_probe_count(const char* who, uint32_t n_probes);
int check_rays_per_probe(const char* who, uint32_t rays_per_probe);
// what a shading pass reads and writes, checked before anything looks at a context; feat_align: 16 on the device, 4 on the host
int check_shade(const char* who, const PtCamera* cam, const PtProbeGrid* g, const void* sh27, const void* features, const void* fallback,
                const PtProbeShade* sp, const void* out_linear, const void* out_rgba, uint32_t feat_align, bool own_features = false);
// what pt_render_probe_lit_* checks of its own before the feature pass checks the rest
int check_probe_lit(const char* who, const PtContext* c, const PtCamera* cam, const PtRenderParams* prm, const PtProbeGrid* g, const void* sh27,
                    const void* fallback, const PtProbeShade* sp, const void* out_linear, const void* out_rgba);
// the launch of a checked shading pass
int shade_launch(PtContext* c, const PtCamera* cam, const PtProbeGrid* g, const float* d_sh27, const float* d_features, const float* d_fallback,
                 const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba, const Maps& maps = {});
// the feature pass into the context's plane, then the shading
int probe_lit_impl(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g, const float* d_sh27,
                   const float* d_fallback, const PtProbeShade* sp, float* d_out_linear, uint8_t* d_out_rgba, const Maps& maps = {});
// the rule on the CPU
void shade_host(const PtCamera* cam, const PtProbeGrid* g, const float* sh27, const float* features, const float* fallback, const PtProbeShade* sp,
                float* out_linear, uint8_t* out_rgba, const Maps& maps = {});
// probe_lit_impl from and into host buffers through the context's staging
int probe_lit_host(PtContext* c, const PtCamera* cam, const PtRenderParams* prm, uint32_t feature_samples, const PtProbeGrid* g, const float* sh27,
                   const float* fallback, const PtProbeShade* sp, float* out_linear, uint8_t* out_rgba, const Maps& maps = {});

// ---- pt_probe_vis.cpp
// the public visibility struct as the rule and the kernels take it: the one conversion; null: all zero, no maps
ptvis::Params rule_visibility(const PtProbeVisibility* vis);
// the parameters of the maps, then their plane: 8-byte aligned for a device entry, 4-byte for a host entry
int check_moments_plane(const char* who, const PtProbeVisibility* vis, const void* moments, bool device);
// the first-hit distances of n_rows x R rays of a source whose film has one row per probe, in chunks of whole rows through the
// feature pass's scratch: source(ctx, base, nb) is the source of the rows base .. base + nb - 1.  Everything checked by the caller.
using RowSource = ptk::RaySourceF (*)(const void* ctx, uint32_t base, uint32_t nb);
int distances_of(PtContext* c, uint32_t n_rows, uint32_t R, const PtRenderParams* prm, float* d_out, RowSource source, const void* ctx);

}  // namespace ptprobe
