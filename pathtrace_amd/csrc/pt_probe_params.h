// pt_probe_params.h -- the parameter structs of the irradiance volume, defined once: the rule headers compute
// from them, the kernels' argument structs (pt_kernels.h) hold them by value, and each is the layout of its public C struct, which
// one helper of the host file that checks it converts (rule_grid, pt_probe_grid.cpp; rule_visibility, pt_probe_vis.cpp; rule_update,
// pt_probe_update.cpp; the layout's static_assert stands beside each).  No HIP, no arithmetic.
#pragma once
#include <stdint.h>

namespace ptgrid {
struct Grid {                 // PtProbeGrid
    double origin[3];
    double spacing[3];
    uint32_t counts[3];
    uint32_t reserved;
};
}  // namespace ptgrid

namespace ptvis {
struct Params {               // PtProbeVisibility; all zero: no maps
    uint32_t resolution;
    uint32_t sharpness_log2;
    float max_distance;
    uint32_t reserved;
};
}  // namespace ptvis

namespace ptupd {
struct Params {               // PtProbeUpdate
    uint32_t rays_per_probe;
    uint32_t first, stride;
    float hysteresis;
    float change_threshold;
    float change_alpha;
    float rotation[9];
    uint32_t reserved;
};
}  // namespace ptupd
