// probe_preview.cpp -- an irradiance volume on builtin scene 2 (the Cornell box of spheres): a grid of SH probes is baked once
// (World::bake_probe_grid), then a frame is shaded from it for the price of a first-hit pass (World::render_probe_lit,
// pt_render_probe_lit_host), beside a path-traced frame of the same camera.
//
//   ./probe_preview [--visibility[=T]] [--update FRAMES[,STRIDE]] [nx [ny [nz [spp [out_prefix]]]]]        defaults: 6 6 6 16 probe_preview
// writes <prefix>_probe_lit.ppm and <prefix>_path_traced.ppm.  The probe-lit frame is biased by construction: mirrors are shaded as
// diffuse surfaces of their colour, and without --visibility light leaks through thin walls.  --visibility[=T] (T in 2 .. 16, default
// 8) bakes the probes' distance-moment maps too (World::bake_probe_visibility) and shades with the visibility term
// (World::render_probe_lit_visibility).  --update FRAMES[,STRIDE] (STRIDE default 1) then dims the light to a quarter
// at frame 0 and follows it without baking again (World::update_probe_grid): per frame every STRIDE-th probe is re-traced
// with 64 rays under that frame's rotation and blended into the stored state, and <prefix>_update_NNN.ppm is written, the probe-lit
// frame over the path-traced frame of the dimmed scene.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../pathtrace_amd/host/pathtrace.hpp"

using namespace pathtrace;

int main(int argc, char** argv) {
    uint32_t resolution = 0;                      // 0: no visibility term
    if (argc > 1 && std::strncmp(argv[1], "--visibility", 12) == 0) {
        resolution = argv[1][12] == '=' ? (uint32_t)std::atoi(argv[1] + 13) : 8u;
        --argc; ++argv;
    }
    uint32_t frames = 0, stride = 1;
    if (argc > 2 && std::strcmp(argv[1], "--update") == 0) {
        frames = (uint32_t)std::atoi(argv[2]);
        if (const char* comma = std::strchr(argv[2], ',')) stride = (uint32_t)std::atoi(comma + 1);
        if (frames == 0 || stride == 0) { std::fprintf(stderr, "--update FRAMES[,STRIDE]: both must be > 0\n"); return 1; }
        argc -= 2; argv += 2;
    }
    uint32_t counts[3] = {6, 6, 6};
    for (int a = 0; a < 3; ++a)
        if (argc > 1 + a) counts[a] = (uint32_t)std::atoi(argv[1 + a]);
    const uint32_t spp = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 16;
    const std::string prefix = argc > 5 ? argv[5] : "probe_preview";
    try {
        const uint32_t W = 256, H = 256;
        World world(Camera::new_(Vector3(0.0, 0.0, 2.0), W, H, 1.0, 35.0));
        uint32_t n = 0;
        check(pt_builtin_scene(2, 0, nullptr, 0, &n));
        std::vector<PtObject> objs(n);
        check(pt_builtin_scene(2, 0, objs.data(), n, &n));
        for (const PtObject& o : objs) world.push(Object::from_pod(o));
        // the box is [-1, 1]^2 x [-3, -1]: the probes stay a tenth away from its walls
        PtProbeGrid grid{};
        const double lo[3] = {-0.9, -0.9, -2.9};
        for (int a = 0; a < 3; ++a) {
            grid.counts[a] = counts[a];
            grid.origin[a] = counts[a] > 1 ? lo[a] : lo[a] + 0.9;
            grid.spacing[a] = counts[a] > 1 ? 1.8 / (counts[a] - 1) : 0.0;
        }
        if (pt_probe_grid_count(&grid) == 0) throw std::runtime_error("the counts must be >= 1 and their product at most 65535");
        world.params().spp = spp;
        world.params().integrator = PT_INTEGRATOR_BRDF_ONLY;
        const std::vector<float> sh = world.bake_probe_grid(grid, 256);
        // the path-traced frame; its emitter pixels are what the probe-lit frame shows where it has nothing to shade
        world.render();
        world.write_ppm(prefix + "_path_traced.ppm");
        const std::vector<Vector3> traced = world.luminance_data;
        PtProbeShade shade{};
        pt_default_probe_shade(&shade);
        shade.normal_bias = 0.02f;
        shade.weight = PT_PROBE_WEIGHT_FACING;
        PtProbeVisibility vis{};
        std::vector<float> maps;
        if (resolution) {
            pt_default_probe_visibility(&grid, &vis);
            vis.resolution = resolution;
            maps = world.bake_probe_visibility(grid, 256, vis);
            world.render_probe_lit_visibility(grid, sh, maps, vis, &shade, 1, &traced);
        } else {
            world.render_probe_lit(grid, sh, &shade, 1, &traced);
        }
        world.write_ppm(prefix + "_probe_lit.ppm");
        std::printf("baked %u x %u x %u probes (256 rays x %u spp each); wrote %s_probe_lit.ppm and %s_path_traced.ppm (%u x %u)\n", counts[0], counts[1],
                    counts[2], spp, prefix.c_str(), prefix.c_str(), W, H);
        if (frames) {
            // the light (the scene's one emissive object) at a quarter; the stored state has run for 16 frames
            for (size_t i = 0; i < objs.size(); ++i)
                if (objs[i].mat_tag == PT_MAT_EMISSIVE) {
                    PtObject dim = objs[i];
                    for (int k = 0; k < 3; ++k) dim.mat[k] *= 0.25;
                    world.set_object(i, Object::from_pod(dim));
                }
            world.render();
            const std::vector<Vector3> dimmed = world.luminance_data;
            std::vector<float> state = sh;
            std::vector<uint32_t> age(pt_probe_grid_count(&grid), 16u);
            for (uint32_t f = 0; f < frames; ++f) {
                PtProbeUpdate upd{};
                pt_default_probe_update(f + 1, stride, &upd);
                world.params().spp_offset = spp * (f + 1);
                world.update_probe_grid(grid, resolution ? &vis : nullptr, upd, state, maps, age);
                if (resolution) world.render_probe_lit_visibility(grid, state, maps, vis, &shade, 1, &dimmed);
                else world.render_probe_lit(grid, state, &shade, 1, &dimmed);
                char name[32];
                std::snprintf(name, sizeof name, "_update_%03u.ppm", f);
                world.write_ppm(prefix + name);
            }
            std::printf("dimmed the light to a quarter and ran %u updates of every %u%s probe (64 rays); wrote %s_update_000.ppm .. %03u\n", frames, stride,
                        stride == 1 ? "st" : "th", prefix.c_str(), frames - 1);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
