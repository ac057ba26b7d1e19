// gradient_frames.cpp -- a few frames of the temporal denoiser with temporal gradients through the C++ mirror:
// World::new(), its first sphere moved by (0.05, 0, 0) per frame with set_object() + scene_update(), every frame one
// render_denoised_gradient(2) at spp_offset = frame * spp.  Writes <out_prefix>.ppm of the last frame and
// <out_prefix>_alpha.txt: per frame the pixels whose blend weight was measured (not NaN) and those where it was raised.
//
//   ./gradient_frames [width height spp frames [out_prefix]]        defaults: 48 32 2 3 gradient
//
// --camera: the scene stands still and the camera orbits the box's centre instead (frame k at the angle whose half-angle
// tangent is 0.006 k, radius 2), the light is dimmed to a quarter from frame dim_frame on, and every frame is one
// render_denoised_gradient_camera(2): the previous frame stays usable across set_camera().
//
//   ./gradient_frames --camera [width height spp frames [out_prefix [dim_frame]]]        dim_frame defaults to frames - 1
//
// --tonemap: the ten-sphere box (built-in scene 2) stands still under a fixed camera, the light is dimmed to a quarter from
// frame dim_frame on, every frame is one render_denoised_gradient(2) and then World::tonemap() with the defaults (auto
// exposure).  <out_prefix>_exposure.txt: per frame log2E and the mean RGBA8 luminance of the fixed sqrt transform and of the
// tone-mapped frame; <out_prefix>.ppm is the last tone-mapped frame.
//
//   ./gradient_frames --tonemap [width height spp frames [out_prefix [dim_frame]]]       dim_frame defaults to frames / 2
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../pathtrace_amd/host/pathtrace.hpp"

using namespace pathtrace;

// the orbit of --camera: a point of the circle of radius 2 around the origin in the plane y = 0, in + - * / alone
static Camera orbit_camera(uint32_t k, uint32_t w, uint32_t h) {
    const double t = 0.006 * k, q = 1.0 + t * t;
    return Camera::look_at(Vector3(2.0 * (2.0 * t) / q, 0.0, 2.0 * (1.0 - t * t) / q), Vector3(0.0, 0.0, 0.0), Vector3(0.0, 1.0, 0.0), w, h, 35.0);
}

static double mean_luma8(const std::vector<Color>& data) {
    double s = 0.0;
    for (const Color& c : data) s += 0.2126 * c.r + 0.7152 * c.g + 0.0722 * c.b;
    return data.empty() ? 0.0 : s / (double)data.size();
}

static int tonemap_frames(uint32_t w, uint32_t h, uint32_t spp, uint32_t frames, const std::string& prefix, uint32_t dim_frame) {
    uint32_t n = 0;
    if (pt_builtin_scene(2, 0, nullptr, 0, &n) != PT_OK) throw std::runtime_error(pt_last_error());
    std::vector<PtObject> objs(n);
    if (pt_builtin_scene(2, 0, objs.data(), n, &n) != PT_OK) throw std::runtime_error(pt_last_error());
    World world(Camera::new_(Vector3(0.0, 0.0, 2.0), w, h, 1.0, 35.0));
    for (const PtObject& o : objs) world.push(Object::from_pod(o));
    world.params().spp = spp;
    FILE* f = std::fopen((prefix + "_exposure.txt").c_str(), "w");
    if (!f) throw std::runtime_error("cannot create " + prefix + "_exposure.txt");
    for (uint32_t i = 0; i < frames; ++i) {
        world.params().spp_offset = i * spp;
        if (i == dim_frame) {
            for (size_t k = 0; k < world.object_count(); ++k) {
                PtObject o = world.object(k).pod();
                if (o.mat_tag != PT_MAT_EMISSIVE) continue;
                for (int j = 0; j < 3; ++j) o.mat[j] *= 0.25;
                world.set_object(k, Object::from_pod(o));
            }
            world.scene_update();
        }
        world.render_denoised_gradient(2);
        const double fixed = mean_luma8(world.data);
        const double log2E = world.tonemap();
        std::fprintf(f, "%.9f %.3f %.3f\n", log2E, fixed, mean_luma8(world.data));
    }
    std::fclose(f);
    world.write_ppm(prefix + ".ppm");
    return 0;
}

int main(int argc, char** argv) {
    const bool camera = argc > 1 && std::string(argv[1]) == "--camera";
    const bool tonemap = argc > 1 && std::string(argv[1]) == "--tonemap";
    if (camera || tonemap) { --argc; ++argv; }
    const uint32_t w = argc > 4 ? (uint32_t)std::atoi(argv[1]) : 48, h = argc > 4 ? (uint32_t)std::atoi(argv[2]) : 32;
    const uint32_t spp = argc > 4 ? (uint32_t)std::atoi(argv[3]) : 2, frames = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 3;
    const std::string prefix = argc > 5 ? argv[5] : "gradient";
    try {
        if (tonemap) return tonemap_frames(w, h, spp, frames, prefix, argc > 6 ? (uint32_t)std::atoi(argv[6]) : frames / 2);
        World world = World::new_();
        world.set_camera(Camera::new_(Vector3(0.0, 0.0, 2.0), w, h, 1.0, 35.0));
        world.params().spp = spp;
        const uint32_t dim_frame = argc > 6 ? (uint32_t)std::atoi(argv[6]) : frames - 1;
        size_t ball = 0;
        while (world.object(ball).pod().shape_tag != PT_SHAPE_SPHERE) ++ball;
        const PtObject start = world.object(ball).pod();
        PtTemporal tp{};
        pt_default_temporal(&tp);
        FILE* f = std::fopen((prefix + "_alpha.txt").c_str(), "w");
        if (!f) throw std::runtime_error("cannot create " + prefix + "_alpha.txt");
        for (uint32_t i = 0; i < frames; ++i) {
            std::vector<float> alpha;
            world.params().spp_offset = i * spp;
            if (camera) {
                world.set_camera(orbit_camera(i, w, h));
                if (i == dim_frame) {
                    for (size_t k = 0; k < world.object_count(); ++k) {
                        PtObject o = world.object(k).pod();
                        if (o.mat_tag != PT_MAT_EMISSIVE) continue;
                        for (int j = 0; j < 3; ++j) o.mat[j] *= 0.25;
                        world.set_object(k, Object::from_pod(o));
                    }
                    world.scene_update();
                }
                world.render_denoised_gradient_camera(2, nullptr, &tp, nullptr, nullptr, &alpha);
            } else {
                PtObject o = start;
                o.shape[0] = start.shape[0] + 0.05 * i;
                world.set_object(ball, Object::from_pod(o));
                world.scene_update();
                world.render_denoised_gradient(2, nullptr, &tp, nullptr, nullptr, &alpha);
            }
            size_t measured = 0, raised = 0;
            for (float a : alpha) {
                measured += !std::isnan(a);
                raised += a > tp.alpha;
            }
            std::fprintf(f, "%zu %zu\n", measured, raised);
        }
        std::fclose(f);
        world.write_ppm(prefix + ".ppm");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
