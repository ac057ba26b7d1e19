// cornell.cpp -- what the reference's main() does, minus the window (src/main.rs:39-67):
// build World::new(), render every pixel, export luminance.csv, and write a PPM of
// World.data instead of blitting it to a winit/pixels surface (out of scope).
//
//   ./cornell [width height spp [out_prefix [exact_math]]] [--aperture A --focus F] [--projection ortho|fisheye|equirect [--fov DEG]] [--cascade] [--filter KIND --radius R] [--bloom [INTENSITY]]       defaults: 400 400 64 cornell 0, no lens
//   --projection ortho|fisheye|equirect [--fov DEG]: another projection of the same camera (World::render_projection; --fov: the
//                       fisheye's field of view across the width, default 180)
//   --cascade: the film is formed by the brightness cascade (World::render_cascade, pt_default_cascade): fireflies are re-weighted
//   --filter box|tent|gaussian|mitchell [--radius R]: the film is reconstructed with that filter (World::render_filtered; gaussian:
//                       alpha 2, mitchell: B = C = 1/3; R defaults to 0.5 / 1 / 1.5 / 2)
//   --bloom [INTENSITY]: behind the render the film goes through World::display (pt_display_device: bloom with pt_default_bloom and
//                       that intensity, default 0.05, then auto-exposure and ACES); the PPM is the displayed frame, the CSV the linear film
//   CORNELL_DENOISE=n: render_denoised with n feature samples (pt_render_denoised) instead of render()
//   CORNELL_ADAPTIVE_DENOISE=n: render_adaptive_denoised with n feature samples (pt_render_adaptive_denoised): spp is spp_max,
//                       spp_min 4, spp_step 4, rel_tol 0.1
//   CORNELL_TEMPORAL=k: k frames of render_denoised_temporal (4 feature samples), frame i at spp_offset i*spp with the camera
//                       origin moved by (0.01 i, 0.005 i, 0); the files hold the last frame
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../pathtrace_amd/host/pathtrace.hpp"

using namespace pathtrace;

int main(int argc, char** argv) {
    // optional, anywhere on the line: --aperture A --focus F (a thin lens, World::render_lens; with CORNELL_DENOISE its denoised form)
    PtLens lens;
    pt_default_lens(&lens);
    bool use_lens = false, use_cascade = false, use_filter = false, use_projection = false;
    Projection projection = Projection::Perspective;
    double projection_fov = 180.0;
    PtFilter flt;
    pt_default_filter(&flt);
    float flt_radius = 0.0f;
    bool use_bloom = false;
    PtBloom bloom;
    pt_default_bloom(&bloom);
    {
        int keep = 1;
        for (int i = 1; i < argc; ++i) {
            const std::string arg = argv[i];
            if ((arg == "--aperture" || arg == "--focus") && i + 1 < argc) {
                (arg == "--aperture" ? lens.aperture : lens.focus_distance) = std::atof(argv[++i]);
                use_lens = true;
            } else if (arg == "--projection" && i + 1 < argc) {
                const std::string kind = argv[++i];
                use_projection = true;
                if (kind == "ortho") projection = Projection::Orthographic;
                else if (kind == "fisheye") projection = Projection::Fisheye;
                else if (kind == "equirect") projection = Projection::Equirect;
                else { std::fprintf(stderr, "--projection: ortho, fisheye or equirect\n"); return 2; }
            } else if (arg == "--fov" && i + 1 < argc) {
                projection_fov = std::atof(argv[++i]);
            } else if (arg == "--cascade") {
                use_cascade = true;
            } else if (arg == "--filter" && i + 1 < argc) {
                const std::string kind = argv[++i];
                use_filter = true;
                if (kind == "box") { flt.kind = PT_FILTER_BOX; flt.radius = 0.5f; }
                else if (kind == "tent") { flt.kind = PT_FILTER_TENT; flt.radius = 1.0f; }
                else if (kind == "mitchell") { flt.kind = PT_FILTER_MITCHELL; flt.radius = 2.0f; flt.a = flt.b = 1.0f / 3.0f; }
                else if (kind != "gaussian") { std::fprintf(stderr, "--filter: box, tent, gaussian or mitchell\n"); return 2; }
            } else if (arg == "--bloom") {
                use_bloom = true;
                if (i + 1 < argc && (std::isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '.') && std::strchr(argv[i + 1], '.'))
                    bloom.intensity = (float)std::atof(argv[++i]);    // an intensity is written with a point: 0.1 (a bare integer is the width)
            } else if (arg == "--radius" && i + 1 < argc) {
                flt_radius = (float)std::atof(argv[++i]);
            } else {
                argv[keep++] = argv[i];
            }
        }
        argc = keep;
    }
    const uint32_t w = argc > 2 ? (uint32_t)std::atoi(argv[1]) : WIDTH;
    const uint32_t h = argc > 2 ? (uint32_t)std::atoi(argv[2]) : HEIGHT;
    const uint32_t spp = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 64;
    const std::string prefix = argc > 4 ? argv[4] : "cornell";
    const uint32_t exact_math = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 0;
    try {
        // World::new() fixes 400x400; other sizes re-author the same scene with the same camera model
        World world = World::new_();
        if (w != WIDTH || h != HEIGHT) {
            // re-author the same 13 objects through the mirrored constructors for a camera of another size
            World resized(Camera::new_(Vector3(0.0, 0.0, 2.0), w, h, 1.0, 35.0));
            uint32_t n = 0;
            check(pt_builtin_scene(1, 0, nullptr, 0, &n));
            std::vector<PtObject> objs(n);
            check(pt_builtin_scene(1, 0, objs.data(), n, &n));
            world = std::move(resized);
            for (const PtObject& o : objs) {
                if (o.shape_tag == PT_SHAPE_TRIANGLE) {
                    TriangleShape t = TriangleShape::new_(Vector3(o.shape[0], o.shape[1], o.shape[2]),
                                                          Vector3(o.shape[3], o.shape[4], o.shape[5]),
                                                          Vector3(o.shape[6], o.shape[7], o.shape[8]));
                    if (o.mat_tag == PT_MAT_EMISSIVE) world.push(Object::new_(t, Emissive::new_(Vector3(o.mat[0], o.mat[1], o.mat[2]))));
                    else world.push(Object::new_(t, LambertianCosineWeighted::new_(Vector3(o.mat[0], o.mat[1], o.mat[2]))));
                } else {
                    world.push(Object::new_(SphereShape::new_(Vector3(o.shape[0], o.shape[1], o.shape[2]), o.shape[3]),
                                            Mirror{o.mat[0], Vector3(o.mat[1], o.mat[2], o.mat[3]), o.mat[4], o.mat[5]}));
                }
            }
        }
        world.params().spp = spp;
        world.params().exact_math = exact_math;
        const auto t0 = std::chrono::steady_clock::now();
        if (std::getenv("CORNELL_TEMPORAL")) {       // temporal form: CORNELL_TEMPORAL = frames
            const uint32_t frames = (uint32_t)std::atoi(std::getenv("CORNELL_TEMPORAL"));
            for (uint32_t i = 0; i < frames; ++i) {
                world.set_camera(Camera::new_(Vector3(0.01 * i, 0.005 * i, 2.0), w, h, 1.0, 35.0));
                world.params().spp_offset = i * spp;
                world.render_denoised_temporal(4);
            }
        } else if (std::getenv("CORNELL_ADAPTIVE_DENOISE"))   // adaptive denoised form: CORNELL_ADAPTIVE_DENOISE = feature samples
            world.render_adaptive_denoised(4, 4, 0.1, 1e-3, (uint32_t)std::atoi(std::getenv("CORNELL_ADAPTIVE_DENOISE")));
        else if (use_lens && std::getenv("CORNELL_DENOISE"))
            world.render_lens_denoised(lens, (uint32_t)std::atoi(std::getenv("CORNELL_DENOISE")));
        else if (use_lens)
            world.render_lens(lens);
        else if (use_projection)
            world.render_projection(projection, projection_fov);
        else if (use_cascade)
            world.render_cascade();
        else if (use_filter) {
            if (flt_radius != 0.0f) flt.radius = flt_radius;
            world.render_filtered(&flt);
        }
        else if (std::getenv("CORNELL_DENOISE"))   // denoised form: CORNELL_DENOISE = feature samples
            world.render_denoised((uint32_t)std::atoi(std::getenv("CORNELL_DENOISE")));
        else if (std::getenv("CORNELL_PROGRESSIVE"))      // live-preview form: one line per increment
            world.render_progressive(std::max(1u, spp / 4), [&](uint32_t done) {
                std::printf("  preview after %u spp: centre pixel rgb = %u %u %u\n", done, world.data[(h / 2) * w + w / 2].r,
                            world.data[(h / 2) * w + w / 2].g, world.data[(h / 2) * w + w / 2].b);
                return false; });
        else
            world.render();
        if (use_bloom) std::printf("display: bloom intensity %g, log2 exposure %.3f\n", bloom.intensity, world.display(&bloom));
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const PtStats st = world.stats();
        std::printf("Rendering complete: %ux%u, %u spp, %zu objects, %.3f s (%.1f Msamples/s), %llu vertices\n", w, h, spp,
                    world.object_count(), dt, (double)st.samples / dt / 1e6, (unsigned long long)st.vertices);
        world.export_luminance(prefix + "_luminance.csv");     // main.rs:64-66
        world.write_ppm(prefix + ".ppm");
        std::printf("wrote %s_luminance.csv and %s.ppm\n", prefix.c_str(), prefix.c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
