// bake.cpp -- light baking on World::new(): the floor of the Cornell box as a 64 x 64 lightmap (World::bake_lightmap,
// pt_bake_lightmap_host) and a 4 x 4 x 4 grid of irradiance probes in the box (World::bake_probes, pt_bake_probes_host), each
// probe's light as nine spherical-harmonics coefficients per channel.
//
//   ./bake [spp [out_prefix]]        defaults: 64 bake
// writes <prefix>_floor.ppm (the floor's outgoing radiance: lightmap x the floor's albedo) and prints, per probe layer, the
// irradiance a surface facing up and one facing down would receive there.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../pathtrace_amd/host/pathtrace.hpp"

using namespace pathtrace;

int main(int argc, char** argv) {
    const uint32_t spp = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 64;
    const std::string prefix = argc > 2 ? argv[2] : "bake";
    try {
        World world = World::new_();
        world.params().spp = spp;
        // the floor of World::new(): y = -1, x in [-1, 1], z in [-3, -1], normal +y; texel centres
        const uint32_t W = 64, H = 64;
        std::vector<float> texels((size_t)W * H * 6);
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                float* t = &texels[6 * ((size_t)y * W + x)];
                t[0] = -1.0f + 2.0f * (x + 0.5f) / W; t[1] = -1.0f; t[2] = -3.0f + 2.0f * (y + 0.5f) / H;
                t[3] = 0.0f; t[4] = 1.0f; t[5] = 0.0f;
            }
        const std::vector<Vector3> map = world.bake_lightmap(W, H, texels);
        const double albedo[3] = {0.2, 0.8, 0.8};
        const std::string path = prefix + "_floor.ppm";
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot create " + path);
        std::fprintf(f, "P6\n%u %u\n255\n", W, H);
        for (const Vector3& v : map) {
            const double c[3] = {v.x * albedo[0], v.y * albedo[1], v.z * albedo[2]};
            for (double ch : c) std::fputc((int)(uint8_t)(std::min(1.0, std::max(0.0, std::sqrt(ch))) * 255.0), f);
        }
        std::fclose(f);
        std::printf("wrote %s (%u x %u texels, %u spp)\n", path.c_str(), W, H, spp);
        // 4 x 4 x 4 probes inside the box
        const uint32_t G = 4, R = 256;
        std::vector<float> pos;
        for (uint32_t k = 0; k < G; ++k)
            for (uint32_t j = 0; j < G; ++j)
                for (uint32_t i = 0; i < G; ++i) {
                    pos.push_back(-0.75f + 0.5f * i); pos.push_back(-0.75f + 0.5f * k); pos.push_back(-2.75f + 0.5f * j);
                }
        world.params().spp = std::max(1u, spp / 16);
        const std::vector<float> sh = world.bake_probes(pos, R);
        for (uint32_t k = 0; k < G; ++k) {
            Vector3 up(0, 0, 0), down(0, 0, 0);
            for (uint32_t p = k * G * G; p < (k + 1) * G * G; ++p) {
                const Vector3 u = World::irradiance(&sh[27 * (size_t)p], Vector3(0, 1, 0)), d = World::irradiance(&sh[27 * (size_t)p], Vector3(0, -1, 0));
                up = Vector3(up.x + u.x / (G * G), up.y + u.y / (G * G), up.z + u.z / (G * G));
                down = Vector3(down.x + d.x / (G * G), down.y + d.y / (G * G), down.z + d.z / (G * G));
            }
            std::printf("probes at y = %+.2f: irradiance facing up (%.3f %.3f %.3f), facing down (%.3f %.3f %.3f)\n", -0.75 + 0.5 * k, up.x, up.y, up.z,
                        down.x, down.y, down.z);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
