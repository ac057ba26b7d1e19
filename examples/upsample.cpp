// upsample.cpp -- one frame of World::new() traced at half the resolution and reconstructed at full size under the full-size
// first-hit features (World::render_denoised_upsampled, pt_render_denoised_upsampled), beside what plain bilinear upsampling
// makes of the same denoised low film.
//
//   ./upsample [spp [out_prefix]]        defaults: 16 upsample
// writes <prefix>_low.ppm (200 x 200), <prefix>_bilinear.ppm and <prefix>_guided.ppm (400 x 400)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../pathtrace_amd/host/pathtrace.hpp"

using namespace pathtrace;

// the display transform of every render: sqrt, clamp, truncation
static void write_ppm(const std::string& path, const std::vector<Vector3>& film, uint32_t w, uint32_t h) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot create " + path);
    std::fprintf(f, "P6\n%u %u\n255\n", w, h);
    for (const Vector3& v : film) {
        const double c[3] = {v.x, v.y, v.z};
        for (double ch : c) std::fputc((int)(uint8_t)(std::min(1.0, std::max(0.0, std::sqrt(ch))) * 255.0), f);
    }
    std::fclose(f);
}

// bilinear upsampling on the positions of the upsampling rule (include/pathtrace_amd.h), taps outside the image dropped
static std::vector<Vector3> bilinear(const std::vector<Vector3>& lo, uint32_t w, uint32_t h, uint32_t W, uint32_t H) {
    std::vector<Vector3> out((size_t)W * H);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const double X = ((x + 0.5) * (w - 1)) / (W - 1) - 0.5, Y = h - 0.5 - ((H - 1 - y + 0.5) * (h - 1)) / (H - 1);
            const double x0 = std::floor(X), y0 = std::floor(Y), fx = X - x0, fy = Y - y0;
            double sum[3] = {0, 0, 0}, wsum = 0;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const int qx = (int)x0 + i, qy = (int)y0 + j;
                    if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h) continue;
                    const double b = (i ? fx : 1 - fx) * (j ? fy : 1 - fy);
                    const Vector3& v = lo[(size_t)qy * w + qx];
                    sum[0] += b * v.x; sum[1] += b * v.y; sum[2] += b * v.z;
                    wsum += b;
                }
            out[(size_t)y * W + x] = Vector3(sum[0] / wsum, sum[1] / wsum, sum[2] / wsum);
        }
    return out;
}

int main(int argc, char** argv) {
    const uint32_t spp = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 16;
    const std::string prefix = argc > 2 ? argv[2] : "upsample";
    try {
        World world = World::new_();
        world.params().spp = spp;
        const uint32_t w = WIDTH / 2, h = HEIGHT / 2;
        std::vector<Vector3> lo;
        world.render_denoised_upsampled(w, h, 4, nullptr, nullptr, &lo);
        write_ppm(prefix + "_low.ppm", lo, w, h);
        write_ppm(prefix + "_bilinear.ppm", bilinear(lo, w, h, WIDTH, HEIGHT), WIDTH, HEIGHT);
        write_ppm(prefix + "_guided.ppm", world.luminance_data, WIDTH, HEIGHT);
        std::printf("wrote %s_low.ppm, %s_bilinear.ppm and %s_guided.ppm (%u spp at %u x %u)\n", prefix.c_str(), prefix.c_str(),
                    prefix.c_str(), spp, w, h);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
