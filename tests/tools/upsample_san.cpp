// Stand-alone driver of the host functions of pathtrace_amd/csrc/pt_upsample.h, built with -fsanitize=address,undefined by
// tests/test_upsample_cpu.py: over the shape pairs of the tests and the degenerate ones around them, every tap index stays
// inside the low planes (which are allocated to their exact size), every pixel has a tap that is not skipped, the equal-size
// case gives the film back bit for bit, records of any bit pattern are taken without a fault, and a NaN or an infinity in the
// low film under a record of another class leaves a pixel that has a tap of its own class the bits it has without it.
// Prints "upsample_san: 0 failed checks".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pathtrace_amd/csrc/pt_upsample.h"

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t next_u32() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }
static float unit() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }
static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

// wild: some fields take any bit pattern (NaN, infinities, denormals, negatives)
static void fill(std::vector<ptup::Rec>& recs, bool wild) {
    for (ptup::Rec& r : recs) {
        // (normals no longer than 1, as a mean of unit normals is: n . n_q <= 1, so the weight of a tap stays finite)
        for (int k = 0; k < 3; ++k) { r.albedo[k] = unit() < 0.1f ? 0.0f : unit(); r.normal[k] = (2.0f * unit() - 1.0f) * 0.57f; }
        r.emitter = unit() < 0.1f ? 1.0f : 0.0f;
        r.depth = unit() < 0.1f ? 0.0f : 0.1f + 10.0f * unit();
        if (wild && unit() < 0.3f) {
            float f[8];                                   // the record's eight floats in order
            std::memcpy(f, &r, sizeof f);
            f[next_u32() % 8u] = from_bits(next_u32());
            std::memcpy(&r, f, sizeof f);
        }
    }
}

static void sweep(uint32_t W, uint32_t H, uint32_t w, uint32_t h, bool wild) {
    const ptup::Shape s{W, H, w, h};
    std::vector<ptup::Rec> lo((size_t)w * h), full((size_t)W * H);
    std::vector<float> c((size_t)w * h * 3), out((size_t)W * H * 3);
    fill(lo, wild);
    fill(full, wild);
    for (float& v : c) v = wild && unit() < 0.05f ? from_bits(next_u32()) : 0.1f + unit();
    CHECK(ptup::ratio(s) >= 1.0f);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            int X0, Y0;
            double fx, fy;
            ptup::position(s, x, y, &X0, &Y0, &fx, &fy);
            CHECK(X0 >= -1 && X0 <= (int)w - 1 && Y0 >= -1 && Y0 <= (int)h - 1);
            CHECK(fx >= 0.0 && fx < 1.0 && fy >= 0.0 && fy < 1.0);
            CHECK((X0 >= 0 && fx < 1.0) || (X0 + 1 < (int)w && fx > 0.0));      // a column with weight inside the image
            CHECK((Y0 >= 0 && fy < 1.0) || (Y0 + 1 < (int)h && fy > 0.0));      // ... and a row
            if (W == w) CHECK(X0 == (int)x && fx == 0.0);
            if (H == h) CHECK(Y0 == (int)y && fy == 0.0);
            const size_t p = (size_t)y * W + x;
            ptup::pixel(s, c.data(), lo.data(), full[p], x, y, 128.0f, 0.025f, &out[3 * p]);
            CHECK((ptup::rgba8(&out[3 * p]) >> 24) == 255u);
            if (!wild) CHECK(out[3 * p] == out[3 * p] && out[3 * p + 1] == out[3 * p + 1] && out[3 * p + 2] == out[3 * p + 2]);
        }
    // zero sigmas: every same-class tap with n . n_q > 0 and equal depth weighs b, the others 0
    float o3[3];
    ptup::pixel(s, c.data(), lo.data(), full[0], 0, 0, 0.0f, 0.0f, o3);
    if (!wild) CHECK(o3[0] == o3[0]);
}

static void identity(uint32_t W, uint32_t H) {
    const ptup::Shape s{W, H, W, H};
    std::vector<ptup::Rec> recs((size_t)W * H);
    std::vector<float> c((size_t)W * H * 3);
    fill(recs, false);
    for (float& v : c) v = unit();
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            float o[3];
            ptup::pixel(s, c.data(), recs.data(), recs[p], x, y, 128.0f, 0.025f, o);
            for (int k = 0; k < 3; ++k) {
                const float a = ptup::albedo(recs[p].albedo[k]);
                const float want = (c[3 * p + k] / a) * a;
                CHECK(std::memcmp(&o[k], &want, 4) == 0);
            }
        }
}

// rule 5: a tap with w_q = 0 is not read.  The low film poisoned under every record that is no surface: a surface pixel with a
// live surface tap keeps its bits; some other pixel does change.
static void isolation(uint32_t W, uint32_t H, uint32_t w, uint32_t h, float sigma_n, float sigma_d) {
    const ptup::Shape s{W, H, w, h};
    std::vector<ptup::Rec> lo((size_t)w * h), full((size_t)W * H);
    std::vector<float> c((size_t)w * h * 3);
    fill(lo, false);
    fill(full, false);
    for (float& v : c) v = 0.1f + unit();
    const float poisons[] = {from_bits(0x7FC00000u), from_bits(0x7F800000u), from_bits(0xFF800000u), 3e38f};
    for (float poison : poisons) {
        std::vector<float> bad = c;
        for (size_t q = 0; q < lo.size(); ++q)
            if (ptup::cls(lo[q]) != ptup::kSurface) bad[3 * q] = bad[3 * q + 1] = bad[3 * q + 2] = poison;
        size_t kept = 0, changed = 0;
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x;
                int X0, Y0;
                double fx, fy;
                ptup::position(s, x, y, &X0, &Y0, &fx, &fy);
                bool own = false;
                for (int k = 0; k < 4; ++k) {
                    const int i = k & 1, j = k >> 1, qx = X0 + i, qy = Y0 + j;
                    const float b = (float)((i ? fx : 1.0 - fx) * (j ? fy : 1.0 - fy));
                    if (qx < 0 || qy < 0 || qx >= (int)w || qy >= (int)h || b == 0.0f) continue;
                    own = own || ptup::cls(lo[(size_t)qy * w + (size_t)qx]) == ptup::cls(full[p]);
                }
                float o0[3], o1[3];
                ptup::pixel(s, c.data(), lo.data(), full[p], x, y, sigma_n, sigma_d, o0);
                ptup::pixel(s, bad.data(), lo.data(), full[p], x, y, sigma_n, sigma_d, o1);
                if (ptup::cls(full[p]) == ptup::kSurface && own) {
                    ++kept;
                    CHECK(std::memcmp(o0, o1, sizeof o0) == 0);
                } else if (std::memcmp(o0, o1, sizeof o0) != 0) {
                    ++changed;
                }
            }
        if (W * H >= 64u) CHECK(kept > 0 && changed > 0);
    }
}

int main() {
    const uint32_t pairs[][4] = {{2, 2, 2, 2}, {64, 48, 64, 48}, {67, 35, 34, 18}, {130, 129, 65, 65}, {257, 3, 33, 2},
                                 {3, 2, 2, 2}, {2, 3, 2, 2}, {9, 2, 3, 2}, {2, 9, 2, 3}, {5, 5, 2, 5}, {5, 5, 5, 2}, {1000, 2, 2, 2}, {7, 7, 6, 6},
                                 // tests/upsample_cases.py: odd integer ratios (pixels on the low lattice), extreme ratios, barely above 1,
                                 // one axis scaled, around the 32 x 8 block
                                 {7, 7, 3, 3}, {16, 10, 6, 4}, {97, 65, 33, 17}, {101, 21, 21, 5}, {1025, 2, 2, 2}, {2, 513, 2, 3}, {300, 3, 3, 3},
                                 {66, 34, 65, 33}, {67, 35, 34, 35}, {67, 35, 67, 18}, {31, 7, 16, 4}, {32, 8, 16, 4}, {33, 9, 17, 5}};
    for (const auto& q : pairs) {
        sweep(q[0], q[1], q[2], q[3], false);
        sweep(q[0], q[1], q[2], q[3], true);
        isolation(q[0], q[1], q[2], q[3], 128.0f, 0.025f);
    }
    isolation(67, 35, 34, 18, 0.0f, 0.0f);
    isolation(16, 10, 6, 4, 3.0f, 0.5f);
    identity(2, 2);
    identity(64, 48);
    ptup::Rec r{};
    CHECK(ptup::cls(r) == ptup::kMiss);
    r.depth = 1.0f; CHECK(ptup::cls(r) == ptup::kSurface);
    r.emitter = 1.0f; CHECK(ptup::cls(r) == ptup::kEmitter);
    r.depth = 0.0f; CHECK(ptup::cls(r) == ptup::kMiss);
    r.depth = from_bits(0x7FC00000u); r.emitter = from_bits(0x7FC00000u); CHECK(ptup::cls(r) == ptup::kSurface);
    std::printf("upsample_san: %d failed checks\n", failed);
    return failed != 0;
}
