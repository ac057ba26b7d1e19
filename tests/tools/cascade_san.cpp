// Stand-alone driver of the host functions of pathtrace_amd/csrc/pt_cascade.h, built with -fsanitize=address,undefined by
// tests/test_cascade_cpu.py: over the image sizes, sample counts and layer counts of the tests, with samples log-uniform over
// 2^-4 .. 2^24 and special values (0, negatives, denormals, NaN, infinities, any bit pattern) among them, every plane is
// allocated to its exact size, so an index outside one is a fault.  Checks on the way: the split takes one branch and its
// weights add up, dark samples give the plain film bit for bit, and the optional planes may be left out.
// Prints "cascade_san: 0 failed checks".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pathtrace_amd/csrc/pt_cascade.h"

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static uint32_t rng_state = 2018u;
static uint32_t next_u32() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }
static float unit() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }
static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

static float sample_value(bool wild) {
    if (wild && unit() < 0.08f) {
        const float special[] = {0.0f, -1.0f, -0.0f, 1e-42f, from_bits(0x7FC00000u), from_bits(0x7F800000u), from_bits(0xFF800000u),
                                 from_bits(next_u32())};
        return special[next_u32() % 8u];
    }
    // 2^(-4 + 28 u) without exp or pow: the exponent field directly, a uniform mantissa
    const uint32_t e = 127u - 4u + next_u32() % 28u;
    return from_bits(e << 23 | (next_u32() & 0x7FFFFFu));
}

static void sweep(uint32_t W, uint32_t H, uint32_t n, uint32_t K, float kappa, bool wild) {
    ptcas::Levels lv;
    CHECK(ptcas::levels(K, 1.0f, 8.0f, kappa, &lv));
    const size_t np = (size_t)W * H;
    std::vector<float> smp(np * n * 3), film(np * 3), plain(np * 3), weights(np * K), film2(np * 3);
    std::vector<uint8_t> rgba(np * 4);
    std::vector<double> layers(np * K * 3);
    for (float& v : smp) v = sample_value(wild);
    ptcas::host_film(lv, W, H, n, smp.data(), film.data(), rgba.data(), plain.data(), layers.data(), weights.data());
    ptcas::host_film(lv, W, H, n, smp.data(), film2.data(), nullptr, nullptr, nullptr, nullptr);
    CHECK(std::memcmp(film.data(), film2.data(), film.size() * sizeof(float)) == 0);
    for (size_t p = 0; p < np; ++p) CHECK(rgba[4 * p + 3] == 255u);
    for (float w : weights) CHECK(w == w && (wild || (w >= 0.0f && w <= 1.0f)));
    if (!wild)
        for (float v : film) CHECK(v == v && v >= 0.0f);
}

static void dark(uint32_t W, uint32_t H, uint32_t n) {
    ptcas::Levels lv;
    CHECK(ptcas::levels(6, 1.0f, 8.0f, 8.0f, &lv));
    const size_t np = (size_t)W * H;
    std::vector<float> smp(np * n * 3), film(np * 3), plain(np * 3);
    for (float& v : smp) v = unit();
    ptcas::host_film(lv, W, H, n, smp.data(), film.data(), nullptr, plain.data(), nullptr, nullptr);
    CHECK(std::memcmp(film.data(), plain.data(), film.size() * sizeof(float)) == 0);
}

int main() {
    const uint32_t sizes[][2] = {{2, 2}, {3, 5}, {17, 9}, {33, 16}, {2, 40}, {40, 2}};
    const uint32_t counts[] = {1, 3, 4, 5, 16}, layer_counts[] = {2, 3, 6, 8};
    for (const auto& s : sizes)
        for (uint32_t n : counts)
            for (uint32_t K : layer_counts) {
                sweep(s[0], s[1], n, K, 1.0f, false);
                sweep(s[0], s[1], n, K, 1.0f, true);
                sweep(s[0], s[1], n, K, 0.0f, true);
            }
    dark(17, 9, 5);
    // the split: one branch, weights that add up, at every level and around it
    for (uint32_t K : layer_counts) {
        ptcas::Levels lv;
        CHECK(ptcas::levels(K, 1.0f, 8.0f, 1.0f, &lv));
        const double nan = __builtin_nan(""), inf = __builtin_inf();
        std::vector<double> cases = {0.0, -3.0, 4.9e-324, nan, inf, -inf, 2.5, 1e30};
        for (uint32_t k = 0; k < K; ++k) { cases.push_back(lv.B[k]); cases.push_back(__builtin_nextafter(lv.B[k], 0.0)); cases.push_back(__builtin_nextafter(lv.B[k], inf)); }
        for (double L : cases) {
            uint32_t j;
            double lo, hi;
            ptcas::split(lv, L, &j, &lo, &hi);
            CHECK(j + 1u < K);
            CHECK(lo >= 0.0 && lo <= 1.0 && hi >= 0.0 && hi <= 1.0);
            const double sum = lo + hi;
            CHECK(sum > 1.0 - 3e-16 && sum < 1.0 + 3e-16);
            if (!(L > lv.B[j])) CHECK(lo == 1.0 && hi == 0.0);
            if (L >= lv.B[K - 1u]) CHECK(j == K - 2u && lo == 0.0 && hi == 1.0);
        }
    }
    ptcas::Levels lv;
    CHECK(!ptcas::levels(1, 1.0f, 8.0f, 1.0f, &lv) && !ptcas::levels(9, 1.0f, 8.0f, 1.0f, &lv) && !ptcas::levels(6, 0.0f, 8.0f, 1.0f, &lv));
    CHECK(!ptcas::levels(6, 1.0f, 1.5f, 1.0f, &lv) && !ptcas::levels(6, 1.0f, 8.0f, -1.0f, &lv));
    CHECK(ptcas::levels(8, 3.4028235e38f, 3.4028235e38f, 1.0f, &lv) && lv.B[7] - lv.B[7] == 0.0);      // the largest table is finite
    CHECK(!ptcas::levels(6, from_bits(0x7FC00000u), 8.0f, 1.0f, &lv) && !ptcas::levels(6, 1.0f, from_bits(0x7F800000u), 1.0f, &lv));
    std::printf("cascade_san: %d failed checks\n", failed);
    return failed != 0;
}
