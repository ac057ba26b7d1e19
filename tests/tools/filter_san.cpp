// Stand-alone driver of the host functions of pathtrace_amd/csrc/pt_filter.h, built with -fsanitize=address,undefined by
// tests/test_filter_cpu.py: over the image sizes, sample counts, kinds and radii of the tests, with samples log-uniform over
// 2^-8 .. 2^8 and special values (0, negatives, denormals, NaN, infinities, any bit pattern) among them, every plane is allocated
// to its exact size, so an index outside one is a fault.  Checks on the way: box 0.5 is the plain film bit for bit with Wt = n,
// a constant image stays constant under the positive filters, the optional planes may be left out, the weight vanishes from R
// on, exp_neg stays in (0, 1], the parameter refusals.
// Prints "filter_san: 0 failed checks".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pathtrace_amd/csrc/pt_filter.h"

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static uint32_t rng_state = 1988u;
static uint32_t next_u32() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }
static float unit() { return (float)(next_u32() >> 8) * (1.0f / 16777216.0f); }
static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

static float sample_value(bool wild) {
    if (wild && unit() < 0.08f) {
        const float special[] = {0.0f, -1.0f, -0.0f, 1e-42f, from_bits(0x7FC00000u), from_bits(0x7F800000u), from_bits(0xFF800000u),
                                 from_bits(next_u32())};
        return special[next_u32() % 8u];
    }
    const uint32_t e = 127u - 8u + next_u32() % 16u;       // 2^(-8 + 16 u): the exponent field directly, a uniform mantissa
    return from_bits(e << 23 | (next_u32() & 0x7FFFFFu));
}

static void sweep(uint32_t W, uint32_t H, uint32_t n, uint32_t kind, float radius, float a, float b, bool wild) {
    ptflt::Rule r;
    CHECK(ptflt::rule(kind, radius, a, b, &r));
    const size_t np = (size_t)W * H;
    std::vector<float> smp(np * n * 3), film(np * 3), plain(np * 3), film2(np * 3);
    std::vector<uint8_t> rgba(np * 4);
    std::vector<double> wsum(np);
    for (float& v : smp) v = sample_value(wild);
    const uint32_t first = next_u32();
    ptflt::host_film(r, W, H, n, first, smp.data(), film.data(), rgba.data(), plain.data(), wsum.data());
    ptflt::host_film(r, W, H, n, first, smp.data(), film2.data(), nullptr, nullptr, nullptr);
    CHECK(std::memcmp(film.data(), film2.data(), film.size() * sizeof(float)) == 0);
    for (size_t p = 0; p < np; ++p) CHECK(rgba[4 * p + 3] == 255u);
    for (double w : wsum) CHECK(w == w && w - w == 0.0);
    if (kind == ptflt::kBox && radius == 0.5f) {
        CHECK(std::memcmp(film.data(), plain.data(), film.size() * sizeof(float)) == 0);
        for (double w : wsum) CHECK(w == (double)n);
    }
    if (!wild && kind != ptflt::kMitchell)
        for (float v : film) CHECK(v == v && v >= 0.0f);
}

static void constant(uint32_t kind, float radius, float a) {
    ptflt::Rule r;
    CHECK(ptflt::rule(kind, radius, a, 0.0f, &r));
    const uint32_t W = 17, H = 9, n = 5;
    std::vector<float> smp((size_t)W * H * n * 3, 0.37f), film((size_t)W * H * 3);
    ptflt::host_film(r, W, H, n, 0, smp.data(), film.data(), nullptr, nullptr, nullptr);
    for (float v : film) CHECK(v > 0.37f - 1e-7f && v < 0.37f + 1e-7f);
}

int main() {
    const uint32_t sizes[][2] = {{2, 2}, {3, 5}, {17, 9}, {33, 16}, {2, 40}, {40, 2}};
    const uint32_t counts[] = {1, 3, 4, 5, 16};
    const float radii[] = {0.5f, 0.75f, 1.5f, 1.51f, 2.0f, 2.5f};
    const float params[][3] = {{0, 0.0f, 0.0f}, {1, 0.0f, 0.0f}, {2, 2.0f, 0.0f}, {2, 16.0f, 0.0f}, {3, 1.0f / 3.0f, 1.0f / 3.0f}, {3, 0.0f, 1.0f}};
    for (const auto& s : sizes)
        for (uint32_t n : counts)
            for (float R : radii)
                for (const auto& p : params) {
                    if ((s[0] * s[1] > 300u) && n == 16 && R < 2.5f) continue;      // (time: the largest images take 16 samples at the widest radius only)
                    sweep(s[0], s[1], n, (uint32_t)p[0], R, p[1], p[2], false);
                    sweep(s[0], s[1], n, (uint32_t)p[0], R, p[1], p[2], true);
                }
    for (float R : radii) { constant(ptflt::kBox, R, 0.0f); constant(ptflt::kTent, R, 0.0f); constant(ptflt::kGaussian, R, 2.0f); }
    // the weight: zero from R on, finite below; the taps reach every sample with a non-zero weight
    for (float R : radii)
        for (const auto& p : params) {
            ptflt::Rule r;
            CHECK(ptflt::rule((uint32_t)p[0], R, p[1], p[2], &r));
            CHECK((double)r.m < r.R + 0.5 && (double)r.m + 1.0 >= r.R + 0.5);
            const double inf = __builtin_inf();
            CHECK(ptflt::weight1(r, r.R) == 0.0 && ptflt::weight1(r, __builtin_nextafter(r.R, inf)) == 0.0 && ptflt::weight1(r, inf) == 0.0);
            CHECK(ptflt::weight1(r, (double)r.m + 0.5) == 0.0 || (double)r.m + 0.5 < r.R);
            for (int i = 0; i < 200; ++i) {
                const double t = r.R * (double)unit(), f = ptflt::weight1(r, t);
                CHECK(f - f == 0.0);
                if (r.kind != ptflt::kMitchell) CHECK(f >= 0.0 && f <= 1.0);
            }
        }
    for (int i = 0; i <= 1000; ++i) {
        const double v = ptflt::exp_neg(0.1 * (double)i);
        CHECK(v > 0.0 && v <= 1.0);
    }
    CHECK(ptflt::exp_neg(0.0) == 1.0);
    // the jitter: odd multiples of 2^-24 inside (0, 1), for any counter
    for (int i = 0; i < 1000; ++i) {
        double ox, oy;
        ptflt::offsets(next_u32(), next_u32(), next_u32(), &ox, &oy);
        CHECK(ox > 0.0 && ox < 1.0 && oy > 0.0 && oy < 1.0);
        const double k = ox * 16777216.0;
        CHECK(k == (double)(uint32_t)k && ((uint32_t)k & 1u) == 1u);
    }
    ptflt::Rule r;
    const float nan = from_bits(0x7FC00000u), inf = from_bits(0x7F800000u);
    CHECK(!ptflt::rule(4, 1.0f, 0.0f, 0.0f, &r) && !ptflt::rule(0, 0.49f, 0.0f, 0.0f, &r) && !ptflt::rule(0, 2.51f, 0.0f, 0.0f, &r));
    CHECK(!ptflt::rule(0, nan, 0.0f, 0.0f, &r) && !ptflt::rule(0, inf, 0.0f, 0.0f, &r));
    CHECK(!ptflt::rule(2, 1.5f, 0.0f, 0.0f, &r) && !ptflt::rule(2, 1.5f, 16.5f, 0.0f, &r) && !ptflt::rule(2, 1.5f, nan, 0.0f, &r));
    CHECK(!ptflt::rule(3, 2.0f, -0.1f, 0.5f, &r) && !ptflt::rule(3, 2.0f, 0.5f, 1.1f, &r) && !ptflt::rule(3, 2.0f, nan, 0.5f, &r) &&
          !ptflt::rule(3, 2.0f, 0.5f, inf, &r));
    CHECK(ptflt::rule(0, 1.0f, nan, nan, &r) && ptflt::rule(1, 1.0f, -3.0f, inf, &r));      // a and b are ignored where unused
    std::printf("filter_san: %d failed checks\n", failed);
    return failed != 0;
}
