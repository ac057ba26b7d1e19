// Stand-alone driver of the host functions of pathtrace_amd/csrc/pt_tonemap.h, built with -fsanitize=address,undefined by
// tests/test_tonemap_cpu.py: every histogram word stays inside the 258, the metering handles empty, one-bin and full
// histograms and every window, and the curve and transfer take any bit pattern.  Prints "tonemap_san: 0 failed checks".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pathtrace_amd/csrc/pt_tonemap.h"

static int failed = 0;
#define CHECK(c) do { if (!(c)) { ++failed; std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); } } while (0)

static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

int main() {
    // rule 1: boundaries, and a sweep over the bit patterns
    CHECK(ptone::word(from_bits(0x37800000u)) == 0u);
    CHECK(ptone::word(from_bits(0x377FFFFFu)) == ptone::kDark);
    CHECK(ptone::word(1.0f) == 128u);
    CHECK(ptone::word(65536.0f) == 255u);
    CHECK(ptone::word(from_bits(0x477FFFFFu)) == 255u);
    CHECK(ptone::word(0.0f) == ptone::kDark && ptone::word(-0.0f) == ptone::kDark && ptone::word(-1.0f) == ptone::kDark);
    CHECK(ptone::word(from_bits(0x7F800000u)) == ptone::kInvalid && ptone::word(from_bits(0xFF800000u)) == ptone::kInvalid);
    CHECK(ptone::word(from_bits(0x7FC00000u)) == ptone::kInvalid && ptone::word(from_bits(0xFFC00001u)) == ptone::kInvalid);
    std::vector<uint32_t> hist(ptone::kWords, 0u);
    uint32_t n = 0;
    for (uint64_t b = 0; b <= 0xFFFFFFFFull; b += 65521u) {
        const uint32_t w = ptone::word(from_bits((uint32_t)b));
        CHECK(w < ptone::kWords);
        if (w < ptone::kWords) { ++hist[w]; ++n; }
    }
    uint64_t sum = 0;
    for (uint32_t v : hist) sum += v;
    CHECK(sum == n);
    // rules 2 and 3
    const float windows[][2] = {{0.f, 0.f}, {0.f, 1.f}, {0.5f, 0.95f}, {1.f, 1.f}, {0.3f, 0.3f}};
    for (const auto& w : windows) {
        const double t = ptone::meter(hist.data(), w[0], w[1], 0.18f, -8.f, 8.f, 0.1f, true, 0.0);
        CHECK(t >= -8.0 && t <= 8.0);
        const double u = ptone::meter(hist.data(), w[0], w[1], 0.18f, -8.f, 8.f, 0.5f, false, 2.0);
        CHECK(u == 2.0 + 0.5 * (t - 2.0));
    }
    std::vector<uint32_t> empty(ptone::kWords, 0u);
    empty[ptone::kDark] = 7u;
    CHECK(ptone::meter(empty.data(), 0.5f, 0.95f, 0.18f, -8.f, 8.f, 0.1f, true, 3.0) == 0.0);
    CHECK(ptone::meter(empty.data(), 0.5f, 0.95f, 0.18f, -8.f, 8.f, 0.1f, false, 3.0) == 3.0);
    std::vector<uint32_t> one(ptone::kWords, 0u);
    one[128] = 1u << 30;                                      // the largest image, one bin: centre 1/16
    CHECK(ptone::meter(one.data(), 0.5f, 0.95f, 1.0f, -8.f, 8.f, 0.1f, true, 0.0) == -(0.5 / 8.0));
    one[255] = 1u << 30; one[0] = 1u << 30;
    const double t3 = ptone::meter(one.data(), 0.0f, 1.0f, 1.0f, -20.f, 20.f, 0.1f, true, 0.0);
    CHECK(t3 > -0.1 && t3 < 0.1);
    // rules 5 and 6 on any bits
    for (uint32_t curve = 0; curve < 3; ++curve)
        for (uint64_t b = 0; b <= 0xFFFFFFFFull; b += 2654435u) {
            const float v = from_bits((uint32_t)b);
            const float c[3] = {v, 1.0f, from_bits((uint32_t)(b * 7u))};
            float y[3];
            ptone::curve(curve, 1.5f, 4.0f, c, y);
            CHECK(y[0] == y[0] && y[1] == y[1] && y[2] == y[2]);
            const uint32_t q0 = ptone::rgba8(ptone::kTransferSqrt, y), q1 = ptone::rgba8(ptone::kTransferSrgb, y);
            CHECK((q0 >> 24) == 255u && (q1 >> 24) == 255u);
        }
    const float ones[3] = {1.0f, 1.0f, 1.0f}, zeros[3] = {0.0f, -1.0f, from_bits(0x7FC00000u)};
    CHECK(ptone::rgba8(ptone::kTransferSrgb, ones) == 0xFFFFFFFFu && ptone::rgba8(ptone::kTransferSqrt, ones) == 0xFFFFFFFFu);
    CHECK(ptone::rgba8(ptone::kTransferSrgb, zeros) == 0xFF000000u && ptone::rgba8(ptone::kTransferSqrt, zeros) == 0xFF000000u);
    std::printf("tonemap_san: %d failed checks\n", failed);
    return failed != 0;
}
