// lens_san.cpp -- the host-usable parts of pathtrace_amd/csrc/pt_lens.h under AddressSanitizer and UBSan: the setup with its
// refusals, and the per-sample rule (disc, ray) in a loop, with the properties the rule promises.  A stand-alone program:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined lens_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../pathtrace_amd/csrc/pt_lens.h"

struct HostMath {
    static float div(float a, float b) { return a / b; }
    static void sincos2pi(float u, float& s, float& c) {
        const double t = 6.283185307179586476925 * (double)u;
        s = (float)std::sin(t); c = (float)std::cos(t);
    }
};

static int failed = 0;
#define CHECK(cond) do { if (!(cond)) { ++failed; std::printf("FAILED %s (line %d)\n", #cond, __LINE__); } } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }
static float u01(uint32_t r) { return (float)(2u * (r >> 9) + 1u) / 16777216.0f; }

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double org[3] = {0.5, 0.25, 3.0}, ll[3] = {-0.3, -0.1, 2.0}, hor[3] = {1.6, 0.0, 0.0}, ver[3] = {0.0, 0.9, 0.0};
    const double zero[3] = {0.0, 0.0, 0.0}, bad[3] = {nan, 0.0, 0.0};
    ptlens::Setup s{}, untouched{};
    // ---- refusals: *out stays as it was
    for (double a : {-1.0, -1e-300, inf, -inf, nan}) CHECK(ptlens::setup(org, ll, hor, ver, a, 2.0, &untouched) == ptlens::kBadAperture);
    for (double f : {0.0, -2.0, inf, -inf, nan}) CHECK(ptlens::setup(org, ll, hor, ver, 0.3, f, &untouched) == ptlens::kBadFocus);
    CHECK(ptlens::setup(org, ll, zero, ver, 0.3, 2.0, &untouched) == ptlens::kBadCamera);
    CHECK(ptlens::setup(org, ll, hor, zero, 0.3, 2.0, &untouched) == ptlens::kBadCamera);
    CHECK(ptlens::setup(org, ll, bad, ver, 0.3, 2.0, &untouched) == ptlens::kBadCamera);
    CHECK(ptlens::setup(bad, ll, hor, ver, 0.3, 2.0, &untouched) == ptlens::kBadCamera);
    {   // D = 0: the screen centre is the origin
        const double c0[3] = {org[0] - 0.8, org[1] - 0.45, org[2]};
        CHECK(ptlens::setup(org, c0, hor, ver, 0.3, 2.0, &untouched) == ptlens::kBadCamera);
    }
    for (int k = 0; k < 3; ++k) CHECK(untouched.lu[k] == 0.0f && untouched.lv[k] == 0.0f);
    CHECK(untouched.inv_phi == 0.0f);
    // ---- the setup: C = (0, 0.1, -1), D = sqrt(1.01)
    CHECK(ptlens::setup(org, ll, hor, ver, 0.3, 2.0, &s) == ptlens::kOk);
    CHECK(s.lu[0] == 0.15f && s.lu[1] == 0.0f && s.lu[2] == 0.0f && s.lv[0] == 0.0f && s.lv[1] == 0.15f && s.lv[2] == 0.0f);
    CHECK(s.inv_phi == (float)(std::sqrt(1.01) / 2.0));
    ptlens::Setup pin{};
    CHECK(ptlens::setup(org, ll, hor, ver, 0.0, 1.0, &pin) == ptlens::kOk);
    for (int k = 0; k < 3; ++k) CHECK(pin.lu[k] == 0.0f && pin.lv[k] == 0.0f);
    // ---- the rule in a loop
    const float o32[3] = {(float)org[0], (float)org[1], (float)org[2]};
    uint32_t seed = 12345u;
    std::vector<float> keep;
    for (int i = 0; i < 200000; ++i) {
        const uint32_t w2 = i == 0 ? 0u : i == 1 ? 0xFFFFFFFFu : lcg(seed), w3 = i == 0 ? 0xFFFFFFFFu : i == 1 ? 0u : lcg(seed);
        float dx, dy;
        ptlens::disc<HostMath>(u01(w2), u01(w3), &dx, &dy);
        CHECK(std::isfinite(dx) && std::isfinite(dy));
        CHECK((double)dx * dx + (double)dy * dy <= 1.0 + 1e-6);
        const float dir[3] = {(float)(ll[0] + hor[0] * u01(lcg(seed)) - org[0]), (float)(ll[1] + ver[1] * u01(lcg(seed)) - org[1]), (float)(ll[2] - org[2])};
        float o[3], d[3];
        ptlens::ray(s, o32, dir, dx, dy, o, d);
        // |o' - origin| <= aperture / 2, and the ray passes origin + dir / inv_phi
        const double lx = (double)o[0] - o32[0], ly = (double)o[1] - o32[1], lz = (double)o[2] - o32[2];
        CHECK(std::sqrt(lx * lx + ly * ly + lz * lz) <= 0.15 * (1.0 + 1e-6));
        const double t = 1.0 / (double)s.inv_phi;
        for (int k = 0; k < 3; ++k) CHECK(std::fabs(((double)o[k] + t * d[k]) - ((double)o32[k] + t * dir[k])) <= 1e-5);
        // aperture 0: the pinhole ray, bit for bit
        ptlens::ray(pin, o32, dir, dx, dy, o, d);
        for (int k = 0; k < 3; ++k) CHECK(o[k] == o32[k] && d[k] == dir[k]);
        keep.push_back(d[0]);
    }
    std::printf("lens_san: %d failed checks (%zu rays)\n", failed, keep.size());
    return failed ? 1 : 0;
}
