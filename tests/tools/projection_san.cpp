// projection_san.cpp -- pathtrace_amd/csrc/pt_projection.h under AddressSanitizer and UBSan: the setup with its refusals, and the
// per-sample rule of every kind over a grid of screen positions, with the properties the rule promises.  A stand-alone program:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined projection_san.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "../../pathtrace_amd/csrc/pt_projection.h"

static int failed = 0;
static long outside = 0;      // calls of sincos2pi outside (0, 1)
#define CHECK(...) do { if (!(__VA_ARGS__)) { ++failed; std::printf("FAILED %s (line %d)\n", #__VA_ARGS__, __LINE__); } } while (0)

struct HostMath {
    static float div(float a, float b) { return a / b; }
    static float sqrt(float x) { return std::sqrt(x); }
    static void sincos2pi(float u, float& s, float& c) {
        if (!(u > 0.0f && u < 1.0f)) ++outside;
        const double t = 6.283185307179586476925 * (double)u;
        s = (float)std::sin(t); c = (float)std::cos(t);
    }
};

template <int KIND>
static void walk(const ptproj::Setup& P, const float org[3], const float ll[3], const float hor[3], const float ver[3], uint32_t w, uint32_t h,
                 long* rays) {
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            for (int j = 0; j < 9; ++j) {
                // the jitter's extremes (an odd multiple of 2^-24) and its middle
                const float e = 1.0f / 16777216.0f, jit[3] = {e, 0.5f + e, 1.0f - e};
                float u, v, dir[3], o[3], d[3], a, b;
                ptproj::screen<HostMath>(org, ll, hor, ver, w, h, x, y, jit[j % 3], jit[j / 3], &u, &v, dir);
                const bool unnormalised = ptproj::ray<HostMath, KIND>(P, org, u, v, dir, o, d, &a, &b);
                CHECK(a == 2.0f * u - 1.0f && b == 2.0f * v - 1.0f);
                double len = 0.0;
                for (int k = 0; k < 3; ++k) { CHECK(std::isfinite(o[k]) && std::isfinite(d[k])); len += (double)d[k] * d[k]; }
                len = std::sqrt(len);
                CHECK(len > 0.0);
                if (KIND == ptproj::kOrthographic) {
                    CHECK(!unnormalised);
                    for (int k = 0; k < 3; ++k) CHECK(d[k] == P.w[k]);
                } else {
                    for (int k = 0; k < 3; ++k) CHECK(o[k] == org[k]);
                }
                if (KIND == ptproj::kPerspective) {
                    CHECK(unnormalised);
                    for (int k = 0; k < 3; ++k) CHECK(d[k] == dir[k]);
                }
                if (KIND == ptproj::kFisheye || KIND == ptproj::kEquirect) CHECK(std::fabs(len - 1.0) <= 1e-5);
                ++*rays;
            }
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double org[3] = {0.5, 0.25, 3.0}, ll[3] = {-0.25, -0.25, 2.0}, hor[3] = {1.5, 0.0, 0.0}, ver[3] = {0.0, 1.0, 0.0};
    const double zero[3] = {0.0, 0.0, 0.0}, bad[3] = {nan, 0.0, 0.0};
    ptproj::Setup s{}, untouched{};
    // ---- refusals: *out stays as it was
    for (uint32_t kind : {4u, 5u, 0xFFFFFFFFu}) CHECK(ptproj::setup(org, ll, hor, ver, kind, 0u, 180.0, &untouched) == ptproj::kBadKind);
    for (uint32_t kind = 0; kind < 4; ++kind) CHECK(ptproj::setup(org, ll, hor, ver, kind, 1u, 180.0, &untouched) == ptproj::kBadReserved);
    for (double f : {0.0, -2.0, 360.5, inf, -inf, nan}) CHECK(ptproj::setup(org, ll, hor, ver, ptproj::kFisheye, 0u, f, &untouched) == ptproj::kBadFov);
    for (uint32_t kind = 0; kind < 4; ++kind) {
        CHECK(ptproj::setup(org, ll, zero, ver, kind, 0u, 180.0, &untouched) == ptproj::kBadCamera);
        CHECK(ptproj::setup(org, ll, hor, zero, kind, 0u, 180.0, &untouched) == ptproj::kBadCamera);
        CHECK(ptproj::setup(org, ll, bad, ver, kind, 0u, 180.0, &untouched) == ptproj::kBadCamera);
        CHECK(ptproj::setup(bad, ll, hor, ver, kind, 0u, 180.0, &untouched) == ptproj::kBadCamera);
        const double c0[3] = {org[0] - 0.75, org[1] - 0.5, org[2]};      // |C| = 0: the screen centre is the origin
        CHECK(ptproj::setup(org, c0, hor, ver, kind, 0u, 180.0, &untouched) == ptproj::kBadCamera);
    }
    for (int k = 0; k < 3; ++k) CHECK(untouched.u[k] == 0.0f && untouched.v[k] == 0.0f && untouched.w[k] == 0.0f && untouched.c[k] == 0.0f);
    CHECK(untouched.aspect == 0.0f && untouched.fov720 == 0.0f);
    // ---- the setup: C = (0, 0, -1)
    CHECK(ptproj::setup(org, ll, hor, ver, ptproj::kFisheye, 0u, 360.0, &s) == ptproj::kOk);
    CHECK(s.u[0] == 1.0f && s.u[1] == 0.0f && s.u[2] == 0.0f && s.v[0] == 0.0f && s.v[1] == 1.0f && s.v[2] == 0.0f);
    CHECK(s.w[0] == 0.0f && s.w[1] == 0.0f && s.w[2] == -1.0f && s.c[2] == -1.0f);
    CHECK(s.aspect == (float)(1.0 / 1.5) && s.fov720 == 0.5f);
    // ---- the angle reduction: 0 and negative revolutions exactly, whole turns, and never a call outside (0, 1)
    {
        float sn, cs, sp, cp;
        ptproj::sincos_rev<HostMath>(0.0f, sn, cs);
        CHECK(sn == 0.0f && cs == 1.0f);
        ptproj::sincos_rev<HostMath>(-0.0f, sn, cs);
        CHECK(sn == 0.0f && cs == 1.0f);
        ptproj::sincos_rev<HostMath>(1.0f, sn, cs);
        CHECK(sn == 0.0f && cs == 1.0f);
        for (float r : {0.125f, 0.25f, 0.4999f, 0.5f, 0.75f, 1.25f, 1.5f}) {
            ptproj::sincos_rev<HostMath>(r, sp, cp);
            ptproj::sincos_rev<HostMath>(-r, sn, cs);
            CHECK(sn == -sp && cs == cp);
            CHECK(std::fabs((double)sp - std::sin(6.283185307179586 * r)) <= 1e-6 && std::fabs((double)cp - std::cos(6.283185307179586 * r)) <= 1e-6);
        }
    }
    // ---- every kind over a grid, the smallest image included (u reaches 2 there)
    const float o32[3] = {(float)org[0], (float)org[1], (float)org[2]}, l32[3] = {(float)ll[0], (float)ll[1], (float)ll[2]};
    const float h32[3] = {(float)hor[0], (float)hor[1], (float)hor[2]}, v32[3] = {(float)ver[0], (float)ver[1], (float)ver[2]};
    long rays = 0;
    const uint32_t sizes[3][2] = {{2u, 2u}, {37u, 23u}, {64u, 3u}};
    for (const auto& wh : sizes) {
        walk<ptproj::kPerspective>(s, o32, l32, h32, v32, wh[0], wh[1], &rays);
        walk<ptproj::kOrthographic>(s, o32, l32, h32, v32, wh[0], wh[1], &rays);
        walk<ptproj::kFisheye>(s, o32, l32, h32, v32, wh[0], wh[1], &rays);
        walk<ptproj::kEquirect>(s, o32, l32, h32, v32, wh[0], wh[1], &rays);
    }
    // ---- the centre of the screen: along Wv, bit for bit, for the fisheye (rho = 0) and the panorama
    {
        const float dir[3] = {0.0f, 0.0f, -1.0f};
        float o[3], d[3], a, b;
        CHECK(!ptproj::ray<HostMath, ptproj::kFisheye>(s, o32, 0.5f, 0.5f, dir, o, d, &a, &b));
        for (int k = 0; k < 3; ++k) CHECK(d[k] == s.w[k]);
        CHECK(ptproj::ray<HostMath, ptproj::kEquirect>(s, o32, 0.5f, 0.5f, dir, o, d, &a, &b));
        CHECK(a == 0.0f && b == 0.0f && d[0] == 0.0f && d[1] == 0.0f && d[2] == -1.0f);
        CHECK(ptproj::ray<HostMath, ptproj::kEquirect>(s, o32, 0.0f, 0.5f, dir, o, d, &a, &b));      // column 0: backwards
        CHECK(a == -1.0f && std::fabs(d[2] - 1.0f) <= 1e-6f && std::fabs(d[0]) <= 1e-6f);
    }
    CHECK(outside == 0);
    std::printf("projection_san: %d failed checks (%ld rays, %ld calls outside the domain)\n", failed, rays, outside);
    return failed ? 1 : 0;
}
