// pt_film_probe_update.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_film_probe_vis.h"
#include "pt_probe_update.h"

// ------------------------------------------------------------------ irradiance volume: updates over frames (rule: pt_probe_update.h)
//   k_probe_update   one workgroup of kBlock threads per slot (probe first + slot stride).  Per block of kBlock rays every thread stages
//                    one ray in LDS, once: the rotated exact direction as three doubles and the clamped distance (8 KB), the three
//                    radiance values (3 KB).  Wave 0 then adds the staged rays to its 27 f64 SH sums in ptbake::sh_lane's order -- lane
//                    j takes the staged rays q = j, j + 64, ..., which are the rays r = q (mod 64) since a block starts at a multiple
//                    of 64 -- and the texel owners (tid < T T, with a visibility struct) run over all staged rays in ascending order
//                    through broadcast reads, as k_probe_moments does.  After the last block wave 0 runs the rule's tree through
//                    cross-lane moves and thread 0 puts the 27 new coefficients in LDS; every thread forms the probe's alpha from
//                    them and from the old DC coefficients and the age it read before the first barrier; threads < 27 blend the
//                    coefficients, the owners their texel, thread 0 writes the age.  Everything in place.  The barriers stand outside
//                    every divergent branch.  No scratch.
namespace PTK_IMPL {
__global__ void __launch_bounds__(kBlock) k_probe_update(ProbeUpdateArgs a) {
    __shared__ double s_ray[kBlock][4];
    __shared__ float s_rad[kBlock][3];
    __shared__ float s_new[27];
    static_assert(kBlock % ptbake::kLanes == 0, "a block of staged rays starts at a multiple of the lane count");
    static_assert(sizeof(ProbeUpdateRule) == sizeof(ptupd::Params), "ProbeUpdateRule is ptupd::Params");
    const ptupd::Params& u = reinterpret_cast<const ptupd::Params&>(a.u);
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, R = u.rays_per_probe, T = a.resolution;
    const uint32_t p = u.first + slot * u.stride;
    if (p >= a.n_probes) return;                      // (the whole workgroup; the host launches the slots that exist)
    const bool vis = a.distances != nullptr, identity = ptupd::is_identity(u.rotation);
    const bool owner = vis && tid < T * T, wave0 = tid < ptbake::kLanes;
    float* __restrict__ sh = a.sh27 + 27 * (size_t)p;
    const uint32_t age = a.age[p];
    const float old0[3] = {sh[0], sh[1], sh[2]};
    const uint32_t tj = tid / (T ? T : 1u), ti = tid - tj * T;
    double n[3], S[3] = {0.0, 0.0, 0.0}, acc[27];
    n[0] = n[1] = n[2] = 0.0;
    if (owner) ptvis::oct_decode(ptvis::centre(T, ti), ptvis::centre(T, tj), n);
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    const float* __restrict__ rad = a.radiance + 3 * (size_t)slot * R;
    const float* __restrict__ dist = vis ? a.distances + (size_t)slot * R : nullptr;
    for (uint32_t base = 0; base < R; base += kBlock) {
        const uint32_t r = base + tid;
        if (r < R) {
            ptupd::stage_ray(r, R, u.rotation, identity, vis, vis ? dist[r] : 0.0f, a.max_distance, s_ray[tid]);
            s_rad[tid][0] = rad[3 * (size_t)r]; s_rad[tid][1] = rad[3 * (size_t)r + 1]; s_rad[tid][2] = rad[3 * (size_t)r + 2];
        }
        __syncthreads();
        const uint32_t nq = R - base < kBlock ? R - base : kBlock;
        if (wave0)
            for (uint32_t q = tid; q < nq; q += ptbake::kLanes) ptupd::sh_add(s_ray[q], s_rad[q], acc);
        if (owner)
            for (uint32_t q = 0; q < nq; ++q) ptvis::add_ray(n, s_ray[q], a.sharpness_log2, S);
        __syncthreads();
    }
    if (wave0) {
#pragma unroll
        for (uint32_t h = ptbake::kLanes / 2; h >= 1u; h /= 2u) {
#pragma unroll
            for (int k = 0; k < 27; ++k) acc[k] = acc[k] + __shfl_down(acc[k], h, (int)ptbake::kLanes);
        }
        if (tid == 0u) {
#pragma unroll
            for (int k = 0; k < 27; ++k) s_new[k] = ptbake::sh_finish(acc[k], R);
        }
    }
    __syncthreads();
    const float new0[3] = {s_new[0], s_new[1], s_new[2]};
    const double alpha = ptupd::alpha(u, age, old0, new0);
    if (tid < 27u) sh[tid] = ptupd::blend(sh[tid], s_new[tid], alpha, age);
    if (owner) {
        float m[2];
        ptvis::finish(S, a.max_distance, m);
        float2* __restrict__ texel = reinterpret_cast<float2*>(a.moments) + (size_t)p * T * T + tid;
        const float2 old = *texel;
        *texel = make_float2(ptupd::blend(old.x, m[0], alpha, age), ptupd::blend(old.y, m[1], alpha, age));
    }
    if (tid == 0u) a.age[p] = ptupd::next_age(age);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_probe_update(const ProbeUpdateArgs& a, uint32_t n_upd, hipStream_t st) {
    if (n_upd) hipLaunchKernelGGL(PTK_IMPL::k_probe_update, dim3(n_upd), dim3(kBlock), 0, st, a);
}
}  // namespace ptk
