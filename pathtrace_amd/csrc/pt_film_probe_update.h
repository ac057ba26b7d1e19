// pt_film_probe_update.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_film_probe_vis.h"
#include "pt_probe_update.h"

// ------------------------------------------------------------------ irradiance volume: updates over frames (rule: pt_probe_update.h)
//   k_probe_update   one workgroup of kBlock threads per slot (probe first + slot stride): probe_staged_rays (pt_film_probe_vis.h) with
//                    the SH sums of wave 0 and, with a visibility struct, the texel owners (tid < T T).  Wave 0 then runs the rule's
//                    tree (sh_wave_tree, pt_film_bake.h) and thread 0 puts the 27 new coefficients in LDS; every thread forms the
//                    probe's alpha from them and from the old DC coefficients and the age it read before the first barrier; threads
//                    < 27 blend the coefficients, the owners their texel, thread 0 writes the age.  Everything in place.  The
//                    barriers stand outside every divergent branch.  No scratch.
namespace PTK_IMPL {
__global__ void __launch_bounds__(kBlock) k_probe_update(ProbeUpdateArgs a) {
    __shared__ double s_ray[kBlock][4];
    __shared__ float s_rad[kBlock][3];
    __shared__ float s_new[27];
    const ptupd::Params& u = a.u;
    const uint32_t slot = blockIdx.x, tid = threadIdx.x, R = u.rays_per_probe, T = a.vis.resolution;
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
    probe_staged_rays<true>(R, u.rotation, identity, vis, vis ? a.distances + (size_t)slot * R : nullptr, a.vis.max_distance,
                            a.radiance + 3 * (size_t)slot * R, owner, n, a.vis.sharpness_log2, s_ray, s_rad, S, acc);
    if (wave0) {
        sh_wave_tree(acc);
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
        ptvis::finish(S, a.vis.max_distance, m);
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
