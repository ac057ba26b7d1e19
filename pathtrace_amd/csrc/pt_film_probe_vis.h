// pt_film_probe_vis.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_film_bake.h"         // (pt_bake.h: sh_add)
#include "pt_film_probe.h"        // the pixel tile
#include "pt_probe_update.h"      // ptupd::stage_ray; pt_probe_vis.h

// ------------------------------------------------------------------ irradiance volume: probe visibility (rule: pt_probe_vis.h)
//   k_probe_distances   one thread per probe ray of a chunk of whole probes: the hit's t, +inf where the id says miss.
//   probe_staged_rays   the pass of one workgroup of kBlock threads over a probe's R rays, for k_probe_moments and k_probe_update
//                       (pt_film_probe_update.h).  Per block of kBlock rays every thread, owner or not, stages the ray base + its
//                       index in LDS, once: the rule's direction under the rotation and the clamped distance (0 without distances)
//                       as four doubles (8 KB), with kSh the three radiance values too (3 KB).  With kSh wave 0 then adds the staged
//                       rays to its 27 f64 SH sums in ptbake::sh_lane's order -- lane j takes the staged rays q = j, j + 64, ...,
//                       which are the rays r = q (mod 64) since a block starts at a multiple of 64 -- and every texel owner runs
//                       over all staged rays in ascending order -- all lanes read the same LDS address, a broadcast -- into its
//                       three f64 sums.  The whole workgroup calls it: the barriers stand outside every divergent branch.
//   k_probe_moments     one workgroup of kBlock threads per probe; thread t < T T owns texel (t % T, t / T): probe_staged_rays under
//                       the identity, then finish.  No scratch.
//   k_probe_shade_vis   k_probe_shade with the visibility term: one thread per pixel on the denoiser's tile; a lit pixel gathers
//                       the 27 floats of its eight corners and, per corner, the four (m1, m2) taps of that probe's map (8-byte
//                       loads; the plane is 8-byte aligned).  An unlit pixel reads its fallback pixel, no probe and no moment.  The
//                       fallback may be the output plane: a thread reads its own 12 bytes before it writes them.
namespace PTK_IMPL {
__global__ void __launch_bounds__(kBlock) k_probe_distances(const int32_t* __restrict__ ids, const float* __restrict__ t, uint32_t n,
                                                            float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = ids[i] >= 0 ? t[i] : __builtin_inff();
}
// dist: the probe's float[R] (with_distance); rad: its float[R][3] (kSh); owner: the thread has a texel, of direction n and sums S; acc: a
// thread of wave 0's SH sums (kSh)
template <bool kSh>
PT_DEV void probe_staged_rays(uint32_t R, const float* rotation, bool identity, bool with_distance, const float* __restrict__ dist, float max_distance,
                              const float* __restrict__ rad, bool owner, const double n[3], uint32_t sharpness_log2, double (*s_ray)[4],
                              float (*s_rad)[3], double S[3], double acc[27]) {
    static_assert(kBlock % ptbake::kLanes == 0, "a block of staged rays starts at a multiple of the lane count");
    const uint32_t tid = threadIdx.x;
    for (uint32_t base = 0; base < R; base += kBlock) {
        const uint32_t r = base + tid;
        if (r < R) {
            ptupd::stage_ray(r, R, rotation, identity, with_distance, with_distance ? dist[r] : 0.0f, max_distance, s_ray[tid]);
            if (kSh) { s_rad[tid][0] = rad[3 * (size_t)r]; s_rad[tid][1] = rad[3 * (size_t)r + 1]; s_rad[tid][2] = rad[3 * (size_t)r + 2]; }
        }
        __syncthreads();
        const uint32_t nq = R - base < kBlock ? R - base : kBlock;
        if (kSh && tid < ptbake::kLanes)
            for (uint32_t q = tid; q < nq; q += ptbake::kLanes) ptbake::sh_add(s_ray[q], s_rad[q], acc);
        if (owner)
            for (uint32_t q = 0; q < nq; ++q) ptvis::add_ray(n, s_ray[q], sharpness_log2, S);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kBlock) k_probe_moments(ProbeMomentsArgs a) {
    __shared__ double s_ray[kBlock][4];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, T = a.vis.resolution, R = a.rays_per_probe;
    const bool owner = tid < T * T;
    const uint32_t tj = tid / T, ti = tid - tj * T;
    double n[3], S[3] = {0.0, 0.0, 0.0};
    ptvis::oct_decode(ptvis::centre(T, ti), ptvis::centre(T, tj), n);       // (a thread without a texel computes a direction nobody reads)
    const float identity[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    probe_staged_rays<false>(R, identity, true, true, a.distances + (size_t)p * R, a.vis.max_distance, nullptr, owner, n, a.vis.sharpness_log2, s_ray,
                             nullptr, S, nullptr);
    if (!owner) return;
    float m[2];
    ptvis::finish(S, a.vis.max_distance, m);
    reinterpret_cast<float2*>(a.moments)[(size_t)p * T * T + tid] = make_float2(m[0], m[1]);
}
__global__ void __launch_bounds__(kDnBx * kDnBy) k_probe_shade_vis(ProbeShadeArgs a, const float* __restrict__ moments, uint32_t resolution) {
    const uint32_t x = blockIdx.x * kDnBx + threadIdx.x, y = blockIdx.y * kDnBy + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float4 f0 = a.feat[2 * p], f1 = a.feat[2 * p + 1];
    const float rec[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
    float v[3];
    if (!ptvis::shade(a.grid, a.normal_bias, a.width, a.height, x, y, rec, a.cam, a.sh27, moments,
                      resolution, v)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = a.fallback ? a.fallback[3 * p + k] : 0.0f;
    }
    a.out_linear[3 * p] = v[0]; a.out_linear[3 * p + 1] = v[1]; a.out_linear[3 * p + 2] = v[2];
    if (a.out_rgba) *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * p) = ptgrid::rgba8(v);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_probe_distances(const int32_t* ids, const float* t, uint32_t n, float* out, hipStream_t st) {
    if (n) hipLaunchKernelGGL(PTK_IMPL::k_probe_distances, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, ids, t, n, out);
}
void launch_probe_moments(const ProbeMomentsArgs& a, hipStream_t st) {
    if (a.n_probes && a.rays_per_probe) hipLaunchKernelGGL(PTK_IMPL::k_probe_moments, dim3(a.n_probes), dim3(kBlock), 0, st, a);
}
void launch_probe_shade_vis(const ProbeShadeArgs& a, const float* moments, uint32_t resolution, hipStream_t st) {
    const dim3 g = dn_grid(a.width, a.height), b(PTK_IMPL::kDnBx, PTK_IMPL::kDnBy);
    hipLaunchKernelGGL(PTK_IMPL::k_probe_shade_vis, g, b, 0, st, a, moments, resolution);
}
}  // namespace ptk
