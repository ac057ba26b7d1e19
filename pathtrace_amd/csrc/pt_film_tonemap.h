// pt_film_tonemap.h -- part of the film unit: included by pt_kernels_film.hip and by nothing else.
#pragma once
#include "pt_kernels_scan.h"
#include "pt_tonemap.h"

// ------------------------------------------------------------------ auto-exposure and tone mapping (pt_tonemap_device)
// The rule is pt_tonemap.h and DESIGN.md 5k.  k_film_histogram reads the film once (12 B per pixel), k_exposure_meter is one
// wave, k_tonemap reads 12 B and writes 4 (+ 12 with the float plane) per pixel.  The exposure never visits the host: the
// meter leaves it in device words and k_tonemap reads it there.
namespace PTK_IMPL {
constexpr uint32_t kHistBlock = 1024;          // one workgroup per compute unit: few workgroups, few flushes
constexpr uint32_t kHistBatch = 4;             // pixels per thread whose loads are in flight together
constexpr uint32_t kHistRounds = 4;            // in-wave reduction: bins settled by one LDS add of a lane count before the rest add singly
// One word per lane and pixel into the workgroup's LDS histogram.  A wave's pixels fall into a few words on most films (a
// wall, the black background): in each of the first kHistRounds rounds the first lane still waiting broadcasts its word, the
// lanes that hold the same word are counted by a ballot and that lane adds the count; what is left after them -- a wave
// whose lanes all differ -- adds singly, without conflicts.  Integer counts: no order to depend on.
PT_DEV void hist_add(uint32_t* s_hist, bool have, uint32_t w, uint32_t lane) {
    unsigned long long todo = __ballot(have);
    for (uint32_t r = 0; r < kHistRounds && todo != 0ull; ++r) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t wf = (uint32_t)__shfl((int)w, first);
        const unsigned long long same = __ballot(have && w == wf);
        if (lane == (uint32_t)first) atomicAdd(&s_hist[wf], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&s_hist[w], 1u);
}
__global__ void __launch_bounds__(kHistBlock) k_film_histogram(const float* __restrict__ lin, uint32_t np, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[ptone::kWords];
    for (uint32_t k = threadIdx.x; k < ptone::kWords; k += kHistBlock) s_hist[k] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * kHistBlock;
    // (the loop's bounds are the workgroup's: every lane of a wave takes every ballot)
    for (uint64_t base = (uint64_t)blockIdx.x * kHistBlock; base < np; base += kHistBatch * stride) {
        uint32_t w[kHistBatch];
        bool have[kHistBatch];
#pragma unroll
        for (uint32_t k = 0; k < kHistBatch; ++k) {
            const uint64_t p = base + k * stride + threadIdx.x;
            have[k] = p < np;
            w[k] = 0u;
            if (have[k]) w[k] = ptone::word(ptone::lum(lin[3 * p], lin[3 * p + 1], lin[3 * p + 2]));
        }
#pragma unroll
        for (uint32_t k = 0; k < kHistBatch; ++k) hist_add(s_hist, have[k], w[k], lane);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < ptone::kWords; k += kHistBlock)
        if (s_hist[k] != 0u) atomicAdd(&hist[k], s_hist[k]);
}

// One wave: lane i holds bins 4 i .. 4 i + 3.  The ranks in front of a lane's bins come from an inclusive scan of the lane
// sums (integers, exact); the window sums are ptone::meter_lane per lane and six butterfly steps -- the order ptone::meter
// restates on the host --, and lane 0 writes the state.
__global__ void __launch_bounds__(64) k_exposure_meter(ExposureArgs a) {
    const uint32_t lane = threadIdx.x;
    uint32_t n[ptone::kBinsPerLane];
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t j = 0; j < ptone::kBinsPerLane; ++j) { n[j] = a.hist[ptone::kBinsPerLane * lane + j]; mine += n[j]; }
    uint32_t incl = mine;                          // (the words add up to W H <= 2^30: no overflow)
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += up;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    const double lo = (double)a.pct_lo * (double)total, hi = (double)a.pct_hi * (double)total;
    double s, w;
    uint32_t point;
    ptone::meter_lane(n, ptone::kBinsPerLane * lane, (uint64_t)(incl - mine), lo, hi, &s, &w, &point);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off); w += __shfl_xor(w, off);
        const uint32_t other = (uint32_t)__shfl_xor((int)point, off);
        point = other < point ? other : point;
    }
    if (lane != 0u) return;
    const ExposureState old = *a.state;
    const bool fresh = old.valid == 0u || old.width != a.width || old.height != a.height;
    ExposureState next{};
    next.log2E = ptone::adapt(total, s, w, point, a.key, a.log2_min, a.log2_max, a.adapt, fresh, old.log2E);
    next.E = ptone::exposure(next.log2E);
    next.valid = 1u; next.width = a.width; next.height = a.height;
    *a.state = next;
}

// One thread per pixel: curve and transfer.  The pixel's three floats are read before any is written: out_linear may be linear.
__global__ void __launch_bounds__(kBlock) k_tonemap(TonemapArgs a) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= a.np) return;
    const float E = a.e_dev ? *a.e_dev : a.e_manual;
    const float c[3] = {a.linear[3 * (size_t)p], a.linear[3 * (size_t)p + 1], a.linear[3 * (size_t)p + 2]};
    float y[3];
    ptone::curve(a.curve, E, a.white, c, y);
    if (a.out_linear) { a.out_linear[3 * (size_t)p] = y[0]; a.out_linear[3 * (size_t)p + 1] = y[1]; a.out_linear[3 * (size_t)p + 2] = y[2]; }
    *reinterpret_cast<uint32_t*>(a.out_rgba + 4 * (size_t)p) = ptone::rgba8(a.transfer, y);
}
}  // namespace PTK_IMPL
namespace ptk {
void launch_film_histogram(const float* linear, uint32_t np, uint32_t* hist, uint32_t n_cus, hipStream_t st) {
    const uint32_t need = (np + PTK_IMPL::kHistBlock - 1) / PTK_IMPL::kHistBlock;
    if (np) hipLaunchKernelGGL(PTK_IMPL::k_film_histogram, dim3(need < n_cus ? need : n_cus), dim3(PTK_IMPL::kHistBlock), 0, st, linear, np, hist);
}
void launch_exposure_meter(const ExposureArgs& a, hipStream_t st) { hipLaunchKernelGGL(PTK_IMPL::k_exposure_meter, dim3(1), dim3(64), 0, st, a); }
void launch_tonemap(const TonemapArgs& a, hipStream_t st) {
    if (a.np) hipLaunchKernelGGL(PTK_IMPL::k_tonemap, dim3((a.np + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
}
}  // namespace ptk
