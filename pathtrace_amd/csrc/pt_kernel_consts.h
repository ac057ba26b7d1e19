// pt_kernel_consts.h -- the constants of the kernels (pt_kernels.h) that the launch sizing (pt_shape.h) needs too.  No HIP: the
// sizing builds with a plain host compiler.
#pragma once
#include <stdint.h>

namespace ptk {

constexpr uint32_t kBlock = 256;
// Scenes of at most kSmallObjs objects stay whole in LDS (scan + shape + material + run
// records: at most 9 float4 per object = 18 KiB); larger scenes stream their scan array
// through one LDS tile and gather shape/material records from global memory.
constexpr uint32_t kSmallObjs = 128;
// SceneView::spheres_only holds for scenes of at most this many spheres (and nothing else): k_paths_regen<MIS, diffuse> then walks
// the scan array as spheres 0 .. n - 1 without the run records (pt_kernels_scan.h)
constexpr uint32_t kSpheresOnlyMax = 16;
// occupancy k_paths_regen is compiled for (waves per SIMD = workgroups per CU): the host launches exactly that many
#ifndef PT_REGEN_WAVES_DIFFUSE
#define PT_REGEN_WAVES_DIFFUSE 6
#endif
#ifndef PT_REGEN_WAVES_SPLIT
#define PT_REGEN_WAVES_SPLIT 5
#endif
constexpr uint32_t kRegenWavesDiffuse = PT_REGEN_WAVES_DIFFUSE, kRegenWavesGeneric = 5, kRegenWavesSplit = PT_REGEN_WAVES_SPLIT;
// k_paths_regen_split: float4 of exchange memory per wave of the launch: 128 stack entries of 5 float4
constexpr uint32_t kRegenSplitF4PerWave = 128u * 5u;
// chunk counters of k_paths_regen: chunk_counter[c * kRegenCounterStride], c < kRegenCounters (256 bytes apart)
constexpr uint32_t kRegenCounters = 8, kRegenCounterStride = 64;

}  // namespace ptk
