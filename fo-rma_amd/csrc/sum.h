// sum.h — the launch of sum_kernel (csrc/sum.hip): the per-pixel, in-sample-order sum
// of a pass's sample records (tracer.rs:170-184), and its workgroup size.
//
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"

namespace fr {

constexpr uint32_t kSumThreads = 256;

// An accumulating frame's resolve (FR_FLAG_ACCUMULATE): launch arguments of the accumulating
// sum kernels, which only a frame's last pass runs.
struct SumAccum {
  float* accum = nullptr;  // A: 3 f32 per pixel slot of the shard, indexed like `running`
  bool start = false;      // A = S (a new accumulation), else A = A + S
  float divisor = 1.0f;    // (float)n, the samples per pixel A holds after this frame
  // FR_FLAG_ACCUM_ERROR: Q, indexed like A; the resolve also does Q = S^2 / spp (start) or
  // Q = Q + S^2 / spp per channel (accum_error.h). Null: the frame carries no Q.
  float* sq = nullptr;
  // A tiled accumulation (fr_ctx_adapt): per shard tile, the samples and frames its pixels
  // hold. The resolve then divides by the tile's own count and advances both for the frame's
  // tiles (KParams::tile_list: an adaptive frame's list, else every tile); `divisor` is unused.
  uint32_t* n_t = nullptr;
  uint32_t* k_t = nullptr;
};

// wps: words per sample record (2 or 3); the record's form by KParams flags.
// acc: null for a plain frame; otherwise the last pass adds the frame's sum to acc->accum and
// writes accum / divisor instead of sum / spp.
hipError_t launch_sum(uint32_t wps, uint32_t blocks, hipStream_t stream, const KParams& kp,
                      const float* samples, float* running, float* out_mean, uint8_t* out_u8, int first, int last,
                      const float4* att, uint32_t n_prims, const SumAccum* acc = nullptr);

}  // namespace fr
