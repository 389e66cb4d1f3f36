// sum.h — the launch of sum_kernel (csrc/sum.hip): the per-pixel, in-sample-order sum
// of a pass's sample records (tracer.rs:170-184), and its workgroup size.
//
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kparams.h"

namespace fr {

constexpr uint32_t kSumThreads = 256;

// wps: words per sample record (2 or 3); the record's form by KParams flags.
hipError_t launch_sum(uint32_t wps, uint32_t blocks, hipStream_t stream, const KParams& kp,
                      const float* samples, float* running, float* out_mean, uint8_t* out_u8, int first, int last,
                      const float4* att, uint32_t n_prims);

}  // namespace fr
