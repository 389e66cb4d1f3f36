// accum_error.hip — the error estimate of a progressive accumulation on demand
// (fr_ctx_accum_error): one kernel turns the accumulators A and Q into a
// per-pixel relative standard error (accum_error.h) and per-workgroup partials of the summary,
// a second one-workgroup kernel adds the partials up. Integer counts and a maximum over bit
// patterns, no float atomics: the summary is bitwise reproducible.
#include "accum_error.h"

#include "sum.h"           // kSumThreads: the slots of a workgroup, as the sum kernels'
#include "trace_kernel.h"  // slot_xy: the trace kernel's pixel-slot order

namespace fr {

constexpr uint32_t kErrWaves = kSumThreads / 64u;
static_assert(kSumThreads % 64u == 0, "whole waves");

// One thread per pixel slot q of the shard (A and Q are indexed by it, 3 f32 each). rel >= 0
// and never NaN, so the maximum is taken over its bits as uint32; slots past the image edge
// count nothing and contribute 0 to the maximum.
__global__ __launch_bounds__(kSumThreads) void accum_error_kernel(KParams kp, const float* __restrict__ accum,
                                                                  const float* __restrict__ sq, float fn, float fk,
                                                                  float threshold, float* __restrict__ err_map,
                                                                  uint32_t* __restrict__ partials) {
  __shared__ uint32_t wave_count[kErrWaves], wave_max[kErrWaves];
  const uint32_t t = threadIdx.x, q = blockIdx.x * kSumThreads + t;
  uint32_t x = 0, y = 0;
  const bool valid = q < kp.P && slot_xy(kp, q, x, y);
  float rel = 0.0f;
  if (valid) {
    const V3 a{accum[3 * q], accum[3 * q + 1], accum[3 * q + 2]};
    const V3 s{sq[3 * q], sq[3 * q + 1], sq[3 * q + 2]};
    rel = accum_rel_error(a, s, fn, fk);
    err_map[static_cast<size_t>(y) * kp.W + x] = rel;
  }
  // per wave: the count by ballot and popcount, the maximum by a butterfly over the lanes
  const unsigned long long done = __ballot(valid && rel <= threshold);
  uint32_t mx = __float_as_uint(rel);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, static_cast<uint32_t>(__shfl_xor(static_cast<int>(mx), d, 64)));
  if ((t & 63u) == 0) {
    wave_count[t >> 6] = static_cast<uint32_t>(__popcll(done));
    wave_max[t >> 6] = mx;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t n = 0, m = 0;
#pragma unroll
    for (uint32_t w = 0; w < kErrWaves; ++w) {
      n += wave_count[w];
      m = max(m, wave_max[w]);
    }
    partials[2 * blockIdx.x] = n;
    partials[2 * blockIdx.x + 1] = m;
  }
}

// Adds the workgroups' partials up (one workgroup, as reduce_counters): integer sum and max,
// so the order of the additions does not show.
__global__ __launch_bounds__(256) void accum_error_reduce(const uint32_t* __restrict__ partials, uint32_t groups,
                                                          ErrSummary* __restrict__ out) {
  __shared__ unsigned long long cnt[256];
  __shared__ uint32_t mxs[256];
  unsigned long long n = 0;
  uint32_t m = 0;
  for (uint32_t g = threadIdx.x; g < groups; g += 256) {
    n += partials[2 * g];
    m = max(m, partials[2 * g + 1]);
  }
  cnt[threadIdx.x] = n;
  mxs[threadIdx.x] = m;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      cnt[threadIdx.x] += cnt[threadIdx.x + h];
      mxs[threadIdx.x] = max(mxs[threadIdx.x], mxs[threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out->converged = cnt[0];
    out->max_bits = mxs[0];
    out->pad = 0;
  }
}

hipError_t launch_accum_error(hipStream_t stream, const KParams& kp, const float* accum, const float* sq, float fn,
                              float fk, float threshold, float* err_map, uint32_t* partials, ErrSummary* summary) {
  if (!accum || !sq || !err_map || !partials || !summary) return hipErrorInvalidValue;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  if (groups)
    hipLaunchKernelGGL(accum_error_kernel, dim3(groups), dim3(kSumThreads), 0, stream, kp, accum, sq, fn, fk, threshold,
                       err_map, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(accum_error_reduce, dim3(1), dim3(256), 0, stream, partials, groups, summary);
  return hipGetLastError();
}

}  // namespace fr
