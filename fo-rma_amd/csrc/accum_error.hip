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
  const bool valid = q < kp.P && slot_xy<false>(kp, q, x, y);
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

// The same for a tiled accumulation (fr_ctx_adapt): fn and fk from the pixel's
// tile's own counts n_t and K_t (K_t >= 2: the counts start from an accumulation of two frames
// or more). A wave is one tile, so the butterfly's maximum is the tile's: with tile_pixels the
// wave's first lane also writes the tile's selection, its image pixels (1 to 64) if the tile is
// active (max rel > threshold as bits, or n_t < min_samples) and 0 if not. kp is the whole
// shard's (no tile list).
__global__ __launch_bounds__(kSumThreads) void adapt_error_kernel(KParams kp, const float* __restrict__ accum,
                                                                  const float* __restrict__ sq,
                                                                  const uint32_t* __restrict__ n_t,
                                                                  const uint32_t* __restrict__ k_t, float threshold,
                                                                  uint32_t min_samples, float* __restrict__ err_map,
                                                                  uint32_t* __restrict__ partials,
                                                                  uint32_t* __restrict__ tile_pixels) {
  __shared__ uint32_t wave_count[kErrWaves], wave_max[kErrWaves];
  const uint32_t t = threadIdx.x, q = blockIdx.x * kSumThreads + t;
  uint32_t x = 0, y = 0;
  const bool valid = q < kp.P && slot_xy<false>(kp, q, x, y);
  const uint32_t tile = q >> 6;
  const uint32_t n = q < kp.P ? n_t[tile] : 0u;
  float rel = 0.0f;
  if (valid) {
    const V3 a{accum[3 * q], accum[3 * q + 1], accum[3 * q + 2]};
    const V3 s{sq[3 * q], sq[3 * q + 1], sq[3 * q + 2]};
    rel = accum_rel_error(a, s, static_cast<float>(n), static_cast<float>(k_t[tile] - 1u));
    err_map[static_cast<size_t>(y) * kp.W + x] = rel;
  }
  const unsigned long long in_image = __ballot(valid);
  const unsigned long long done = __ballot(valid && rel <= threshold);
  uint32_t mx = __float_as_uint(rel);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, static_cast<uint32_t>(__shfl_xor(static_cast<int>(mx), d, 64)));
  if ((t & 63u) == 0) {
    wave_count[t >> 6] = static_cast<uint32_t>(__popcll(done));
    wave_max[t >> 6] = mx;
    if (tile_pixels && q < kp.P) {
      const bool active = mx > __float_as_uint(threshold) || n < min_samples;
      tile_pixels[tile] = active ? static_cast<uint32_t>(__popcll(in_image)) : 0u;
    }
  }
  __syncthreads();
  if (t == 0) {
    uint32_t c = 0, m = 0;
#pragma unroll
    for (uint32_t w = 0; w < kErrWaves; ++w) {
      c += wave_count[w];
      m = max(m, wave_max[w]);
    }
    partials[2 * blockIdx.x] = c;
    partials[2 * blockIdx.x + 1] = m;
  }
}

// One workgroup: the summary as accum_error_reduce forms it, then the active tile list, the
// tiles whose tile_pixels entry is not 0 in ascending order. Each round takes 256 consecutive
// tiles: a ballot and a popcount below the lane give a tile's place in its wave, the waves'
// totals (LDS) its place in the round, the rounds run in order. No atomics.
__global__ __launch_bounds__(256) void adapt_select_kernel(const uint32_t* __restrict__ partials, uint32_t groups,
                                                           const uint32_t* __restrict__ tile_pixels, uint32_t n_tiles,
                                                           uint32_t* __restrict__ list,
                                                           AdaptSummary* __restrict__ out) {
  __shared__ unsigned long long cnt[256];
  __shared__ uint32_t mxs[256];
  __shared__ uint32_t wave_n[4];
  const uint32_t t = threadIdx.x;
  unsigned long long n = 0;
  uint32_t m = 0;
  for (uint32_t g = t; g < groups; g += 256) {
    n += partials[2 * g];
    m = max(m, partials[2 * g + 1]);
  }
  cnt[t] = n;
  mxs[t] = m;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (t < h) {
      cnt[t] += cnt[t + h];
      mxs[t] = max(mxs[t], mxs[t + h]);
    }
    __syncthreads();
  }
  const unsigned long long converged = cnt[0];
  const uint32_t max_bits = mxs[0];
  __syncthreads();
  uint32_t base = 0;            // list entries of the rounds before (the same in every thread)
  unsigned long long px = 0;    // this thread's active tiles' pixels
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256) {
    const uint32_t tile = t0 + t;
    const uint32_t p = tile < n_tiles ? tile_pixels[tile] : 0u;
    const unsigned long long b = __ballot(p != 0u);
    if ((t & 63u) == 0) wave_n[t >> 6] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
      before += w < (t >> 6) ? wave_n[w] : 0u;
      total += wave_n[w];
    }
    if (p) {
      list[base + before + static_cast<uint32_t>(__popcll(b & ((1ull << (t & 63u)) - 1ull)))] = tile;
      px += p;
    }
    base += total;
    __syncthreads();  // wave_n is rewritten next round
  }
  cnt[t] = px;
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (t < h) cnt[t] += cnt[t + h];
    __syncthreads();
  }
  if (t == 0) {
    out->converged = converged;
    out->active_pixels = cnt[0];
    out->max_bits = max_bits;
    out->active_tiles = base;
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

hipError_t launch_adapt(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                        const uint32_t* n_t, const uint32_t* k_t, float threshold, uint32_t min_samples,
                        float* err_map, uint32_t* partials, uint32_t* tile_pixels, uint32_t* list,
                        AdaptSummary* adapt, ErrSummary* summary) {
  if (!accum || !sq || !n_t || !k_t || !err_map || !partials || kp.tile_list) return hipErrorInvalidValue;
  if (adapt ? (!tile_pixels || !list || summary) : !summary) return hipErrorInvalidValue;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  if (groups)
    hipLaunchKernelGGL(adapt_error_kernel, dim3(groups), dim3(kSumThreads), 0, stream, kp, accum, sq, n_t, k_t,
                       threshold, min_samples, err_map, partials, adapt ? tile_pixels : nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (adapt)
    hipLaunchKernelGGL(adapt_select_kernel, dim3(1), dim3(256), 0, stream, partials, groups, tile_pixels, kp.n_tiles,
                       list, adapt);
  else
    hipLaunchKernelGGL(accum_error_reduce, dim3(1), dim3(256), 0, stream, partials, groups, summary);
  return hipGetLastError();
}

}  // namespace fr
