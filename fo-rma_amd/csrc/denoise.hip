// denoise.hip — the variance-guided filter of a progressive accumulation on the device
// (fr_ctx_denoise): a prep kernel turns A, Q and the counts into one 16-byte
// pixel (r, g, b, var) per image pixel, then one kernel launch per a-trous level reads the
// ping buffer and writes the pong buffer; the last level also writes the mean, the u8 image
// and the variance map. The arithmetic is denoise.h's. No atomics, no scratch, no LDS: every
// tap of a 32-pixel row is one coalesced 16-byte load per lane, and L2 carries the reuse.
#include "denoise.h"

#include "sum.h"           // kSumThreads: the slots of a prep workgroup, as the sum kernels'
#include "trace_kernel.h"  // slot_xy: the trace kernel's pixel-slot order

namespace fr {

static_assert(sizeof(DnPixel) == 16, "one 16-byte load or store per pixel");

// One thread per pixel slot q of the shard (A and Q are indexed by it, 3 f32 each), in
// accum_error_kernel's order; the counts as adapt_error_kernel reads them, or the uniform
// pair when the accumulation is not tiled (n_t null).
__global__ __launch_bounds__(kSumThreads) void denoise_prep_kernel(KParams kp, const float* __restrict__ accum,
                                                                   const float* __restrict__ sq,
                                                                   const uint32_t* __restrict__ n_t,
                                                                   const uint32_t* __restrict__ k_t, uint32_t n,
                                                                   uint32_t frames, float4* __restrict__ out) {
  const uint32_t q = blockIdx.x * kSumThreads + threadIdx.x;
  uint32_t x = 0, y = 0;
  if (q >= kp.P || !slot_xy<false>(kp, q, x, y)) return;
  if (n_t) {
    n = n_t[q >> 6];
    frames = k_t[q >> 6];
  }
  const V3 a{accum[3 * q], accum[3 * q + 1], accum[3 * q + 2]};
  const V3 s{sq[3 * q], sq[3 * q + 1], sq[3 * q + 2]};
  const DnPixel p = dn_prep(a, s, static_cast<float>(n), static_cast<float>(frames - 1u));
  out[static_cast<size_t>(y) * kp.W + x] = make_float4(p.r, p.g, p.b, p.var);
}

struct DnFetch {
  const float4* __restrict__ in;
  int W;
  __device__ __forceinline__ DnPixel operator()(int x, int y) const {
    const float4 v = in[static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x)];
    return DnPixel{v.x, v.y, v.z, v.w};
  }
};

// One thread per image pixel, a 32 x 8 pixel workgroup: each wave covers two 32-pixel rows, and
// for every tap the 32 lanes of a row read 32 contiguous 16-byte pixels at any step.
template <bool LAST>
__global__ __launch_bounds__(kDnTileW* kDnTileH) void denoise_level_kernel(const float4* __restrict__ in,
                                                                           float4* __restrict__ out, int W, int H,
                                                                           int step, float k,
                                                                           float* __restrict__ mean_rgb,
                                                                           uint8_t* __restrict__ rgb8,
                                                                           float* __restrict__ var) {
  const int x = static_cast<int>(blockIdx.x * kDnTileW + threadIdx.x);
  const int y = static_cast<int>(blockIdx.y * kDnTileH + threadIdx.y);
  if (x >= W || y >= H) return;
  const DnPixel o = dn_level(DnFetch{in, W}, x, y, W, H, step, k);
  const size_t i = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
  out[i] = make_float4(o.r, o.g, o.b, o.var);
  if (LAST) {
    mean_rgb[3 * i] = o.r;
    mean_rgb[3 * i + 1] = o.g;
    mean_rgb[3 * i + 2] = o.b;
    rgb8[3 * i] = to_u8(o.r);
    rgb8[3 * i + 1] = to_u8(o.g);
    rgb8[3 * i + 2] = to_u8(o.b);
    var[i] = dn_var(o);
  }
}

hipError_t launch_denoise(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                          const uint32_t* n_t, const uint32_t* k_t, uint32_t n, uint32_t frames, uint32_t levels,
                          float k, DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8, float* var) {
  if (!accum || !sq || !ping || !pong || !mean_rgb || !rgb8 || !var || kp.tile_list) return hipErrorInvalidValue;
  if ((n_t == nullptr) != (k_t == nullptr) || kp.shard_count != 1 || levels < 1 || levels > kDnLevelsMax)
    return hipErrorInvalidValue;
  if (!kp.P || !kp.W || !kp.H) return hipSuccess;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  hipLaunchKernelGGL(denoise_prep_kernel, dim3(groups), dim3(kSumThreads), 0, stream, kp, accum, sq, n_t, k_t, n, frames,
                     reinterpret_cast<float4*>(ping));
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_denoise_levels(stream, kp.W, kp.H, levels, k, ping, pong, mean_rgb, rgb8, var);
}

hipError_t launch_denoise_levels(hipStream_t stream, uint32_t width, uint32_t height, uint32_t levels, float k,
                                 DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8, float* var) {
  if (!ping || !pong || !mean_rgb || !rgb8 || !var || levels < 1 || levels > kDnLevelsMax) return hipErrorInvalidValue;
  if (!width || !height) return hipSuccess;
  hipError_t e = hipSuccess;
  const dim3 grid((width + kDnTileW - 1u) / kDnTileW, (height + kDnTileH - 1u) / kDnTileH), block(kDnTileW, kDnTileH);
  const float4* in = reinterpret_cast<const float4*>(ping);
  float4* out = reinterpret_cast<float4*>(pong);
  const int W = static_cast<int>(width), H = static_cast<int>(height);
  for (uint32_t i = 0; i < levels && e == hipSuccess; ++i) {
    const int step = 1 << i;
    if (i + 1 == levels)
      hipLaunchKernelGGL(denoise_level_kernel<true>, grid, block, 0, stream, in, out, W, H, step, k, mean_rgb, rgb8, var);
    else
      hipLaunchKernelGGL(denoise_level_kernel<false>, grid, block, 0, stream, in, out, W, H, step, k, nullptr, nullptr,
                         nullptr);
    e = hipGetLastError();
    const float4* t = in;
    in = out;
    out = const_cast<float4*>(t);
  }
  return e;
}

// ---- the feature-guided filter (fr_ctx_denoise_guided) ----------------

struct DnFeatFetch {
  const float4* __restrict__ g0;
  const float4* __restrict__ g1;
  int W;
  __device__ __forceinline__ DnFeat operator()(int x, int y) const {
    const size_t i = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
    const float4 a = g0[i], b = g1[i];
    return DnFeat{V3{a.x, a.y, a.z}, a.w, V3{b.x, b.y, b.z}, __float_as_uint(b.w)};
  }
};

// denoise_prep_kernel with the pixel's features and albedo (indexed by image pixel, y * W + x).
__global__ __launch_bounds__(kSumThreads) void denoise_prep_guided_kernel(
    KParams kp, const float* __restrict__ accum, const float* __restrict__ sq, const uint32_t* __restrict__ n_t,
    const uint32_t* __restrict__ k_t, uint32_t n, uint32_t frames, const float4* __restrict__ g0,
    const float4* __restrict__ g1, const float4* __restrict__ alb, uint32_t demodulate, float4* __restrict__ out) {
  const uint32_t q = blockIdx.x * kSumThreads + threadIdx.x;
  uint32_t x = 0, y = 0;
  if (q >= kp.P || !slot_xy<false>(kp, q, x, y)) return;
  if (n_t) {
    n = n_t[q >> 6];
    frames = k_t[q >> 6];
  }
  const V3 a{accum[3 * q], accum[3 * q + 1], accum[3 * q + 2]};
  const V3 s{sq[3 * q], sq[3 * q + 1], sq[3 * q + 2]};
  const size_t i = static_cast<size_t>(y) * kp.W + x;
  const float4 al = alb[i];
  const DnFeat f = DnFeatFetch{g0, g1, static_cast<int>(kp.W)}(static_cast<int>(x), static_cast<int>(y));
  const DnPixel p = dn_prep_guided(a, s, static_cast<float>(n), static_cast<float>(frames - 1u), f,
                                   V3{al.x, al.y, al.z}, demodulate != 0u);
  out[i] = make_float4(p.r, p.g, p.b, p.var);
}

// denoise_level_kernel's shape; per tap three independent coalesced 16-byte loads: the pixel,
// G0 and G1.
template <bool LAST>
__global__ __launch_bounds__(kDnTileW* kDnTileH) void denoise_level_guided_kernel(
    const float4* __restrict__ in, float4* __restrict__ out, const float4* __restrict__ g0,
    const float4* __restrict__ g1, const float4* __restrict__ alb, int W, int H, int step, float k, float sigma_z,
    uint32_t normal_pow2, uint32_t demodulate, float* __restrict__ mean_rgb, uint8_t* __restrict__ rgb8,
    float* __restrict__ var) {
  const int x = static_cast<int>(blockIdx.x * kDnTileW + threadIdx.x);
  const int y = static_cast<int>(blockIdx.y * kDnTileH + threadIdx.y);
  if (x >= W || y >= H) return;
  const DnPixel o = dn_level_guided(DnFetch{in, W}, DnFeatFetch{g0, g1, W}, x, y, W, H, step, k, sigma_z, normal_pow2);
  const size_t i = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
  out[i] = make_float4(o.r, o.g, o.b, o.var);
  if (LAST) {
    const float4 al = alb[i];
    const V3 m = dn_remodulate(o, V3{al.x, al.y, al.z}, demodulate != 0u);
    mean_rgb[3 * i] = m.x;
    mean_rgb[3 * i + 1] = m.y;
    mean_rgb[3 * i + 2] = m.z;
    rgb8[3 * i] = to_u8(m.x);
    rgb8[3 * i + 1] = to_u8(m.y);
    rgb8[3 * i + 2] = to_u8(m.z);
    var[i] = dn_var(o);
  }
}

hipError_t launch_denoise_guided(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                                 const uint32_t* n_t, const uint32_t* k_t, uint32_t n, uint32_t frames,
                                 uint32_t levels, float k, const DnGuide& guide, const float4* g0, const float4* g1,
                                 const float4* alb, DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8,
                                 float* var) {
  if (!accum || !sq || !ping || !pong || !mean_rgb || !rgb8 || !var || !g0 || !g1 || !alb || kp.tile_list)
    return hipErrorInvalidValue;
  if ((n_t == nullptr) != (k_t == nullptr) || kp.shard_count != 1 || levels < 1 || levels > kDnLevelsMax ||
      guide.normal_pow2 > kDnNormalPow2Max)
    return hipErrorInvalidValue;
  if (!kp.P || !kp.W || !kp.H) return hipSuccess;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  hipLaunchKernelGGL(denoise_prep_guided_kernel, dim3(groups), dim3(kSumThreads), 0, stream, kp, accum, sq, n_t, k_t, n,
                     frames, g0, g1, alb, guide.demodulate, reinterpret_cast<float4*>(ping));
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e
                         : launch_denoise_guided_levels(stream, kp.W, kp.H, levels, k, guide, g0, g1, alb, ping, pong,
                                                        mean_rgb, rgb8, var);
}

hipError_t launch_denoise_guided_levels(hipStream_t stream, uint32_t width, uint32_t height, uint32_t levels, float k,
                                        const DnGuide& guide, const float4* g0, const float4* g1, const float4* alb,
                                        DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8, float* var) {
  if (!ping || !pong || !mean_rgb || !rgb8 || !var || !g0 || !g1 || !alb || levels < 1 || levels > kDnLevelsMax ||
      guide.normal_pow2 > kDnNormalPow2Max)
    return hipErrorInvalidValue;
  if (!width || !height) return hipSuccess;
  hipError_t e = hipSuccess;
  const dim3 grid((width + kDnTileW - 1u) / kDnTileW, (height + kDnTileH - 1u) / kDnTileH), block(kDnTileW, kDnTileH);
  const float4* in = reinterpret_cast<const float4*>(ping);
  float4* out = reinterpret_cast<float4*>(pong);
  const int W = static_cast<int>(width), H = static_cast<int>(height);
  for (uint32_t i = 0; i < levels && e == hipSuccess; ++i) {
    const int step = 1 << i;
    if (i + 1 == levels)
      hipLaunchKernelGGL(denoise_level_guided_kernel<true>, grid, block, 0, stream, in, out, g0, g1, alb, W, H, step, k,
                         guide.sigma_z, guide.normal_pow2, guide.demodulate, mean_rgb, rgb8, var);
    else
      hipLaunchKernelGGL(denoise_level_guided_kernel<false>, grid, block, 0, stream, in, out, g0, g1, alb, W, H, step, k,
                         guide.sigma_z, guide.normal_pow2, guide.demodulate, nullptr, nullptr, nullptr);
    e = hipGetLastError();
    const float4* t = in;
    in = out;
    out = const_cast<float4*>(t);
  }
  return e;
}

}  // namespace fr
