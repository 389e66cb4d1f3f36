// temporal.hip — temporal reuse of a progressive accumulation on the device (fr_ctx_temporal,
// DESIGN.md §4.5f): a reprojection kernel, once per new accumulation, gathers each pixel's prior
// from the previous view's totals through the G-buffers of both views; a prep kernel, every call,
// adds the prior to the live accumulation, keeps the totals as the view's history and writes the
// filter's pixel; with levels = 0 a finalise kernel writes the picture straight from prep. The
// arithmetic is temporal.h's. No atomics, no scratch, no LDS: the current view's words are
// coalesced 16-byte loads, a source is four 16-byte loads (G0, G1, TA, TQ) at one gathered
// address, and neighbouring pixels gather from neighbouring sources, so L2 carries the reuse.
#include "temporal.h"

#include "sum.h"           // kSumThreads: the slots of a prep workgroup, as the sum kernels'
#include "trace_kernel.h"  // slot_xy: the trace kernel's pixel-slot order

namespace fr {

constexpr uint32_t kTpTileW = 32, kTpTileH = 8;  // a workgroup: 32 x 8 pixels, as a denoise level's

__device__ __forceinline__ DnFeat tp_feat(float4 a, float4 b) {
  return DnFeat{V3{a.x, a.y, a.z}, a.w, V3{b.x, b.y, b.z}, __float_as_uint(b.w)};
}
__device__ __forceinline__ float4 tp_f4(GbF4 v) { return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ GbF4 tp_gbf4(float4 v) { return GbF4{v.x, v.y, v.z, v.w}; }

// The previous view's pixel j < W * H (tp_project's range).
struct TpHist {
  const float4* __restrict__ g0;
  const float4* __restrict__ g1;
  const float4* __restrict__ ta;
  const float4* __restrict__ tq;
  __device__ __forceinline__ void operator()(uint32_t j, DnFeat& f0, GbF4& a, GbF4& q) const {
    f0 = tp_feat(g0[j], g1[j]);
    a = tp_gbf4(ta[j]);
    q = tp_gbf4(tq[j]);
  }
};

__global__ __launch_bounds__(kTpTileW* kTpTileH) void temporal_reproject_kernel(
    TpCam cam, TpOpt opt, uint32_t W, uint32_t H, const float4* __restrict__ g0, const float4* __restrict__ g1,
    const uint32_t* __restrict__ cls, uint32_t n_prims, const float4* __restrict__ h_g0,
    const float4* __restrict__ h_g1, const float4* __restrict__ h_ta, const float4* __restrict__ h_tq,
    float4* __restrict__ prior_a, float4* __restrict__ prior_q, uint32_t* __restrict__ source,
    uint32_t* __restrict__ reason) {
  const uint32_t x = blockIdx.x * kTpTileW + threadIdx.x;
  const uint32_t y = blockIdx.y * kTpTileH + threadIdx.y;
  if (x >= W || y >= H) return;
  const uint32_t i = y * W + x;
  const DnFeat f = tp_feat(g0[i], g1[i]);
  // (an id past the table can only be a miss; the class of one is never read)
  const uint32_t c = f.id < n_prims ? cls[f.id] : static_cast<uint32_t>(SC_NONE);
  const TpPrior p = tp_reproject(cam, opt, f, c, W, H, TpHist{h_g0, h_g1, h_ta, h_tq});
  prior_a[i] = tp_f4(p.a);
  prior_q[i] = tp_f4(p.q);
  source[i] = p.source;
  reason[i] = p.reason;
}

// One thread per pixel slot q of the shard, in denoise_prep_kernel's order and with its counts.
template <bool GUIDED>
__global__ __launch_bounds__(kSumThreads) void temporal_prep_kernel(
    KParams kp, const float* __restrict__ accum, const float* __restrict__ sq, const uint32_t* __restrict__ n_t,
    const uint32_t* __restrict__ k_t, uint32_t n, uint32_t frames, const float4* __restrict__ prior_a,
    const float4* __restrict__ prior_q, float4* __restrict__ ta, float4* __restrict__ tq,
    const float4* __restrict__ g0, const float4* __restrict__ g1, const float4* __restrict__ alb, uint32_t demodulate,
    float4* __restrict__ out) {
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
  const TpTotals t = tp_totals(a, s, n, frames, tp_gbf4(prior_a[i]), tp_gbf4(prior_q[i]));
  ta[i] = tp_f4(t.a);
  tq[i] = tp_f4(t.q);
  DnPixel p;
  if (GUIDED) {
    const float4 al = alb[i];
    p = tp_prep_guided(t, tp_feat(g0[i], g1[i]), V3{al.x, al.y, al.z}, demodulate != 0u);
  } else {
    p = tp_prep(t, __float_as_uint(g1[i].w) == kGbMiss);
  }
  out[i] = make_float4(p.r, p.g, p.b, p.var);
}

// The last level's outputs without a level: one thread per image pixel.
__global__ __launch_bounds__(kTpTileW* kTpTileH) void temporal_finalise_kernel(
    uint32_t W, uint32_t H, const float4* __restrict__ in, const float4* __restrict__ alb, uint32_t demodulate,
    float* __restrict__ mean_rgb, uint8_t* __restrict__ rgb8, float* __restrict__ var) {
  const uint32_t x = blockIdx.x * kTpTileW + threadIdx.x;
  const uint32_t y = blockIdx.y * kTpTileH + threadIdx.y;
  if (x >= W || y >= H) return;
  const size_t i = static_cast<size_t>(y) * W + x;
  const float4 v = in[i];
  const DnPixel o{v.x, v.y, v.z, v.w};
  V3 m{o.r, o.g, o.b};
  if (alb) {
    const float4 al = alb[i];
    m = dn_remodulate(o, V3{al.x, al.y, al.z}, demodulate != 0u);
  }
  mean_rgb[3 * i] = m.x;
  mean_rgb[3 * i + 1] = m.y;
  mean_rgb[3 * i + 2] = m.z;
  rgb8[3 * i] = to_u8(m.x);
  rgb8[3 * i + 1] = to_u8(m.y);
  rgb8[3 * i + 2] = to_u8(m.z);
  var[i] = dn_var(o);
}

hipError_t launch_temporal_reproject(hipStream_t stream, const TpCam& cam, const TpOpt& opt, uint32_t W, uint32_t H,
                                     const float4* g0, const float4* g1, const uint32_t* cls, uint32_t n_prims,
                                     const float4* h_g0, const float4* h_g1, const float4* h_ta, const float4* h_tq,
                                     float4* prior_a, float4* prior_q, uint32_t* source, uint32_t* reason) {
  if (!g0 || !g1 || !h_g0 || !h_g1 || !h_ta || !h_tq || !prior_a || !prior_q || !source || !reason ||
      (n_prims && !cls))
    return hipErrorInvalidValue;
  if (static_cast<uint64_t>(W) * H > 0x7FFFFFFFull / 16u) return hipErrorInvalidValue;  // fr_ctx_gbuffer's limit
  if (!W || !H) return hipSuccess;
  const dim3 grid((W + kTpTileW - 1u) / kTpTileW, (H + kTpTileH - 1u) / kTpTileH), block(kTpTileW, kTpTileH);
  hipLaunchKernelGGL(temporal_reproject_kernel, grid, block, 0, stream, cam, opt, W, H, g0, g1, cls, n_prims, h_g0, h_g1,
                     h_ta, h_tq, prior_a, prior_q, source, reason);
  return hipGetLastError();
}

hipError_t launch_temporal_prep(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                                const uint32_t* n_t, const uint32_t* k_t, uint32_t n, uint32_t frames,
                                const float4* prior_a, const float4* prior_q, float4* ta, float4* tq, const float4* g0,
                                const float4* g1, const float4* alb, uint32_t demodulate, DnPixel* ping) {
  if (!accum || !sq || !prior_a || !prior_q || !ta || !tq || !ping || !g1 || kp.tile_list) return hipErrorInvalidValue;
  if ((n_t == nullptr) != (k_t == nullptr) || kp.shard_count != 1) return hipErrorInvalidValue;
  if ((g0 == nullptr) != (alb == nullptr)) return hipErrorInvalidValue;
  if (!kp.P || !kp.W || !kp.H) return hipSuccess;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  float4* out = reinterpret_cast<float4*>(ping);
  if (g0)
    hipLaunchKernelGGL(temporal_prep_kernel<true>, dim3(groups), dim3(kSumThreads), 0, stream, kp, accum, sq, n_t, k_t, n,
                       frames, prior_a, prior_q, ta, tq, g0, g1, alb, demodulate, out);
  else
    hipLaunchKernelGGL(temporal_prep_kernel<false>, dim3(groups), dim3(kSumThreads), 0, stream, kp, accum, sq, n_t, k_t,
                       n, frames, prior_a, prior_q, ta, tq, g0, g1, alb, demodulate, out);
  return hipGetLastError();
}

hipError_t launch_temporal_finalise(hipStream_t stream, uint32_t W, uint32_t H, const DnPixel* ping, const float4* alb,
                                    uint32_t demodulate, float* mean_rgb, uint8_t* rgb8, float* var) {
  if (!ping || !mean_rgb || !rgb8 || !var) return hipErrorInvalidValue;
  if (!W || !H) return hipSuccess;
  const dim3 grid((W + kTpTileW - 1u) / kTpTileW, (H + kTpTileH - 1u) / kTpTileH), block(kTpTileW, kTpTileH);
  hipLaunchKernelGGL(temporal_finalise_kernel, grid, block, 0, stream, W, H, reinterpret_cast<const float4*>(ping), alb,
                     demodulate, mean_rgb, rgb8, var);
  return hipGetLastError();
}

}  // namespace fr
