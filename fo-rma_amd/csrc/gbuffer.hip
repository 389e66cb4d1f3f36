// gbuffer.hip — the first-hit feature buffers on the device (fr_ctx_gbuffer):
// one thread per pixel casts the pinhole primary ray through the scene's list, in list order,
// and writes the winner's normal, root, point, index and attenuation as three 16-byte stores.
// The arithmetic is gbuffer.h's. The primitive index is wave-uniform, so every record arrives
// by scalar loads as in the trace kernel's list loop (rec_at). Scenes that have a tree take
// gbuffer_tree_kernel (cast.hip) from a camera within the tree's reach; this
// kernel is the pass for every other scene and camera. No atomics, no scratch, no LDS.
#include "gbuffer.h"

#include <type_traits>

#include "trace_kernel.h"  // RecRef, rec_at: a record through the constant address space

namespace fr {

struct GbArgs {
  GbScene sc;
  GbCam cam;
  uint32_t W, H;
  float4* g0;
  float4* g1;
  float4* alb;
};

__global__ __launch_bounds__(kGbTileW* kGbTileH) void gbuffer_kernel(GbArgs a) {
  const uint32_t x = blockIdx.x * kGbTileW + threadIdx.x;
  const uint32_t y = blockIdx.y * kGbTileH + threadIdx.y;
  // lanes past the image edge walk the list with their wave (the loop is wave-uniform) on the
  // ray of the last pixel of their row or column, and store nothing
  const bool inside = (x < a.W) & (y < a.H);
  const GbRay r = gb_primary_ray(a.cam, x < a.W ? x : a.W - 1u, y < a.H ? y : a.H - 1u, a.W, a.H);
  float closest = 3.40282347e+38f;
  int best = -1;
  auto test_one = [&](auto kind_tag, uint32_t i) {
    float t = 0.0f;
    if (gb_test<decltype(kind_tag)::value>(rec_at(a.sc.rec, i), r, closest, t)) {
      closest = t;
      best = static_cast<int>(i);
    }
  };
  // The list in order, as its kind runs (KScene::runs): one scalar kind branch per run.
  typedef __attribute__((address_space(4))) const uint32_t cu32;
  for (uint32_t rr = 0; rr < a.sc.n_runs; ++rr) {
    const cu32* rp = (cu32*)(reinterpret_cast<uintptr_t>(a.sc.runs)) + 4u * __builtin_amdgcn_readfirstlane(rr);
    const uint32_t k = rp[0], i0 = rp[1], i1 = rp[2];
    if (k == FR_AABB) {
      for (uint32_t i = i0; i < i1; ++i)
        test_one(std::integral_constant<uint32_t, FR_AABB>{}, __builtin_amdgcn_readfirstlane(i));
    } else if (k == FR_SPHERE) {
      for (uint32_t i = i0; i < i1; ++i)
        test_one(std::integral_constant<uint32_t, FR_SPHERE>{}, __builtin_amdgcn_readfirstlane(i));
    } else if (k == FR_PLANE) {
      for (uint32_t i = i0; i < i1; ++i)
        test_one(std::integral_constant<uint32_t, FR_PLANE>{}, __builtin_amdgcn_readfirstlane(i));
    } else if (k == FR_TRIANGLE) {
      for (uint32_t i = i0; i < i1; ++i)
        test_one(std::integral_constant<uint32_t, FR_TRIANGLE>{}, __builtin_amdgcn_readfirstlane(i));
    } else if (k == FR_OBB) {
      for (uint32_t i = i0; i < i1; ++i)
        test_one(std::integral_constant<uint32_t, FR_OBB>{}, __builtin_amdgcn_readfirstlane(i));
    }  // FR_STUB: never hits
  }
  if (!inside) return;
  GbPixel p = gb_miss();
  if (best >= 0) {
    // the winner's record, class and attenuation: per-lane loads, once per pixel
    const uint32_t b = static_cast<uint32_t>(best);
    struct Rec {
      float4 v[4];
      __device__ __forceinline__ float4 operator[](int k) const { return v[k]; }
    };
    const float4* rb = a.sc.rec + 4u * static_cast<size_t>(b);
    const Rec rec{{rb[0], rb[1], rb[2], rb[3]}};
    p = gb_hit(b, __float_as_uint(rec.v[3].w), a.sc.cls[b], rec, a.sc.att[b], r, closest);
  }
  const size_t i = static_cast<size_t>(y) * a.W + x;
  a.g0[i] = make_float4(p.g0.x, p.g0.y, p.g0.z, p.g0.w);
  a.g1[i] = make_float4(p.g1.x, p.g1.y, p.g1.z, p.g1.w);
  a.alb[i] = make_float4(p.alb.x, p.alb.y, p.alb.z, p.alb.w);
}

hipError_t launch_gbuffer(hipStream_t stream, const GbScene& sc, const GbCam& cam, uint32_t W, uint32_t H, float4* g0,
                          float4* g1, float4* alb) {
  if (!sc.rec || !sc.runs || !sc.cls || !sc.att || !g0 || !g1 || !alb || !W || !H) return hipErrorInvalidValue;
  const dim3 grid((W + kGbTileW - 1u) / kGbTileW, (H + kGbTileH - 1u) / kGbTileH), block(kGbTileW, kGbTileH);
  hipLaunchKernelGGL(gbuffer_kernel, grid, block, 0, stream, GbArgs{sc, cam, W, H, g0, g1, alb});
  return hipGetLastError();
}

}  // namespace fr
