// gbuffer.hip — the first-hit feature buffers on the device (fr_ctx_gbuffer):
// one thread per pixel casts the pinhole primary ray through the scene's list, in list order
// (scene_walk<false>, scene_walk.h: a wave-uniform index, scalar record loads), and writes the
// winner's normal, root, point, index and attenuation as three 16-byte stores. Scenes that have
// a tree take gbuffer_tree_kernel (cast.hip) from a camera within the tree's
// reach; this kernel is the pass for every other scene and camera. No atomics, no scratch, no LDS.
#include "scene_walk.h"

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
  ClosestHit h;
  scene_walk<false>(CastScene{a.sc}, r, 0u, h);  // the list alone: no other table is read
  if (inside) cast_store(a.sc, r, h, static_cast<size_t>(y) * a.W + x, a.g0, a.g1, a.alb);
}

hipError_t launch_gbuffer(hipStream_t stream, const GbScene& sc, const GbCam& cam, uint32_t W, uint32_t H, float4* g0,
                          float4* g1, float4* alb) {
  if (!sc.rec || !sc.runs || !sc.cls || !sc.att || !g0 || !g1 || !alb || !W || !H) return hipErrorInvalidValue;
  const dim3 grid((W + kGbTileW - 1u) / kGbTileW, (H + kGbTileH - 1u) / kGbTileH), block(kGbTileW, kGbTileH);
  hipLaunchKernelGGL(gbuffer_kernel, grid, block, 0, stream, GbArgs{sc, cam, W, H, g0, g1, alb});
  return hipGetLastError();
}

}  // namespace fr
