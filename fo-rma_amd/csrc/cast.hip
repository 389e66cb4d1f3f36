// cast.hip — ray queries on the device (fr_ctx_cast): one thread per ray takes
// the closest hit of scene_walk (scene_walk.h: the scene's list, or its tree with TREE = true)
// and writes the winner as the G-buffer's three 16-byte words. cast_kernel<TREE, true> starts
// closest at the ray's own t_max (FR_CAST_TMAX) and is otherwise the same kernel.
// gbuffer_tree_kernel is the same walk with the pinhole ray of a pixel as the ray source.
// No scratch; no atomics but one add per wave into the cast's striped wave counter; dynamic LDS
// is the tree walk's stack (cast_lds_bytes).
#include "scene_walk.h"

namespace fr {

struct CastArgs {
  CastScene sc;
  const float4* rays;
  uint32_t n;
  float4* g0;
  float4* g1;
  float4* alb;
  uint32_t* waves;
};

// RANGED: the ray's t_max is its second word's .w (FR_CAST_TMAX); otherwise the word is not read.
template <bool TREE, bool RANGED = false>
__global__ __launch_bounds__(kCastBlock) void cast_kernel(CastArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x * kCastBlock + tid;
  // lanes past n walk with their wave on the batch's last ray and store nothing
  const bool inside = i < a.n;
  const size_t q = 2u * static_cast<size_t>(inside ? i : a.n - 1u);
  const float4 ro = a.rays[q], rd = a.rays[q + 1u];
  const GbRay r = cast_ray(V3{ro.x, ro.y, ro.z}, V3{rd.x, rd.y, rd.z});
  ClosestHit h(RANGED ? rd.w : kCastTMax);
  const bool list_walk = scene_walk<TREE>(a.sc, r, tid, h);
  // one add per wave that holds a ray (a wave's first lane has its lowest index)
  if ((tid & 63u) == 0u && inside)
    atomicAdd(&a.waves[(blockIdx.x % kCastStripes) * kCastStripeWords + (list_walk ? 1u : 0u)], 1u);
  if (inside) cast_store(a.sc.gb, r, h, i, a.g0, a.g1, a.alb);
}

struct GbTreeArgs {
  CastScene sc;
  GbCam cam;
  uint32_t W, H;
  float4* g0;
  float4* g1;
  float4* alb;
};

// A workgroup covers gbuffer_kernel's 32 x 8 pixels; a wave is one 8 x 8 tile of them, so that
// its rays meet the same nodes (two rows of 32, gbuffer_kernel's map, measured no faster:
// DESIGN.md §4.5g).
__global__ __launch_bounds__(kCastBlock) void gbuffer_tree_kernel(GbTreeArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const uint32_t lx = 8u * wave + (lane & 7u), ly = lane >> 3;
  const uint32_t x = blockIdx.x * kGbTileW + lx, y = blockIdx.y * kGbTileH + ly;
  // lanes past the image edge walk with their wave on the ray of the last pixel of their row or
  // column, and store nothing
  const bool inside = (x < a.W) & (y < a.H);
  const GbRay r = gb_primary_ray(a.cam, x < a.W ? x : a.W - 1u, y < a.H ? y : a.H - 1u, a.W, a.H);
  ClosestHit h;
  scene_walk<true>(a.sc, r, tid, h);
  if (inside) cast_store(a.sc.gb, r, h, static_cast<size_t>(y) * a.W + x, a.g0, a.g1, a.alb);
}

bool cast_scene_ok(const CastScene& sc, bool tree) {
  if (!sc.gb.rec || !sc.gb.runs || !sc.gb.cls || !sc.gb.att) return false;
  if (!tree) return true;
  return sc.bvh && sc.bvh_order && sc.lrec && sc.segs && sc.n_segs && sc.levels >= 1u && sc.levels <= kBvhStack;
}

hipError_t launch_cast(hipStream_t stream, const CastScene& sc, bool tree, const float4* rays, uint32_t n, float4* g0,
                       float4* g1, float4* alb, uint32_t* waves, bool ranged) {
  if (!cast_scene_ok(sc, tree) || !rays || !n || !g0 || !g1 || !alb || !waves) return hipErrorInvalidValue;
  const dim3 grid((n + kCastBlock - 1u) / kCastBlock), block(kCastBlock);
  const CastArgs a{sc, rays, n, g0, g1, alb, waves};
  if (tree && ranged)
    hipLaunchKernelGGL((cast_kernel<true, true>), grid, block, cast_lds_bytes(sc.levels), stream, a);
  else if (tree)
    hipLaunchKernelGGL((cast_kernel<true, false>), grid, block, cast_lds_bytes(sc.levels), stream, a);
  else if (ranged)
    hipLaunchKernelGGL((cast_kernel<false, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((cast_kernel<false, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_gbuffer_tree(hipStream_t stream, const CastScene& sc, const GbCam& cam, uint32_t W, uint32_t H, float4* g0,
                               float4* g1, float4* alb) {
  if (!cast_scene_ok(sc, true) || !g0 || !g1 || !alb || !W || !H) return hipErrorInvalidValue;
  static_assert(kGbTileW * kGbTileH == kCastBlock, "a workgroup is gbuffer_kernel's 32 x 8 pixels");
  const dim3 grid((W + kGbTileW - 1u) / kGbTileW, (H + kGbTileH - 1u) / kGbTileH), block(kCastBlock);
  hipLaunchKernelGGL(gbuffer_tree_kernel, grid, block, cast_lds_bytes(sc.levels), stream, GbTreeArgs{sc, cam, W, H, g0, g1, alb});
  return hipGetLastError();
}

}  // namespace fr
