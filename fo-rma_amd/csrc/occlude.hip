// occlude.hip — occlusion queries on the device (fr_ctx_occluded): one thread
// per ray answers "does anything of the scene lie in (kGbTMin, t_max) of this ray?" as one byte.
// The answer is the OR over every list primitive of its test against t_max itself (cast.h
// occl_walk_list), which is scene_walk with the AnyHit policy (scene_walk.h): no closest, no
// winner, no record, and a lane stops at its first accepted test. No scratch; no atomics but two
// adds per wave into the striped wave counter.
#include "scene_walk.h"
#include "tuning.h"

namespace fr {

struct OcclArgs {
  CastScene sc;
  const float4* rays;
  uint32_t n;
  uint32_t ranged;  // the ray's t_max is its second word's .w (FR_CAST_TMAX); 0: kCastTMax
  uint8_t* out;
  uint32_t* waves;
};

template <bool TREE>
__global__ __launch_bounds__(kCastBlock) void occlude_kernel(OcclArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x * kCastBlock + tid;
  // lanes past n walk with their wave on the batch's last ray and store nothing
  const bool inside = i < a.n;
  const size_t q = 2u * static_cast<size_t>(inside ? i : a.n - 1u);
  const float4 ro = a.rays[q], rd = a.rays[q + 1u];
  const GbRay r = cast_ray(V3{ro.x, ro.y, ro.z}, V3{rd.x, rd.y, rd.z});
  AnyHit<FR_OCCL_EXIT_EVERY> h(a.ranged ? rd.w : kCastTMax);
  const bool list_walk = scene_walk<TREE>(a.sc, r, tid, h);
  // per wave that holds a ray (its first lane has its lowest index): one add to the tree / list
  // word of the workgroup's stripe, one of the wave's occluded rays to the third word
  const uint32_t hits = __popcll(__ballot(h.occ & inside));
  if ((tid & 63u) == 0u && inside) {
    uint32_t* stripe = a.waves + (blockIdx.x % kCastStripes) * kCastStripeWords;
    atomicAdd(&stripe[list_walk ? 1u : 0u], 1u);
    atomicAdd(&stripe[2], hits);
  }
  if (inside) a.out[i] = h.occ ? 1u : 0u;  // a wave's 64 bytes: one line
}

hipError_t launch_occlude(hipStream_t stream, const CastScene& sc, bool tree, const float4* rays, uint32_t n, bool ranged,
                          uint8_t* out, uint32_t* waves) {
  if (!cast_scene_ok(sc, tree) || !rays || !n || !out || !waves) return hipErrorInvalidValue;
  const dim3 grid((n + kCastBlock - 1u) / kCastBlock), block(kCastBlock);
  const OcclArgs a{sc, rays, n, ranged ? 1u : 0u, out, waves};
  if (tree)
    hipLaunchKernelGGL(occlude_kernel<true>, grid, block, cast_lds_bytes(sc.levels), stream, a);
  else
    hipLaunchKernelGGL(occlude_kernel<false>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace fr
