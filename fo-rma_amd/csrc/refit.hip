// refit.hip — geometry edits in place on the device. scene_patch_kernel
// scatters the host's staged rows (refit.h PatchRow) into a scene copy's tables: one thread per
// edited primitive writes its 64-B record and, where it has a leaf slot, the leaf record and the
// slot's bounds. bvh_refit_kernel then recomputes every node from its children, one launch per
// tree height, lowest first: a thread forms both children's unpadded boxes (a leaf's from its
// slots' bounds, an internal child's from the union an earlier launch left), stores them padded in
// the builder's layout and leaves its own union for its parent. The arithmetic is refit.h's
// refit_node, the host refit's (bvh.cpp bvh_refit). Stream order between the launches is the only
// ordering: no workgroup waits for another, and there are no atomics.
#include <hip/hip_runtime.h>

#include "refit.h"

namespace fr {

constexpr uint32_t kRefitBlock = 256;

__global__ __launch_bounds__(kRefitBlock) void scene_patch_kernel(RefitTables t, const float4* __restrict__ rows,
                                                                  uint32_t n) {
  const uint32_t k = blockIdx.x * kRefitBlock + threadIdx.x;
  if (k >= n) return;
  const float4* row = rows + static_cast<size_t>(k) * (sizeof(PatchRow) / sizeof(float4));
  const uint32_t i = __float_as_uint(row[0].x);
  if (i >= t.n) return;
  float4* rec = t.rec + 4u * static_cast<size_t>(i);
  for (int w = 0; w < 4; ++w) rec[w] = row[1 + w];
  const uint32_t slot = t.slot_of[i];
  if (slot >= t.n_slots) return;  // kNoSlot: a plane, a stub, a list scene
  float4* lrec = t.lrec + 4u * static_cast<size_t>(slot);
  for (int w = 0; w < 4; ++w) lrec[w] = row[5 + w];
  float4* sb = reinterpret_cast<float4*>(t.slot_bounds + slot);
  sb[0] = row[9];
  sb[1] = row[10];
}

// The nodes sched[first .. first + count): one height of the schedule.
__global__ __launch_bounds__(kRefitBlock) void bvh_refit_kernel(RefitTables t, uint32_t first, uint32_t count, float pad) {
  const uint32_t k = blockIdx.x * kRefitBlock + threadIdx.x;
  if (k >= count) return;
  const uint32_t id = t.sched[first + k];
  if (id >= t.n_nodes) return;
  BvhNode nd = t.nodes[id];
  RefitBox un;
  refit_node(nd, un, t.slot_bounds, t.unions, pad);
  t.nodes[id] = nd;
  t.unions[id] = un;
}

hipError_t launch_scene_patch(hipStream_t stream, const RefitTables& t, const PatchRow* rows, uint32_t n) {
  if (!rows || !n || !t.rec || !t.slot_of) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scene_patch_kernel, dim3((n + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, stream, t,
                     reinterpret_cast<const float4*>(rows), n);
  return hipGetLastError();
}

hipError_t launch_bvh_refit(hipStream_t stream, const RefitTables& t, const RefitSchedule& sched, float pad,
                            uint32_t* launches) {
  *launches = 0;
  if (!t.nodes || !t.slot_bounds || !t.unions || !t.sched || sched.ids.size() != t.n_nodes) return hipErrorInvalidValue;
  for (uint32_t h = 0; h < sched.heights; ++h) {
    const uint32_t first = sched.offset[h], count = sched.offset[h + 1] - first;
    if (!count) continue;
    hipLaunchKernelGGL(bvh_refit_kernel, dim3((count + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, stream, t,
                       first, count, pad);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*launches;
  }
  return hipSuccess;
}

}  // namespace fr
