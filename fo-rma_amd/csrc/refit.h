// refit.h — geometry edits in place: what the host refit (bvh.cpp bvh_refit),
// the packer (pack.cpp) and the device kernels (refit.hip) share. A moved primitive keeps its
// leaf slot; its records are rewritten and every box above it is recomputed from the slots'
// bounds. The tree's topology stays, which the walks' results do not depend on (bvh.h).
#pragma once

#include <stdint.h>

#include "bvh.h"

#if !defined(FR_HD)
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FR_HD __host__ __device__ __forceinline__
#else
#define FR_HD static inline
#endif
#endif

namespace fr {

// An unpadded box: a slot's bounds (prim_bounds at the scene's reach) or a node's union.
struct RefitBox {
  float lo[3];
  float pad0;
  float hi[3];
  float pad1;
};
static_assert(sizeof(RefitBox) == 32, "RefitBox is two float4");

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // slot_of: the primitive is in no leaf

// The empty box and the builder's compare-selects (bvh.cpp Box3::grow: std::min and std::max
// of a point, and a box as its two corners), so that host and device select alike, zero signs
// included.
FR_HD RefitBox refit_empty() {
  const float inf = __builtin_inff();
  return RefitBox{{inf, inf, inf}, 0.0f, {-inf, -inf, -inf}, 0.0f};
}
FR_HD void refit_grow(RefitBox& b, const float p[3]) {
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = p[k] < b.lo[k] ? p[k] : b.lo[k];
    b.hi[k] = b.hi[k] < p[k] ? p[k] : b.hi[k];
  }
}
FR_HD void refit_grow(RefitBox& b, const RefitBox& o) {
  refit_grow(b, o.lo);
  refit_grow(b, o.hi);
}

// A child's unpadded box: the union of a leaf's slots, or an internal child's own union.
FR_HD RefitBox refit_child(uint32_t ref, const RefitBox* slot_bounds, const RefitBox* unions) {
  if (ref < kBvhLeaf) return unions[ref];
  RefitBox b = refit_empty();
  const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u), count = ((ref >> kBvhSlotBits) & 15u) + 1u;
  for (uint32_t s = 0; s < count; ++s) refit_grow(b, slot_bounds[first + s]);
  return b;
}

// One node: both children's boxes padded into the builder's layout (Builder::build), and the
// node's own union for its parent.
FR_HD void refit_node(BvhNode& nd, RefitBox& un, const RefitBox* slot_bounds, const RefitBox* unions, float pad) {
  const RefitBox l = refit_child(nd.ref[0], slot_bounds, unions), r = refit_child(nd.ref[1], slot_bounds, unions);
  for (int k = 0; k < 3; ++k) {
    nd.a[k] = l.lo[k] - pad;
    nd.b[k] = l.hi[k] + pad;
  }
  nd.a[3] = r.lo[0] - pad;
  nd.b[3] = r.hi[0] + pad;
  nd.c[0] = r.lo[1] - pad;
  nd.c[1] = r.lo[2] - pad;
  nd.c[2] = r.hi[1] + pad;
  nd.c[3] = r.hi[2] + pad;
  un = refit_empty();
  refit_grow(un, l);
  refit_grow(un, r);
}

// One edited primitive as the host stages it for scene_patch_kernel.
struct PatchRow {
  uint32_t index;  // list index
  uint32_t pad[3];
  float rec[16];   // the 64-B record (pack.cpp pack_record)
  float lrec[16];  // the leaf record (a sphere's carries RN(r r))
  RefitBox bounds; // prim_bounds at the scene's reach (unused without a slot)
};
static_assert(sizeof(PatchRow) == 176, "PatchRow is eleven float4");

// The height schedule: node ids sorted by height (0: both children are leaves), and
// offset[h] .. offset[h + 1] the ids of height h. Heights stay below kBvhStack.
struct RefitSchedule {
  std::vector<uint32_t> ids;
  uint32_t offset[kBvhStack + 1] = {};
  uint32_t heights = 0;  // heights in use
};
RefitSchedule bvh_refit_schedule(const std::vector<BvhNode>& nodes);

// The host refit, the definition the kernel is held to: every node recomputed from the slots'
// bounds in the schedule's order. `unions` receives one box per node.
void bvh_refit(std::vector<BvhNode>& nodes, const RefitSchedule& sched, const std::vector<RefitBox>& slot_bounds,
               float pad, std::vector<RefitBox>& unions);

// prim_bounds (bvh.cpp) for callers outside the builder: the primitive's bounds from an empty
// box, `reach` as there (< 0: a sphere's own ball). False: no bounds (a stub, a plane, non-finite).
bool bvh_prim_bounds(const fr_prim& p, float reach, RefitBox* out);

#if defined(__HIPCC__) || defined(__HIP__)
// The device tables of one copy the kernels write (offsets into its blob: pack.h).
struct RefitTables {
  float4* rec;
  float4* lrec;
  BvhNode* nodes;
  RefitBox* slot_bounds;
  RefitBox* unions;
  const uint32_t* slot_of;
  const uint32_t* sched;
  uint32_t n, n_slots, n_nodes;  // primitives, leaf slots, nodes: the tables' lengths
};
// scene_patch_kernel over n staged rows (on the device), then one bvh_refit_kernel per height
// (none for a copy without a tree), all on `stream`. *launches: the refit launches made.
hipError_t launch_scene_patch(hipStream_t stream, const RefitTables& t, const PatchRow* rows, uint32_t n);
hipError_t launch_bvh_refit(hipStream_t stream, const RefitTables& t, const RefitSchedule& sched, float pad,
                            uint32_t* launches);
#endif

}  // namespace fr
