// Bounding volume hierarchy over a scene's primitives.
//
// A binary BVH whose nodes carry both children's boxes ("child boxes in the parent"):
// one 64-B fetch gives a lane two independent box tests; it steps into the nearer child
// it enters and keeps the other on a short per-lane stack in LDS. Leaves are referenced
// inline by the parent (first leaf slot, count) and their primitives' records are
// stored in leaf order, so a leaf costs no index hop. Used only as a conservative cull
// in front of the primitives' own tests; the closest-hit result is the same as the
// list-order loop (tracer.rs:195-200) because every primitive's candidate t does not
// depend on t_max and exact ties are broken by list index (render.hip, the BVH hit
// loop), whatever order the leaves are visited in.
#pragma once

#include <stdint.h>

#if !defined(__HIPCC_RTC__)  // the constants below are also read by the run-time kernel build
#include <math.h>

#include <vector>

#include "../../include/forma_rt.h"
#else
#include "forma_rt.h"
#endif

namespace fr {

// Child reference: an internal node index (< kBvhLeaf), a leaf
// kBvhLeaf | (count - 1) << kBvhSlotBits | first slot, or kBvhEnd.
constexpr uint32_t kBvhLeaf = 0x80000000u;
constexpr uint32_t kBvhEnd = 0xFFFFFFFFu;
constexpr uint32_t kBvhSlotBits = 27;      // leaf slots < 2^27
constexpr uint32_t kBvhLeafCountMax = 16;  // count field: 4 bits
constexpr uint32_t bvh_leaf_ref(uint32_t first, uint32_t count) {
  return kBvhLeaf | ((count - 1u) << kBvhSlotBits) | first;
}

struct BvhNode {
  float a[4];       // left lo x y z, right lo x
  float b[4];       // left hi x y z, right hi x
  float c[4];       // right lo y z, right hi y z
  uint32_t ref[2];  // left, right child
  uint32_t pad[2];
};
static_assert(sizeof(BvhNode) == 64, "BvhNode is four float4");

constexpr uint32_t kBvhLeafMax = 4;    // primitives per leaf of sphere-only lists (2 for others; more only for huge scenes)
// The in-order loop (wave-uniform, scalar loads) beats the per-lane walk only for small
// lists: weight box / sphere 1, oriented box 2, triangle 2.5. Measured at 1080p
// (tools/bvh_threshold.sh): 43 mixed prims (scene_01) 38 ms in order vs 55 BVH; 50
// spheres 6.4 vs 5.1; 50 oriented boxes 17.9 vs 9.4; 74 (scene_05) 32.6 vs 27.1.
constexpr uint32_t kBvhMinPrims = 48;  // smaller scenes keep the in-order loop
constexpr float kBvhMinCost = 48.0f;
// Traversal stack entries per lane (LDS). The builder keeps every internal node at
// depth < kBvhStack (median splits where SAH would go deeper), and a lane holds at most
// one entry per internal node on its current path.
constexpr uint32_t kBvhStack = 16;

// The closest-hit list cut at its planes: runs of consecutive non-plane primitives (one
// BVH each) and single planes, in list order. A plane hit ignores t_max and may leave
// a stale record (plane.rs:24-44), so planes are tested one by one where they stand.
struct BvhSegment {
  uint32_t plane;  // 1: a plane, prims index `prim`; 0: a run
  uint32_t root;   // run: root reference (kBvhEnd: nothing boundable)
  uint32_t pad;
  uint32_t prim;
};
static_assert(sizeof(BvhSegment) == 16, "BvhSegment is one uint4");

constexpr uint32_t kBvhMaxPlanes = 32;  // more planes: the in-order loop

#if !defined(__HIPCC_RTC__)
// Segments, nodes and the leaf-order primitive list (`order[slot]` = list index) for a
// scene; false if the scene is too small, has too many planes or is too large for the
// reference encoding. `force` drops the size and cost thresholds (A/B runs).
// `extent` (if given) receives the largest |coordinate| of any primitive's bounds: the
// boxes are padded by 1e-4 * (extent + 1).
bool build_segments(const std::vector<fr_prim>& prims, std::vector<BvhSegment>& segs, std::vector<BvhNode>& nodes,
                    std::vector<uint32_t>& order, bool force = false, float* extent = nullptr);
#endif

// Ray origins the node cull's slab arithmetic is conservative for:
// |o| <= kBvhOriginReach * (extent + 1) (the kernel's fused node slabs add |o| 2^-24 to a
// slab distance; the padding allows 2^24 * 1e-4 = 1677 times that). The reach of a scene is
// bvh_origin_reach below, which is shorter with spheres; a camera farther out renders with
// the in-order loop, and so does a wave with a scatter origin farther out.
constexpr float kBvhOriginReach = 100.0f;
// The node cull's reciprocal direction is clamped to [-kBvhInvClamp, kBvhInvClamp]: a
// zero direction component (inv = +-inf) would make fma(lo, inv, -o inv) NaN. A clamped
// slab is conservative while the hit's t is far below its width: a hit inside a box padded by
// >= 1e-4 (extent + 1) keeps that axis's slab >= 1e-4 (extent + 1) 2^100 wide about the
// origin, and a direction with one component of 2^-70 or more has every hit at
// t <= 101 (extent + 1) 2^70. A direction that is tiny in every component (hits at
// t ~ 2^100, clamped or not) takes the in-order loop: kBvhTinyDir, the kernel's list_walk
// ballot, which also sends an overflowing o inv (|o| >= 2^28 with a clamped component) there.
constexpr float kBvhInvClamp = 0x1p100f;
constexpr float kBvhTinyDir = 0x1p-70f;

#if !defined(__HIPCC_RTC__)
// The reach for a scene: kBvhOriginReach extents, less for a scene with spheres. The sphere
// test's discriminant b b - a c carries a rounding error of up to 15 * 2^-24 |o - c|^2 a
// (three-term dot products, the two products and the difference), so from far away it accepts
// rays that pass the sphere at a distance of up to sqrt(r^2 + E) with
// E = 2^-20 |o - c|^2, and the cull must not reject what the test accepts. Half of the padding
// covers that for |o - c|^2 <= 3 (|o| + extent)^2 while E <= r pad + pad^2 / 4, r the
// smallest radius. The reach is never set below extent + 1, because every scatter origin
// lies there and a shorter reach would switch the BVH off: that floor is a policy, not a
// bound. Where extent is more than about 10 r (the test lattices; 10,000 spheres of radius
// 2.5 over +-5000) the derived distance is below the floor, and inside the floor the test can
// still accept a far sphere by rounding error that the cull rejects. No frame of the suite
// shows it (such a far "hit" lies behind nearer ones almost always); closing it needs sphere
// bounds padded by the test's own error, which is not done here.
inline float bvh_origin_reach(float extent, float sphere_rmin) {
  const float unit = extent + 1.0f;
  float reach = kBvhOriginReach * unit;
  if (sphere_rmin >= 0.0f) {
    const float pad = 1e-4f * extent + 1e-4f;
    const float safe = sqrtf((sphere_rmin * pad + 0.25f * pad * pad) * (1048576.0f / 3.0f)) - extent;
    reach = fminf(reach, fmaxf(unit, safe));
  }
  return reach;
}
#endif

#if !defined(__HIPCC_RTC__)
// Largest internal-node depth of the trees (root = 0): below kBvhStack by construction.
uint32_t bvh_max_depth(const std::vector<BvhSegment>& segs, const std::vector<BvhNode>& nodes);
#endif

}  // namespace fr
