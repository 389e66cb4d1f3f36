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
// `extent` (if given) receives the largest |coordinate| of any primitive's own bounds: the
// boxes are padded by 1e-4 * (extent + 1), and a sphere is bounded by bvh_sphere_bound at the
// scene's reach (bvh_origin_reach of that extent and the smallest radius).
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
// origin, and a direction with one component of 2^-60 or more has every hit at
// t <= 101 (extent + 1) 2^60. A direction that is tiny in every component takes the in-order
// loop: kBvhTinyDir, the kernel's list_walk ballot, which also sends an overflowing o inv
// (|o| >= 2^28 with a clamped component) there. The limit is 2^-60 and not the 2^-70 the clamp
// alone would allow because of the sphere test: below it dot(d, d) < 2^-120 and the products of
// the discriminant lose their relative accuracy to underflow (at |d| ~ 2^-69 b b and a c are
// denormals of a few ulps and the test accepts rays that pass a sphere far outside any
// padding). At 2^-60 the underflow is bounded by kSphereDiscAbs below.
constexpr float kBvhInvClamp = 0x1p100f;
constexpr float kBvhTinyDir = 0x1p-60f;

#if !defined(__HIPCC_RTC__)
// What the sphere test accepts, and the bounds that follow from it. sphere_root_rr (rt_core.h)
// accepts when RN(b b) > RN(a cc) (the difference of two floats has its exact sign), with
// oc = RN(o - c), b = dot(oc, d), cc = RN(dot(oc, oc) - rr), a = dot(d, d), every dot product
// three rounded products and two rounded sums. With u = 2^-24, L = |o - c|, D = |d| and p the
// ray's distance from the centre (a (p^2 - r^2) = a cc - b b exactly), to first order in u:
//   oc        u per component
//   b         4 u L D (oc 1, product 1, sums 2)       RN(b b) <= b^2 + 9 u L^2 D^2
//   dot(oc,oc) 5 u L^2 (oc 2, product 1, sums 2); rr u r^2; the subtraction u (L^2 - r^2)
//                                                     cc >= L^2 - r^2 - 6 u L^2
//   a         3 u D^2; the product a cc one more u    RN(a cc) >= a (L^2 - r^2) - 10 u L^2 D^2
// so an accepted ray has p^2 - r^2 < 19 u L^2, the second-order terms (~100 u^2 L^2) and the
// underflow of a direction at the tiny limit included in
//   p^2 < r^2 + kSphereDiscErr L^2 + kSphereDiscAbs,   kSphereDiscErr = 20 * 2^-24.
// Underflow: an operation that underflows errs by U = 2^-150 at most. The three products of a,
// the three of b, and b b and a cc add U (2 + 3 L^2 + 6 L D) to a (p^2 - r^2); with one direction
// component of kBvhTinyDir = 2^-60 or more, a >= 2^-120, which is 2^-29 + 0.05 u L^2 + 6 L 2^-90 in
// p^2: kSphereDiscAbs = 2^-28 and the slack of 20 over 19 hold it. (The bound assumes no
// overflow: L D < 2^63, far beyond any scene the padding's own arithmetic holds for.)
// The accepted root lies on the chord of that larger ball: sq^2 = disc <= a (r^2 + E - p^2), so
// the hit point is within sqrt(r^2 + E) of the centre, up to the root's own rounding (a few
// u L), which the boxes' padding covers as it does for every kind's roots.
constexpr float kSphereDiscErr = 20.0f * 0x1p-24f;
constexpr float kSphereDiscAbs = 0x1p-28f;
// The radius of the ball every accepted root of a sphere (centre c, radius r) lies in, for
// every ray the walk admits: origin components within `reach` (cast_fallback's first
// condition, so |o_k - c_k| <= reach + |c_k|) and a direction component of kBvhTinyDir or more.
// The builder bounds a sphere by c +- this. Formed in double and rounded up.
inline float bvh_sphere_bound(const float c[3], float r, float reach) {
  double l2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double l = static_cast<double>(reach) + fabs(static_cast<double>(c[k]));
    l2 += l * l;
  }
  const double R = sqrt(static_cast<double>(r) * r + static_cast<double>(kSphereDiscErr) * l2 + kSphereDiscAbs);
  float f = static_cast<float>(R);
  if (static_cast<double>(f) < R) f = nextafterf(f, INFINITY);
  return f;
}

// The reach for a scene: kBvhOriginReach extents, less for a scene with spheres, whose bounds
// grow with it (bvh_sphere_bound: E = kSphereDiscErr |o - c|^2 is added to r^2). It is chosen
// so that E stays within r pad + pad^2 / 4 (r the smallest radius, pad the boxes' padding, with
// 2^-20 for the constant and |o - c|^2 <= 3 (|o| + extent)^2): up to there a sphere's bounds
// grow by less than half the padding. The reach is never set below extent + 1, because every
// scatter origin lies there and a shorter reach would switch the BVH off. Where extent is more
// than about 10 r (the test lattices; 10,000 spheres of radius 2.5 over +-5000) the floor
// decides, and the bounds of a small sphere grow by more than its radius: at the floor
// sqrt(E) <= sqrt(60 * 2^-24) (2 extent + 1) = 0.0038 extent. The generator's 10,000 spheres of
// radius 2.5 (a 10 x 1000 grid at a spacing of 5, extent 4997.5) get bounds of radius 9.8 to
// 13.6, which overlap several neighbours a side: its trace costs 2.3 times what it did with
// bounds of 2.5. The scalar reach is a cube, so x and z count 5000 units each
// for a scene 50 wide and 5 deep; a reach per axis would cut those bounds to a radius of 4 to 6
// and is not done here (it changes the kernels' fallback test). The reach is a policy for the
// boxes' size; the cull is conservative for any reach the bounds were built with
// (tests/test_cull_host.py).
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
// The smallest sphere radius of a list (-1: no sphere; a NaN radius counts as 0): the second
// argument of bvh_origin_reach, SceneFacts::bvh_sphere_rmin.
float bvh_sphere_rmin(const std::vector<fr_prim>& prims);
#endif

#if !defined(__HIPCC_RTC__)
// Largest internal-node depth of the trees (root = 0): below kBvhStack by construction.
uint32_t bvh_max_depth(const std::vector<BvhSegment>& segs, const std::vector<BvhNode>& nodes);
#endif

}  // namespace fr
