// occlude.hip — occlusion queries on the device (fr_ctx_occluded): one thread
// per ray answers "does anything of the scene lie in (kGbTMin, t_max) of this ray?" as one byte.
// The answer is the OR over every list primitive of its test against t_max itself (cast.h
// occl_walk_list), so the order of the tests is free and a lane stops at its first accepted one:
// no closest, no winner, no record. TREE = true walks the scene's tree as cast_walk<true> does
// (fallback ballot, scalar segment reads, the level-major per-lane LDS stack with its sentinel
// row, the branch-free node step at closest = t_max, scalar loads where every walking lane is at
// one node or leaf); a lane with a hit sets its reference to kBvhEnd and leaves the loops, and
// the segment loop ends when no lane is still looking. TREE = false, and a wave holding a ray the
// cull is not conservative for (cast_fallback), tests the list with a wave-uniform index and
// leaves once every lane is occluded. No scratch; no atomics but two adds per wave into the
// striped wave counter.
#include "cast.h"

#include <type_traits>

#include "trace_kernel.h"  // RecRef, rec_at, buf_load4, lds_u32_at: table reads as the trace kernel's
#include "tuning.h"

namespace fr {

extern __shared__ uint32_t occl_stack[];  // [level][lane of the workgroup]; level 0 is the sentinel row

constexpr uint32_t kOcclLevelB = kCastBlock * 4u;  // bytes of one stack level
constexpr bool kOcclNearFirst = FR_OCCL_NEAR_FIRST != 0;
constexpr uint32_t kOcclExitEvery = FR_OCCL_EXIT_EVERY;
static_assert(kOcclExitEvery >= 1u, "FR_OCCL_EXIT_EVERY counts primitives");

struct OcclLeafRec {  // a leaf-order record by per-lane buffer loads
  const float4* base;
  uint32_t off;
  __device__ __forceinline__ float4 operator[](uint32_t k) const { return buf_load4(base, off + 16u * k); }
};

// The children of a node in the order the any-hit walk takes them: cast_node_step's (the nearer
// entered child first), or the left one first. Which children are entered is the same.
template <class F4>
__device__ __forceinline__ CastStep occl_node_step(const F4& na, const F4& nb, const F4& nc, uint32_t cl, uint32_t cr,
                                                   const CastCull& c, float t_max) {
  if (kOcclNearFirst) return cast_node_step(na, nb, nc, cl, cr, c, t_max);
  float tl, tr;
  const bool ml = cast_node_enter(V3{na.x, na.y, na.z}, V3{nb.x, nb.y, nb.z}, c, t_max, tl);
  const bool mr = cast_node_enter(V3{na.w, nc.x, nc.y}, V3{nb.w, nc.z, nc.w}, c, t_max, tr);
  CastStep s;
  s.near = ml ? cl : cr;
  s.far = ml ? cr : cl;
  s.any = ml | mr;
  s.both = ml & mr;
  return s;
}

// occ: whether any primitive's test accepts r in (kGbTMin, t_max). tid: the lane's index in its
// workgroup. Every lane of the wave must be here (the table indices are wave-uniform and the
// fallback is a ballot). Returns true if the wave walked the list.
template <bool TREE>
__device__ __forceinline__ bool occl_walk(const CastScene& sc, const GbRay& r, uint32_t tid, const float t_max, bool& occ) {
  occ = false;
  typedef __attribute__((address_space(4))) const uint32_t cu32;
  bool list_walk = !TREE;
  if (TREE) {
    const CastCull cull = cast_cull(r);
    list_walk = __ballot(cast_fallback(r, cull, sc.reach)) != 0;
    if (!list_walk) {
      const uint32_t tbase = lds_addr(occl_stack) + 4u * tid;
      lds_u32_at(tbase) = kBvhEnd;  // the sentinel: what an empty stack pops
      for (uint32_t sg = 0; sg < sc.n_segs; ++sg) {
        if (__ballot(!occ) == 0) break;  // no lane is still looking
        const cu32* sp = (cu32*)(reinterpret_cast<uintptr_t>(sc.segs)) + 4u * __builtin_amdgcn_readfirstlane(sg);
        if (sp[0]) {  // a plane, where it stands
          float t = 0.0f;
          occ |= gb_test<FR_PLANE>(rec_at(sc.gb.rec, sp[3]), r, t_max, t);
          continue;
        }
        uint32_t ref = occ ? kBvhEnd : sp[1];  // a lane with a hit walks no further
        uint32_t tso = tbase + kOcclLevelB;    // the lane's next free entry (LDS byte address)
        while (ref != kBvhEnd) {
          while (ref < kBvhLeaf) {
            // the stack's top, read before the node arrives (the sentinel when it is empty)
            const uint32_t tdown = tso - kOcclLevelB;
            const uint32_t top = lds_u32_at(tdown);
            CastStep st;
            // (the lanes here are the walking ones: a lane with a hit has left both loops)
            const uint32_t ref0 = __builtin_amdgcn_readfirstlane(ref);
            if (__ballot(ref != ref0) == 0) {
              // every walking lane at one node: scalar loads, the slabs on SGPR operands
              const RecRef nd = rec_at(sc.bvh, ref0);
              const float4 cr = nd[3];
              st = occl_node_step(nd[0], nd[1], nd[2], __float_as_uint(cr.x), __float_as_uint(cr.y), cull, t_max);
              asm volatile("; occlude node step: scalar");
            } else {
              const uint32_t nb0 = ref * 64u;  // node byte offset (< 2^32: nodes < 2^26)
              const uint4 nr = __builtin_bit_cast(uint4, buf_load4(sc.bvh, nb0 + 48u));
              st = occl_node_step(buf_load4(sc.bvh, nb0), buf_load4(sc.bvh, nb0 + 16u), buf_load4(sc.bvh, nb0 + 32u), nr.x,
                                  nr.y, cull, t_max);
              asm volatile("; occlude node step: vector");
            }
            // branch-free: the far child goes to the free entry either way (a node at depth d
            // has at most d entries below it, d < levels) and the position moves on a push or pop
            lds_u32_at(tso) = st.far;
            ref = st.any ? st.near : top;
            tso = st.both ? tso + kOcclLevelB : (st.any ? tso : tdown);
          }
          if (ref == kBvhEnd) break;
          // leaf: slots [first, first + count) of the leaf-order records, each against t_max
          const uint32_t leaf0 = __builtin_amdgcn_readfirstlane(ref);
          if (__ballot(ref != leaf0) == 0) {
            // every lane at one leaf: its records through scalar loads
            const uint32_t first0 = leaf0 & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt0 = ((leaf0 >> kBvhSlotBits) & 15u) + 1u;
            for (uint32_t kk = 0; kk < cnt0; ++kk) {
              const RecRef lr = rec_at(sc.lrec, first0 + kk);
              float t = 0.0f;
              occ |= cast_leaf_test(__float_as_uint(lr[3].w), lr, r, t_max, t);
            }
            asm volatile("; occlude leaf: scalar");
          } else {
            const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt = ((ref >> kBvhSlotBits) & 15u) + 1u;
            for (uint32_t kk = 0; kk < cnt; ++kk) {
              const OcclLeafRec lr{sc.lrec, (first + kk) * 64u};  // buffer loads: 32-bit offsets (slots < 2^26)
              float t = 0.0f;
              occ |= cast_leaf_test(__float_as_uint(lr[3].w), lr, r, t_max, t);
            }
            asm volatile("; occlude leaf: vector");
          }
          tso -= kOcclLevelB;  // pop (the sentinel when the stack was empty)
          ref = occ ? kBvhEnd : lds_u32_at(tso);
        }
      }
    }
  }
  if (list_walk) {
    // The list as its kind runs: one scalar kind branch per run, a wave-uniform index, and a
    // ballot every kOcclExitEvery primitives that ends the walk once every lane is occluded.
    bool looking = true;
    auto run = [&](auto kind_tag, uint32_t i0, uint32_t i1) {
      for (uint32_t i = i0; i < i1 && looking;) {
        const uint32_t e = i1 - i < kOcclExitEvery ? i1 : i + kOcclExitEvery;
        for (; i < e; ++i) {
          float t = 0.0f;
          occ |= gb_test<decltype(kind_tag)::value>(rec_at(sc.gb.rec, __builtin_amdgcn_readfirstlane(i)), r, t_max, t);
        }
        looking = __ballot(!occ) != 0;
      }
    };
    for (uint32_t rr = 0; rr < sc.gb.n_runs && looking; ++rr) {
      const cu32* rp = (cu32*)(reinterpret_cast<uintptr_t>(sc.gb.runs)) + 4u * __builtin_amdgcn_readfirstlane(rr);
      const uint32_t k = rp[0], i0 = rp[1], i1 = rp[2];
      if (k == FR_AABB)
        run(std::integral_constant<uint32_t, FR_AABB>{}, i0, i1);
      else if (k == FR_SPHERE)
        run(std::integral_constant<uint32_t, FR_SPHERE>{}, i0, i1);
      else if (k == FR_PLANE)
        run(std::integral_constant<uint32_t, FR_PLANE>{}, i0, i1);
      else if (k == FR_TRIANGLE)
        run(std::integral_constant<uint32_t, FR_TRIANGLE>{}, i0, i1);
      else if (k == FR_OBB)
        run(std::integral_constant<uint32_t, FR_OBB>{}, i0, i1);
      // FR_STUB: never hits
    }
  }
  return list_walk;
}

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
  bool occ;
  const bool list_walk = occl_walk<TREE>(a.sc, r, tid, a.ranged ? rd.w : kCastTMax, occ);
  // per wave that holds a ray (its first lane has its lowest index): one add to the tree / list
  // word of the workgroup's stripe, one of the wave's occluded rays to the third word
  const uint32_t hits = __popcll(__ballot(occ & inside));
  if ((tid & 63u) == 0u && inside) {
    uint32_t* stripe = a.waves + (blockIdx.x % kCastStripes) * kCastStripeWords;
    atomicAdd(&stripe[list_walk ? 1u : 0u], 1u);
    atomicAdd(&stripe[2], hits);
  }
  if (inside) a.out[i] = occ ? 1u : 0u;  // a wave's 64 bytes: one line
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
