// scene_walk.h — the one device walk of a scene outside the trace kernel:
// scene_walk<TREE, Hit> takes one ray per lane through the scene's list in order (TREE = false:
// kind runs, a wave-uniform index, scalar record loads) or through its tree (TREE = true: the
// list cut at its planes, each run through its own tree, bvh.h), and a hit policy says what a
// test's answer does. ClosestHit keeps the winner as the list loop leaves it (fr_ctx_cast, both
// G-buffer passes); AnyHit<N> keeps whether any test accepted (fr_ctx_occluded). The arithmetic
// is cast.h's and gbuffer.h's, and the host walks of cast.h are the definition the kernels are
// held to. A wave holding a ray the cull is not conservative for (cast_fallback) walks the list
// for all its lanes. No scratch, no atomics; the tree walk's per-lane traversal stack is dynamic
// LDS, level-major (cast_lds_bytes). Device only.
#pragma once
#include <type_traits>

#include "cast.h"
#include "trace_kernel.h"  // RecRef, rec_at, buf_load4, lds_u32_at: table reads as the trace kernel's

namespace fr {

extern __shared__ uint32_t walk_stack[];  // [level][lane of the workgroup]; level 0 is the sentinel row

constexpr uint32_t kWalkLevelB = kCastBlock * 4u;  // bytes of one stack level

struct WalkLeafRec {  // a leaf-order record by per-lane buffer loads
  const float4* base;
  uint32_t off;
  __device__ __forceinline__ float4 operator[](uint32_t k) const { return buf_load4(base, off + 16u * k); }
};

// The closest hit: closest and best as the list loop leaves them. Tests run against the
// shrinking closest, a leaf's against cast_leaf_tmax of its list index; the nearer entered child
// goes first; a lane never stops.
struct ClosestHit {
  int best = -1;
  float closest;  // starts at the ray's range (kCastTMax, or its own t_max: DESIGN.md §4.5h)
  static constexpr uint32_t kExitEvery = 0;  // the list loop takes no ballot
  __device__ __forceinline__ explicit ClosestHit(float t_max = kCastTMax) : closest(t_max) {}
  static constexpr __device__ bool done() { return false; }
  template <class F4>
  __device__ __forceinline__ CastStep node_step(const F4& na, const F4& nb, const F4& nc, uint32_t cl, uint32_t cr,
                                                const CastCull& c) const {
    return cast_node_step(na, nb, nc, cl, cr, c, closest);
  }
  // a list record of kind K at list index i (a plane where it stands included)
  template <uint32_t K, class Rec>
  __device__ __forceinline__ void list_test(const Rec& rec, const GbRay& r, uint32_t i) {
    float t = 0.0f;
    if (gb_test<K>(rec, r, closest, t)) {
      closest = t;
      best = static_cast<int>(i);
    }
  }
  // a leaf-order record; index() reads its list index
  template <class Rec, class Index>
  __device__ __forceinline__ void leaf_test(const Rec& lr, const GbRay& r, Index index) {
    const uint32_t i = index();
    float t = 0.0f;
    if (cast_leaf_test(__float_as_uint(lr[3].w), lr, r, cast_leaf_tmax(i, best, closest), t)) {
      closest = t;
      best = static_cast<int>(i);
    }
  }
};

// Any hit: the OR of every test against t_max itself, so the order of the tests is free. The
// left entered child goes first (which children are entered is cast_node_step's; near first
// measured slower on every ray set); no list index is read; a lane that has its
// answer walks no further, and the list loop asks every EXIT_EVERY primitives whether a lane of
// the wave is still looking.
template <uint32_t EXIT_EVERY>
struct AnyHit {
  static_assert(EXIT_EVERY >= 1u, "EXIT_EVERY counts primitives");
  const float t_max;
  bool occ = false;
  static constexpr uint32_t kExitEvery = EXIT_EVERY;
  __device__ __forceinline__ explicit AnyHit(float t_max_) : t_max(t_max_) {}
  __device__ __forceinline__ bool done() const { return occ; }
  template <class F4>
  __device__ __forceinline__ CastStep node_step(const F4& na, const F4& nb, const F4& nc, uint32_t cl, uint32_t cr,
                                                const CastCull& c) const {
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
  template <uint32_t K, class Rec>
  __device__ __forceinline__ void list_test(const Rec& rec, const GbRay& r, uint32_t) {
    float t = 0.0f;
    occ |= gb_test<K>(rec, r, t_max, t);
  }
  template <class Rec, class Index>
  __device__ __forceinline__ void leaf_test(const Rec& lr, const GbRay& r, Index) {
    float t = 0.0f;
    occ |= cast_leaf_test(__float_as_uint(lr[3].w), lr, r, t_max, t);
  }
};

// Walks r through sc and leaves the answer in h. tid: the lane's index in its workgroup. Every
// lane of the wave must be here (the table indices are wave-uniform and the fallback is a
// ballot). Returns true if the wave walked the list.
template <bool TREE, class Hit>
__device__ __forceinline__ bool scene_walk(const CastScene& sc, const GbRay& r, uint32_t tid, Hit& h) {
  typedef __attribute__((address_space(4))) const uint32_t cu32;
  constexpr bool kStops = Hit::kExitEvery != 0;  // a lane can have its answer before the walk ends
  bool list_walk = !TREE;
  if constexpr (TREE) {
    const CastCull cull = cast_cull(r);
    list_walk = __ballot(cast_fallback(r, cull, sc.reach)) != 0;
    if (!list_walk) {
      const uint32_t tbase = lds_addr(walk_stack) + 4u * tid;
      lds_u32_at(tbase) = kBvhEnd;  // the sentinel: what an empty stack pops
      for (uint32_t sg = 0; sg < sc.n_segs; ++sg) {
        if constexpr (kStops)
          if (__ballot(!h.done()) == 0) break;  // no lane is still looking
        const cu32* sp = (cu32*)(reinterpret_cast<uintptr_t>(sc.segs)) + 4u * __builtin_amdgcn_readfirstlane(sg);
        if (sp[0]) {  // a plane, where it stands
          const uint32_t i = sp[3];
          h.template list_test<FR_PLANE>(rec_at(sc.gb.rec, i), r, i);
          continue;
        }
        uint32_t ref = h.done() ? kBvhEnd : sp[1];  // a lane that is done walks no further
        uint32_t tso = tbase + kWalkLevelB;         // the lane's next free entry (LDS byte address)
        while (ref != kBvhEnd) {
          while (ref < kBvhLeaf) {
            // the stack's top, read before the node arrives (the sentinel when it is empty)
            const uint32_t tdown = tso - kWalkLevelB;
            const uint32_t top = lds_u32_at(tdown);
            CastStep st;
            // (the lanes here are the walking ones: a lane that is done has left both loops)
            const uint32_t ref0 = __builtin_amdgcn_readfirstlane(ref);
            if (__ballot(ref != ref0) == 0) {
              // every walking lane at one node: scalar loads, the slabs on SGPR operands
              const RecRef nd = rec_at(sc.bvh, ref0);
              const float4 cr = nd[3];
              st = h.node_step(nd[0], nd[1], nd[2], __float_as_uint(cr.x), __float_as_uint(cr.y), cull);
              asm volatile("; walk node step: scalar");
            } else {
              const uint32_t nb0 = ref * 64u;  // node byte offset (< 2^32: nodes < 2^26)
              const uint4 nr = __builtin_bit_cast(uint4, buf_load4(sc.bvh, nb0 + 48u));
              st = h.node_step(buf_load4(sc.bvh, nb0), buf_load4(sc.bvh, nb0 + 16u), buf_load4(sc.bvh, nb0 + 32u), nr.x, nr.y,
                               cull);
              asm volatile("; walk node step: vector");
            }
            // branch-free: the far child goes to the free entry either way (a node at depth d
            // has at most d entries below it, d < levels) and the position moves on a push or pop
            lds_u32_at(tso) = st.far;
            ref = st.any ? st.near : top;
            tso = st.both ? tso + kWalkLevelB : (st.any ? tso : tdown);
          }
          if (ref == kBvhEnd) break;
          // leaf: slots [first, first + count) of the leaf-order records
          const uint32_t leaf0 = __builtin_amdgcn_readfirstlane(ref);
          if (__ballot(ref != leaf0) == 0) {
            // every lane at one leaf: its records through scalar loads
            const cu32* ord = (cu32*)(reinterpret_cast<uintptr_t>(sc.bvh_order));
            const uint32_t first0 = leaf0 & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt0 = ((leaf0 >> kBvhSlotBits) & 15u) + 1u;
            for (uint32_t kk = 0; kk < cnt0; ++kk)
              h.leaf_test(rec_at(sc.lrec, first0 + kk), r, [&] { return ord[first0 + kk]; });
            asm volatile("; walk leaf: scalar");
          } else {
            const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt = ((ref >> kBvhSlotBits) & 15u) + 1u;
            for (uint32_t kk = 0; kk < cnt; ++kk) {
              const uint32_t slot = first + kk;  // buffer loads: 32-bit offsets (slots < 2^26)
              h.leaf_test(WalkLeafRec{sc.lrec, slot * 64u}, r, [&] { return buf_load1(sc.bvh_order, slot * 4u); });
            }
            asm volatile("; walk leaf: vector");
          }
          tso -= kWalkLevelB;  // pop (the sentinel when the stack was empty)
          ref = h.done() ? kBvhEnd : lds_u32_at(tso);
        }
      }
    }
  }
  if (list_walk) {
    // The list in order, as its kind runs (KScene::runs): one scalar kind branch per run, a
    // wave-uniform index, and where lanes stop a ballot every kExitEvery primitives that ends
    // the walk once no lane is still looking.
    bool looking = true;
    auto span = [&](auto kind_tag, uint32_t i, uint32_t e) {
      for (; i < e; ++i) {
        const uint32_t iu = __builtin_amdgcn_readfirstlane(i);
        h.template list_test<decltype(kind_tag)::value>(rec_at(sc.gb.rec, iu), r, iu);
      }
    };
    auto run = [&](auto kind_tag, uint32_t i0, uint32_t i1) {
      if constexpr (!kStops) {
        span(kind_tag, i0, i1);
      } else {
        for (uint32_t i = i0; i < i1 && looking;) {
          const uint32_t e = i1 - i < Hit::kExitEvery ? i1 : i + Hit::kExitEvery;
          span(kind_tag, i, e);
          i = e;
          looking = __ballot(!h.done()) != 0;
        }
      }
    };
    for (uint32_t rr = 0; rr < sc.gb.n_runs && (!kStops || looking); ++rr) {
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

// The closest hit's words at index i of the three buffers: per-lane loads of the winner's
// record, class and attenuation, once per ray.
__device__ __forceinline__ void cast_store(const GbScene& sc, const GbRay& r, const ClosestHit& h, size_t i, float4* g0,
                                           float4* g1, float4* alb) {
  GbPixel p = gb_miss();
  if (h.best >= 0) {
    const uint32_t b = static_cast<uint32_t>(h.best);
    struct Rec {
      float4 v[4];
      __device__ __forceinline__ float4 operator[](int k) const { return v[k]; }
    };
    const float4* rb = sc.rec + 4u * static_cast<size_t>(b);
    const Rec rec{{rb[0], rb[1], rb[2], rb[3]}};
    p = gb_hit(b, __float_as_uint(rec.v[3].w), sc.cls[b], rec, sc.att[b], r, h.closest);
  }
  g0[i] = make_float4(p.g0.x, p.g0.y, p.g0.z, p.g0.w);
  g1[i] = make_float4(p.g1.x, p.g1.y, p.g1.z, p.g1.w);
  alb[i] = make_float4(p.alb.x, p.alb.y, p.alb.z, p.alb.w);
}

}  // namespace fr
