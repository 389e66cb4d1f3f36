// cast.hip — ray queries on the device (fr_ctx_cast): one thread per ray walks
// the scene's list in order (TREE = false: gbuffer_kernel's loop, wave-uniform index, scalar
// record loads) or the scene's tree (TREE = true: the list cut at its planes, each run through
// its own tree, bvh.h), and writes the winner as the G-buffer's three 16-byte words. The
// arithmetic is cast.h's and gbuffer.h's; the tree walk equals the list loop bit for bit, and a
// wave holding a ray the cull is not conservative for (cast_fallback) walks the list for all its
// lanes. cast_kernel<TREE, true> starts closest at the ray's own t_max (FR_CAST_TMAX, DESIGN.md
// §4.5h) and is otherwise the same kernel. gbuffer_tree_kernel is the same walk with the pinhole
// ray of a pixel as the ray source.
// No scratch; no atomics but one add per wave into the cast's striped wave counter; the tree
// walk's per-lane traversal stack is dynamic LDS, level-major (cast_lds_bytes).
#include "cast.h"

#include <type_traits>

#include "trace_kernel.h"  // RecRef, rec_at, buf_load4, lds_u32_at: table reads as the trace kernel's

namespace fr {

extern __shared__ uint32_t cast_stack[];  // [level][lane of the workgroup]; level 0 is the sentinel row

constexpr uint32_t kCastLevelB = kCastBlock * 4u;  // bytes of one stack level

struct CastLeafRec {  // a leaf-order record by per-lane buffer loads
  const float4* base;
  uint32_t off;
  __device__ __forceinline__ float4 operator[](uint32_t k) const { return buf_load4(base, off + 16u * k); }
};

// The closest hit of r: closest and best as the list loop leaves them. tid: the lane's index in
// its workgroup. Every lane of the wave must be here (the table indices are wave-uniform and
// the fallback is a ballot). Returns true if the wave walked the list. t_max: what closest starts
// at, the ray's range; the walks below are written against closest alone.
template <bool TREE>
__device__ __forceinline__ bool cast_walk(const CastScene& sc, const GbRay& r, uint32_t tid, float& closest, int& best,
                                          const float t_max = kCastTMax) {
  closest = t_max;
  best = -1;
  typedef __attribute__((address_space(4))) const uint32_t cu32;
  bool list_walk = !TREE;
  if (TREE) {
    const CastCull cull = cast_cull(r);
    list_walk = __ballot(cast_fallback(r, cull, sc.reach)) != 0;
    if (!list_walk) {
      const uint32_t tbase = lds_addr(cast_stack) + 4u * tid;
      lds_u32_at(tbase) = kBvhEnd;  // the sentinel: what an empty stack pops
      for (uint32_t sg = 0; sg < sc.n_segs; ++sg) {
        const cu32* sp = (cu32*)(reinterpret_cast<uintptr_t>(sc.segs)) + 4u * __builtin_amdgcn_readfirstlane(sg);
        if (sp[0]) {  // a plane, where it stands
          const uint32_t i = sp[3];
          float t = 0.0f;
          if (gb_test<FR_PLANE>(rec_at(sc.gb.rec, i), r, closest, t)) {
            closest = t;
            best = static_cast<int>(i);
          }
          continue;
        }
        uint32_t ref = sp[1];
        uint32_t tso = tbase + kCastLevelB;  // the lane's next free entry (LDS byte address)
        while (ref != kBvhEnd) {
          while (ref < kBvhLeaf) {
            // the stack's top, read before the node arrives (the sentinel when it is empty)
            const uint32_t tdown = tso - kCastLevelB;
            const uint32_t top = lds_u32_at(tdown);
            CastStep st;
            const uint32_t ref0 = __builtin_amdgcn_readfirstlane(ref);
            if (__ballot(ref != ref0) == 0) {
              // every walking lane at one node: scalar loads, the slabs on SGPR operands
              const RecRef nd = rec_at(sc.bvh, ref0);
              const float4 cr = nd[3];
              st = cast_node_step(nd[0], nd[1], nd[2], __float_as_uint(cr.x), __float_as_uint(cr.y), cull, closest);
              asm volatile("; cast node step: scalar");
            } else {
              const uint32_t nb0 = ref * 64u;  // node byte offset (< 2^32: nodes < 2^26)
              const uint4 nr = __builtin_bit_cast(uint4, buf_load4(sc.bvh, nb0 + 48u));
              st = cast_node_step(buf_load4(sc.bvh, nb0), buf_load4(sc.bvh, nb0 + 16u), buf_load4(sc.bvh, nb0 + 32u), nr.x,
                                  nr.y, cull, closest);
              asm volatile("; cast node step: vector");
            }
            // branch-free: the far child goes to the free entry either way (a node at depth d
            // has at most d entries below it, d < levels) and the position moves on a push or pop
            lds_u32_at(tso) = st.far;
            ref = st.any ? st.near : top;
            tso = st.both ? tso + kCastLevelB : (st.any ? tso : tdown);
          }
          if (ref == kBvhEnd) break;
          // leaf: slots [first, first + count) of the leaf-order records
          auto leaf_test = [&](const uint32_t i, const auto& lr) {
            float t = 0.0f;
            if (cast_leaf_test(__float_as_uint(lr[3].w), lr, r, cast_leaf_tmax(i, best, closest), t)) {
              closest = t;
              best = static_cast<int>(i);
            }
          };
          const uint32_t leaf0 = __builtin_amdgcn_readfirstlane(ref);
          if (__ballot(ref != leaf0) == 0) {
            // every lane at one leaf: its records through scalar loads
            const cu32* ord = (cu32*)(reinterpret_cast<uintptr_t>(sc.bvh_order));
            const uint32_t first0 = leaf0 & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt0 = ((leaf0 >> kBvhSlotBits) & 15u) + 1u;
            for (uint32_t kk = 0; kk < cnt0; ++kk) leaf_test(ord[first0 + kk], rec_at(sc.lrec, first0 + kk));
            asm volatile("; cast leaf: scalar");
          } else {
            const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt = ((ref >> kBvhSlotBits) & 15u) + 1u;
            for (uint32_t kk = 0; kk < cnt; ++kk) {
              const uint32_t slot = first + kk;  // buffer loads: 32-bit offsets (slots < 2^26)
              leaf_test(buf_load1(sc.bvh_order, slot * 4u), CastLeafRec{sc.lrec, slot * 64u});
            }
            asm volatile("; cast leaf: vector");
          }
          tso -= kCastLevelB;  // pop (the sentinel when the stack was empty)
          ref = lds_u32_at(tso);
        }
      }
    }
  }
  if (list_walk) {
    auto test_one = [&](auto kind_tag, uint32_t i) {
      float t = 0.0f;
      if (gb_test<decltype(kind_tag)::value>(rec_at(sc.gb.rec, i), r, closest, t)) {
        closest = t;
        best = static_cast<int>(i);
      }
    };
    // The list in order, as its kind runs: one scalar kind branch per run (gbuffer_kernel's loop).
    for (uint32_t rr = 0; rr < sc.gb.n_runs; ++rr) {
      const cu32* rp = (cu32*)(reinterpret_cast<uintptr_t>(sc.gb.runs)) + 4u * __builtin_amdgcn_readfirstlane(rr);
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
  }
  return list_walk;
}

// The winner's words at index i of the three buffers: per-lane loads of its record, class and
// attenuation, once per ray.
__device__ __forceinline__ void cast_store(const GbScene& sc, const GbRay& r, float closest, int best, size_t i, float4* g0,
                                           float4* g1, float4* alb) {
  GbPixel p = gb_miss();
  if (best >= 0) {
    const uint32_t b = static_cast<uint32_t>(best);
    struct Rec {
      float4 v[4];
      __device__ __forceinline__ float4 operator[](int k) const { return v[k]; }
    };
    const float4* rb = sc.rec + 4u * static_cast<size_t>(b);
    const Rec rec{{rb[0], rb[1], rb[2], rb[3]}};
    p = gb_hit(b, __float_as_uint(rec.v[3].w), sc.cls[b], rec, sc.att[b], r, closest);
  }
  g0[i] = make_float4(p.g0.x, p.g0.y, p.g0.z, p.g0.w);
  g1[i] = make_float4(p.g1.x, p.g1.y, p.g1.z, p.g1.w);
  alb[i] = make_float4(p.alb.x, p.alb.y, p.alb.z, p.alb.w);
}

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
  float closest;
  int best;
  const bool list_walk = cast_walk<TREE>(a.sc, r, tid, closest, best, RANGED ? rd.w : kCastTMax);
  // one add per wave that holds a ray (a wave's first lane has its lowest index)
  if ((tid & 63u) == 0u && inside)
    atomicAdd(&a.waves[(blockIdx.x % kCastStripes) * kCastStripeWords + (list_walk ? 1u : 0u)], 1u);
  if (inside) cast_store(a.sc.gb, r, closest, best, i, a.g0, a.g1, a.alb);
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
  float closest;
  int best;
  cast_walk<true>(a.sc, r, tid, closest, best);
  if (inside) cast_store(a.sc.gb, r, closest, best, static_cast<size_t>(y) * a.W + x, a.g0, a.g1, a.alb);
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
