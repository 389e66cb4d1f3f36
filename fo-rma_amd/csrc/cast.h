// cast.h — ray queries (fr_ctx_cast): the closest hit of a caller's own ray, as
// the G-buffer's pixel (gbuffer.h: id, own root t, N, P, albedo), through the list in order or
// through the scene's tree (bvh.h). Its f32 arithmetic, shared by the kernels (cast.hip) and a
// CPU program (tests/c/cast_check.cpp), and the launches. gbuffer.h's rules hold: every named
// operation rounds once in f32, no contraction, IEEE '/' and sqrt.
//
// The tree walk equals the list loop bit for bit: the list is cut into
// BvhSegments, in order. A plane is tested where it stands against `closest`. A run yields the
// least (t, index) of the run below `closest`: a leaf primitive is tested with t_max = closest,
// or one ulp above closest when its index is below the current winner's (it may take an exact
// tie), and the node boxes are padded over bounds that hold each test's own error (a sphere's:
// bvh.h bvh_sphere_bound), so nothing the list loop accepts is culled while the three conditions of
// cast_fallback hold; a ray that fails one takes the list.
//
// Ranged casts and occlusion queries (fr_ctx_occluded): the walks take the ray's
// t_max as what `closest` starts at, and occl_walk_list / occl_walk_tree answer whether any
// primitive's test accepts the ray within (kGbTMin, t_max) (occlude.hip, tests/c/occlude_check.cpp).
#pragma once
#include <float.h>

#include "bvh.h"
#include "gbuffer.h"

namespace fr {

constexpr float kCastTMax = FLT_MAX;  // the reference's range: (kGbTMin, FLT_MAX)

// The GbRay of an arbitrary ray: gb_primary_ray's last three lines.
FR_HD GbRay cast_ray(V3 o, V3 d) {
  GbRay r;
  r.o = o;
  r.d = d;
  r.inv = V3{box_inv_clamp(1.0f / d.x), box_inv_clamp(1.0f / d.y), box_inv_clamp(1.0f / d.z)};
  r.oinv = V3{r.o.x * r.inv.x, r.o.y * r.inv.y, r.o.z * r.inv.z};
  r.a = dot(r.d, r.d);
  return r;
}

// The node cull's reciprocals and o inv: r.inv clamped to +-kBvhInvClamp. (kBoxInvClamp is the
// same 2^100 today, so the clamp changes no value and oinv is r.oinv; the cull stays right if
// the box test's clamp ever moves.)
struct CastCull {
  V3 inv, oinv;
};
FR_HD CastCull cast_cull(const GbRay& r) {
  CastCull c;
  c.inv = V3{fmin_num(fmax_num(r.inv.x, -kBvhInvClamp), kBvhInvClamp), fmin_num(fmax_num(r.inv.y, -kBvhInvClamp), kBvhInvClamp),
             fmin_num(fmax_num(r.inv.z, -kBvhInvClamp), kBvhInvClamp)};
  c.oinv = V3{r.o.x * c.inv.x, r.o.y * c.inv.y, r.o.z * c.inv.z};
  return c;
}

// A ray the node cull is not conservative for (bvh.h; the trace kernel's list_walk ballot):
// !(max|o_k| <= reach), !(max|d_k| >= kBvhTinyDir) or !(max|o_k inv_k| <= FLT_MAX). The first and
// the third are taken per component, so that a NaN component fails them (a NaN-ignoring max
// would drop it); the second asks for one component that is large enough. Such a ray takes the
// list in order.
FR_HD bool cast_fallback(const GbRay& r, const CastCull& c, float reach) {
  const bool near = (__builtin_fabsf(r.o.x) <= reach) & (__builtin_fabsf(r.o.y) <= reach) & (__builtin_fabsf(r.o.z) <= reach);
  const float ad = fmax3_num(__builtin_fabsf(r.d.x), __builtin_fabsf(r.d.y), __builtin_fabsf(r.d.z));
  const bool finite = (__builtin_fabsf(c.oinv.x) <= FLT_MAX) & (__builtin_fabsf(c.oinv.y) <= FLT_MAX) &
                      (__builtin_fabsf(c.oinv.z) <= FLT_MAX);
  return !near | !(ad >= kBvhTinyDir) | !finite;
}

// A node's box (lo, hi) against the ray: entered iff tn <= tf, tf >= t_min and tn <= closest
// (the trace kernel's node_pick test). tn: the box's near distance, the children's order.
FR_HD bool cast_node_enter(V3 lo, V3 hi, const CastCull& c, float closest, float& tn) {
  const Slab s = slab3_fused(lo, hi, c.oinv, c.inv);
  tn = s.tn;
  return (s.tn <= s.tf) & (s.tf >= kGbTMin) & (s.tn <= closest);
}

// The two children of a node (bvh.h BvhNode as four 16-byte words a, b, c and the references).
struct CastStep {
  uint32_t near, far;  // the nearer entered child (the left one on a tie), the other
  bool any, both;      // one child is entered at least; both are
};
template <class F4>
FR_HD CastStep cast_node_step(const F4& na, const F4& nb, const F4& nc, uint32_t cl, uint32_t cr, const CastCull& c,
                              float closest) {
  float tl, tr;
  const bool ml = cast_node_enter(V3{na.x, na.y, na.z}, V3{nb.x, nb.y, nb.z}, c, closest, tl);
  const bool mr = cast_node_enter(V3{na.w, nc.x, nc.y}, V3{nb.w, nc.z, nc.w}, c, closest, tr);
  const bool gol = ml & ((tl <= tr) | !mr);
  CastStep s;
  s.near = gol ? cl : cr;
  s.far = gol ? cr : cl;
  s.any = ml | mr;
  s.both = ml & mr;
  return s;
}

// t_max of a leaf test of list index i: one ulp above closest when i precedes the winner.
FR_HD float cast_leaf_tmax(uint32_t i, int best, float closest) {
  if (static_cast<int>(i) < best) {
    uint32_t u;
    memcpy(&u, &closest, 4);
    ++u;
    float f;
    memcpy(&f, &u, 4);
    return f;
  }
  return closest;
}

// One leaf-order record (pack.cpp off_lrec: the list record, a sphere's radius replaced by
// RN(radius radius), the product sphere_root forms) of kind `kind` in (kGbTMin, t_max): the plain
// IEEE forms gb_test uses. Planes and stubs are never in a leaf.
template <class Rec>
FR_HD bool cast_leaf_test(uint32_t kind, const Rec& lrec, const GbRay& r, float t_max, float& t) {
  if (kind == FR_SPHERE) {
    const auto g = lrec[0];
    return sphere_root_rr(gb_xyz(g), g.w, r.o, r.d, r.a, kGbTMin, t_max, t);
  }
  if (kind == FR_AABB) return gb_test<FR_AABB>(lrec, r, t_max, t);
  if (kind == FR_TRIANGLE) return gb_test<FR_TRIANGLE>(lrec, r, t_max, t);
  if (kind == FR_OBB) return gb_test<FR_OBB>(lrec, r, t_max, t);
  return false;
}

// One list record of kind `kind` against closest, as the list loop tests it.
template <class Rec>
FR_HD bool cast_list_test(uint32_t kind, const Rec& rec, const GbRay& r, float t_max, float& t) {
  if (kind == FR_AABB) return gb_test<FR_AABB>(rec, r, t_max, t);
  if (kind == FR_SPHERE) return gb_test<FR_SPHERE>(rec, r, t_max, t);
  if (kind == FR_PLANE) return gb_test<FR_PLANE>(rec, r, t_max, t);
  if (kind == FR_TRIANGLE) return gb_test<FR_TRIANGLE>(rec, r, t_max, t);
  if (kind == FR_OBB) return gb_test<FR_OBB>(rec, r, t_max, t);
  return false;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The tables of a packed scene as the walks below read them (pack.h's blob, on the host).
struct CastTables {
  const float* rec;         // 16 words per primitive, list order
  const float* lrec;        // 16 words per leaf slot
  const uint32_t* order;    // list index of each leaf slot
  const BvhNode* nodes;
  const BvhSegment* segs;
  const uint32_t* runs;     // {kind, first, end, 0} per kind run
  uint32_t n_runs, n_segs;
};
struct CastRec {
  const float* w;
  GbF4 operator[](int k) const { return GbF4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]}; }
};
inline uint32_t cast_rec_kind(const float* w) {
  uint32_t k;
  memcpy(&k, &w[15], 4);
  return k;
}

// The list loop: the definition every walk must equal. t_max: the ray's range (kGbTMin, t_max),
// what `closest` starts at; whatever a NaN, an infinity, 0 or a negative gives in
// the comparisons below is the answer.
inline void cast_walk_list(const CastTables& s, const GbRay& r, float& closest, int& best, float t_max = kCastTMax) {
  closest = t_max;
  best = -1;
  for (uint32_t rr = 0; rr < s.n_runs; ++rr) {
    const uint32_t k = s.runs[4 * rr], i0 = s.runs[4 * rr + 1], i1 = s.runs[4 * rr + 2];
    for (uint32_t i = i0; i < i1; ++i) {
      float t = 0.0f;
      if (cast_list_test(k, CastRec{s.rec + 16 * static_cast<size_t>(i)}, r, closest, t)) {
        closest = t;
        best = static_cast<int>(i);
      }
    }
  }
}

// The tree walk as a definition: segments in order, near child first, the far child stacked.
// steps (if given) receives the node steps taken. t_max: as cast_walk_list's (the node cull and
// cast_leaf_tmax are written against `closest`, whatever it starts at).
inline void cast_walk_tree(const CastTables& s, const GbRay& r, float& closest, int& best, uint32_t* steps = nullptr,
                           float t_max = kCastTMax) {
  closest = t_max;
  best = -1;
  const CastCull c = cast_cull(r);
  uint32_t nsteps = 0;
  for (uint32_t sg = 0; sg < s.n_segs; ++sg) {
    const BvhSegment& seg = s.segs[sg];
    if (seg.plane) {
      float t = 0.0f;
      if (gb_test<FR_PLANE>(CastRec{s.rec + 16 * static_cast<size_t>(seg.prim)}, r, closest, t)) {
        closest = t;
        best = static_cast<int>(seg.prim);
      }
      continue;
    }
    uint32_t stack[kBvhStack + 1];
    uint32_t sp = 0;
    stack[sp++] = kBvhEnd;  // the sentinel
    uint32_t ref = seg.root;
    while (ref != kBvhEnd) {
      if (ref < kBvhLeaf) {
        const BvhNode& nd = s.nodes[ref];
        const CastStep st = cast_node_step(GbF4{nd.a[0], nd.a[1], nd.a[2], nd.a[3]}, GbF4{nd.b[0], nd.b[1], nd.b[2], nd.b[3]},
                                           GbF4{nd.c[0], nd.c[1], nd.c[2], nd.c[3]}, nd.ref[0], nd.ref[1], c, closest);
        ++nsteps;
        if (st.both) stack[sp++] = st.far;
        ref = st.any ? st.near : stack[--sp];
        continue;
      }
      const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u), cnt = ((ref >> kBvhSlotBits) & 15u) + 1u;
      for (uint32_t k = 0; k < cnt; ++k) {
        const float* lw = s.lrec + 16 * static_cast<size_t>(first + k);
        const uint32_t i = s.order[first + k];
        float t = 0.0f;
        if (cast_leaf_test(cast_rec_kind(lw), CastRec{lw}, r, cast_leaf_tmax(i, best, closest), t)) {
          closest = t;
          best = static_cast<int>(i);
        }
      }
      ref = stack[--sp];
    }
  }
  if (steps) *steps = nsteps;
}

// Occlusion (any hit): the OR over every list primitive of its test against
// t_max itself. It equals "cast_walk_list(.., t_max) finds a winner": the first primitive that
// loop accepts was tested against t_max, and one that passes at t_max is accepted or preceded by
// one that was. Being an OR, the order of the tests is free and a walk may stop at the first.
inline bool occl_walk_list(const CastTables& s, const GbRay& r, float t_max) {
  bool occ = false;
  for (uint32_t rr = 0; rr < s.n_runs; ++rr) {
    const uint32_t k = s.runs[4 * rr], i0 = s.runs[4 * rr + 1], i1 = s.runs[4 * rr + 2];
    for (uint32_t i = i0; i < i1; ++i) {
      float t = 0.0f;
      occ |= cast_list_test(k, CastRec{s.rec + 16 * static_cast<size_t>(i)}, r, t_max, t);
    }
  }
  return occ;
}

// The any-hit tree walk as a definition: segments in order, a plane where it stands against
// t_max, a run from its root with the node cull at closest = t_max and its leaves tested against
// t_max; returns at the first accepted test. steps (if given) receives the node steps taken.
inline bool occl_walk_tree(const CastTables& s, const GbRay& r, float t_max, uint32_t* steps = nullptr) {
  const CastCull c = cast_cull(r);
  uint32_t nsteps = 0;
  bool occ = false;
  for (uint32_t sg = 0; sg < s.n_segs && !occ; ++sg) {
    const BvhSegment& seg = s.segs[sg];
    float t = 0.0f;
    if (seg.plane) {
      occ = gb_test<FR_PLANE>(CastRec{s.rec + 16 * static_cast<size_t>(seg.prim)}, r, t_max, t);
      continue;
    }
    uint32_t stack[kBvhStack + 1];
    uint32_t sp = 0;
    stack[sp++] = kBvhEnd;  // the sentinel
    uint32_t ref = seg.root;
    while (ref != kBvhEnd && !occ) {
      if (ref < kBvhLeaf) {
        const BvhNode& nd = s.nodes[ref];
        const CastStep st = cast_node_step(GbF4{nd.a[0], nd.a[1], nd.a[2], nd.a[3]}, GbF4{nd.b[0], nd.b[1], nd.b[2], nd.b[3]},
                                           GbF4{nd.c[0], nd.c[1], nd.c[2], nd.c[3]}, nd.ref[0], nd.ref[1], c, t_max);
        ++nsteps;
        if (st.both) stack[sp++] = st.far;
        ref = st.any ? st.near : stack[--sp];
        continue;
      }
      const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u), cnt = ((ref >> kBvhSlotBits) & 15u) + 1u;
      for (uint32_t k = 0; k < cnt && !occ; ++k) {
        const float* lw = s.lrec + 16 * static_cast<size_t>(first + k);
        occ = cast_leaf_test(cast_rec_kind(lw), CastRec{lw}, r, t_max, t);
      }
      ref = stack[--sp];
    }
  }
  if (steps) *steps = nsteps;
  return occ;
}
#endif

}  // namespace fr

#if defined(__HIPCC__) || defined(__HIP__)

namespace fr {

constexpr uint32_t kCastBlock = 256;  // threads per workgroup: one ray each
// The wave counter (waves that walked the tree, waves that fell back to the list) is kept as
// kCastStripes pairs of words, one 128-byte line each, which fr_ctx_cast_info sums: a workgroup
// adds to the pair of its index modulo kCastStripes. One pair for all waves serialised 32,400
// adds to one address at 1080p, 0.34 ms of a 0.38 ms cast.
constexpr uint32_t kCastStripes = 256, kCastStripeWords = 32;
constexpr size_t kCastWaveBytes = static_cast<size_t>(kCastStripes) * kCastStripeWords * 4u;

// The scene tables the walks read (pack.h): GbScene's, and the tree's when n_segs > 0.
struct CastScene {
  GbScene gb;
  const float4* bvh;
  const uint32_t* bvh_order;
  const float4* lrec;
  const uint4* segs;
  uint32_t n_segs;  // 0: no tree, the list
  uint32_t levels;  // traversal-stack levels a lane can use (SceneFacts::bvh_levels)
  float reach;      // bvh_origin_reach
};

// Dynamic LDS of a tree launch: `levels` rows and the sentinel row, one u32 per lane each.
inline size_t cast_lds_bytes(uint32_t levels) { return (static_cast<size_t>(levels) + 1u) * kCastBlock * 4u; }

// Enqueues n rays (two float4 each: o, pad, d, pad) on `stream`; hit i lands in g0[i], g1[i],
// alb[i] (the G-buffer's words). tree: walk the scene's tree (sc.n_segs > 0). waves:
// kCastWaveBytes, zeroed by the caller; +1 per wave that walked the tree (word 0 of a stripe) /
// fell back to the list (word 1). ranged: a ray's second word's .w is its t_max;
// otherwise the word is not read and t_max is kCastTMax.
hipError_t launch_cast(hipStream_t stream, const CastScene& sc, bool tree, const float4* rays, uint32_t n, float4* g0,
                       float4* g1, float4* alb, uint32_t* waves, bool ranged = false);
// Occlusion queries (occlude.hip): out[i] = 1 if anything of the scene lies in
// (kGbTMin, t_max_i) of ray i, else 0; t_max_i is the second word's .w if ranged, else kCastTMax.
// waves: as launch_cast's, and word 2 of a stripe receives the wave's count of occluded rays.
hipError_t launch_occlude(hipStream_t stream, const CastScene& sc, bool tree, const float4* rays, uint32_t n, bool ranged,
                          uint8_t* out, uint32_t* waves);
// cast.hip's check of the tables a launch reads.
bool cast_scene_ok(const CastScene& sc, bool tree);
// fr_ctx_gbuffer through the tree: launch_gbuffer's contract for a scene with segments.
hipError_t launch_gbuffer_tree(hipStream_t stream, const CastScene& sc, const GbCam& cam, uint32_t W, uint32_t H, float4* g0,
                               float4* g1, float4* alb);

}  // namespace fr
#endif
