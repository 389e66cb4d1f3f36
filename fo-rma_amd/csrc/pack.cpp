// pack.cpp — pack_scene (pack.h): the primitive list as the kernels' tables. Host f32
// under the Makefile's numerics rule (no contraction): the triangle normal is formed
// exactly as the oracle forms it.
#include "pack.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "bvh.h"
#include "refit.h"
#include "rt_core.h"

namespace fr {

// Effective scatter class after each shape's fallback chain
// (sphere.rs:56-69: 0/1/2/3 else lambertian; plane.rs:48-59: 1 metal else lambertian).
static uint32_t scatter_class(const fr_prim& p) {
  if (p.kind == FR_STUB) return SC_NONE;
  if (p.kind == FR_PLANE) return p.material == FR_METAL ? SC_METAL : SC_LAMBERT;
  switch (p.material) {
    case FR_METAL: return SC_METAL;
    case FR_DIELECTRIC: return SC_DIELECTRIC;
    case FR_LIGHT: return SC_LIGHT;
    default: return SC_LAMBERT;
  }
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct F4 {
  float x, y, z, w;
};

void pack_record(const fr_prim& p, float rec[16]) {
  uint32_t kind = p.kind;
  F4 g[4] = {};
  switch (p.kind) {
    case FR_SPHERE: g[0] = F4{p.g[0], p.g[1], p.g[2], p.g[3]}; break;
    case FR_AABB:
      g[0] = F4{p.g[0], p.g[1], p.g[2], 0.0f};
      g[1] = F4{p.g[3], p.g[4], p.g[5], 0.0f};
      break;
    case FR_PLANE:
      g[0] = F4{p.g[0], p.g[1], p.g[2], 0.0f};
      g[1] = F4{p.g[3], p.g[4], p.g[5], 0.0f};
      g[2] = F4{p.g[6], p.g[7], p.g[8], 0.0f};
      break;
    case FR_OBB:
      g[0] = F4{p.g[0], p.g[1], p.g[2], p.g[12]};
      g[1] = F4{p.g[3], p.g[4], p.g[5], p.g[13]};
      g[2] = F4{p.g[6], p.g[7], p.g[8], p.g[14]};
      g[3] = F4{p.g[9], p.g[10], p.g[11], 0.0f};
      break;
    case FR_TRIANGLE: {
      // v0, edges e1 = v1 - v0 and e2 = v2 - v0, and the unit winding normal
      // unit(cross(e1, e2)), all in host f32 exactly as the oracle forms them
      const V3 v0{p.g[0], p.g[1], p.g[2]};
      const V3 e1 = sub(V3{p.g[3], p.g[4], p.g[5]}, v0), e2 = sub(V3{p.g[6], p.g[7], p.g[8]}, v0);
      const V3 nw = unit(cross(e1, e2));
      g[0] = F4{v0.x, v0.y, v0.z, 0.0f};
      g[1] = F4{e1.x, e1.y, e1.z, 0.0f};
      g[2] = F4{e2.x, e2.y, e2.z, 0.0f};
      g[3] = F4{nw.x, nw.y, nw.z, 0.0f};
      break;
    }
    default: kind = FR_STUB;
  }
  memcpy(&g[3].w, &kind, 4);  // kind bits in g3.w
  memcpy(rec, g, 64);
}

void leaf_record(const float rec[16], float lrec[16]) {
  memcpy(lrec, rec, 64);
  uint32_t kind;
  memcpy(&kind, &lrec[15], 4);
  if (kind == FR_SPHERE) lrec[3] = lrec[3] * lrec[3];
}

PackedScene pack_scene(const std::vector<fr_prim>& prims, bool force_bvh) {
  PackedScene c;
  const uint32_t n = static_cast<uint32_t>(prims.size());
  const size_t m = n ? n : 1;  // never hand the kernel a null array
  // BVH runs between planes for scenes of kBvhMinPrims or more (bvh.h)
  std::vector<BvhSegment> bvh_segs;
  std::vector<BvhNode> bvh_nodes;
  std::vector<uint32_t> bvh_order;
  float bvh_extent = 0.0f;
  const bool bvh_ok = build_segments(prims, bvh_segs, bvh_nodes, bvh_order, force_bvh, &bvh_extent);
  if (!bvh_ok) {
    bvh_segs.clear();
    bvh_nodes.clear();
    bvh_order.clear();
  }
  // kind runs: maximal runs of consecutive primitives of one kind, in list order
  std::vector<uint32_t> runs;
  for (uint32_t i = 0; i < n;) {
    const uint32_t k = prims[i].kind <= FR_TRIANGLE ? prims[i].kind : FR_STUB;
    uint32_t j = i + 1;
    while (j < n && (prims[j].kind <= FR_TRIANGLE ? prims[j].kind : FR_STUB) == k) ++j;
    runs.insert(runs.end(), {k, i, j, 0u});
    i = j;
  }
  c.n_runs = static_cast<uint32_t>(runs.size() / 4);
  size_t off = 0;
  auto table = [&off](size_t& at, size_t bytes) {
    at = off;
    off = align_up(off + bytes, 256);
  };
  table(c.off_mat, m * 16);
  table(c.off_cls, m * 4);
  table(c.off_att, (static_cast<size_t>(n) + 1) * 16);  // + the unit entry
  table(c.off_rec, m * 64);
  table(c.off_bvh, (bvh_nodes.size() ? bvh_nodes.size() : 1) * sizeof(BvhNode));
  table(c.off_bvh_order, (bvh_order.size() ? bvh_order.size() : 1) * 4);
  table(c.off_lrec, (bvh_order.size() ? bvh_order.size() : 1) * 64);
  table(c.off_segs, (bvh_segs.size() ? bvh_segs.size() : 1) * sizeof(BvhSegment));
  table(c.off_runs, (runs.size() ? runs.size() : 4) * 4);
  table(c.off_acls, m * 4);
  table(c.off_acls_att, (kNibbleMaxPrims + 1) * 16);
  // the refit's tables (refit.h), after everything the trace and walk kernels read
  table(c.off_slot_bounds, (bvh_order.size() ? bvh_order.size() : 1) * sizeof(RefitBox));
  table(c.off_slot_of, m * 4);
  table(c.off_unions, (bvh_nodes.size() ? bvh_nodes.size() : 1) * sizeof(RefitBox));
  table(c.off_sched, (bvh_nodes.size() ? bvh_nodes.size() : 1) * 4);
  std::vector<unsigned char>& host = c.bytes;
  host.assign(off, 0);
  std::vector<F4> aclass;  // distinct attenuations, first appearance order
  bool aclass_ok = true;
  if (!bvh_nodes.empty()) memcpy(&host[c.off_bvh], bvh_nodes.data(), bvh_nodes.size() * sizeof(BvhNode));
  if (!bvh_order.empty()) memcpy(&host[c.off_bvh_order], bvh_order.data(), bvh_order.size() * 4);
  if (!bvh_segs.empty()) memcpy(&host[c.off_segs], bvh_segs.data(), bvh_segs.size() * sizeof(BvhSegment));
  if (!runs.empty()) memcpy(&host[c.off_runs], runs.data(), runs.size() * 4);
  SceneFacts& sf = c.facts;
  sf.n = n;
  sf.bvh_ok = bvh_ok;
  sf.bvh_extent = bvh_extent;
  sf.bvh_sphere_rmin = bvh_sphere_rmin(prims);
  sf.n_segs = static_cast<uint32_t>(bvh_segs.size());
  sf.bvh_levels = bvh_ok ? std::min(bvh_max_depth(bvh_segs, bvh_nodes) + 1u, kBvhStack) : kBvhStack;
  for (uint32_t i = 0; i < n; ++i) {
    const fr_prim& p = prims[i];
    const uint32_t cls = scatter_class(p);
    if (cls == SC_METAL || cls == SC_DIELECTRIC) sf.diffuse = false;
    const F4 mat{p.color[0], p.color[1], p.color[2], p.fuzz};
    const F4 att = cls == SC_LIGHT ? F4{1.0f, 1.0f, 1.0f, 0.0f} : F4{p.color[0], p.color[1], p.color[2], 0.0f};
    memcpy(&host[c.off_mat + 16 * i], &mat, 16);
    memcpy(&host[c.off_cls + 4 * i], &cls, 4);
    memcpy(&host[c.off_att + 16 * i], &att, 16);
    {
      uint32_t k = 0;
      while (k < aclass.size() && memcmp(&aclass[k], &att, 12) != 0) ++k;
      if (k == aclass.size()) {
        if (aclass.size() < kNibbleMaxPrims)
          aclass.push_back(att);
        else
          aclass_ok = false;
      }
      const uint32_t kc = k < kNibbleMaxPrims ? k : 0u;
      memcpy(&host[c.off_acls + 4 * i], &kc, 4);
    }
    for (float a : {att.x, att.y, att.z})
      if (!(a >= 0.0f) || std::signbit(a) || !std::isfinite(a)) c.att_nonneg = false;
    float rec[16];
    pack_record(p, rec);
    memcpy(&host[c.off_rec + 64 * i], rec, 64);
    sf.has_plane |= p.kind == FR_PLANE;
    sf.kinds |= 1u << (p.kind <= FR_TRIANGLE ? p.kind : FR_STUB);
  }
  c.rec_words.resize(16u * static_cast<size_t>(n));
  if (n) memcpy(c.rec_words.data(), &host[c.off_rec], 64u * static_cast<size_t>(n));
  sf.n_aclass = aclass_ok && n ? static_cast<uint32_t>(aclass.size()) : 0u;
  const F4 one{1.0f, 1.0f, 1.0f, 0.0f};
  for (uint32_t k = 0; k <= kNibbleMaxPrims; ++k) {  // entries past the classes: the unit attenuation
    const F4 a = k < aclass.size() ? aclass[k] : one;
    memcpy(&host[c.off_acls_att + 16 * k], &a, 16);
  }
  // the BVH leaves' records, in leaf-slot order; a sphere's carries RN(radius^2) in place of
  // its radius, the product its hit test forms (sphere.rs:34; one VALU per leaf test saved)
  for (size_t slot = 0; slot < bvh_order.size(); ++slot) {
    float rec[16], lr[16];
    memcpy(rec, &host[c.off_rec + 64 * static_cast<size_t>(bvh_order[slot])], 64);
    leaf_record(rec, lr);
    memcpy(&host[c.off_lrec + 64 * slot], lr, 64);
  }
  // the refit's tables: each slot's bounds as the builder took them, the slot of each primitive,
  // the nodes' unpadded unions (bvh_refit over a copy of the nodes, which it reproduces) and the
  // height schedule
  c.slot_of.assign(m, kNoSlot);
  c.n_slots = static_cast<uint32_t>(bvh_order.size());
  c.n_nodes = static_cast<uint32_t>(bvh_nodes.size());
  if (bvh_ok) {
    const float reach = bvh_origin_reach(bvh_extent, sf.bvh_sphere_rmin);
    std::vector<RefitBox> sb(bvh_order.size());
    for (size_t slot = 0; slot < bvh_order.size(); ++slot) {
      c.slot_of[bvh_order[slot]] = static_cast<uint32_t>(slot);
      (void)bvh_prim_bounds(prims[bvh_order[slot]], reach, &sb[slot]);
    }
    c.sched = bvh_refit_schedule(bvh_nodes);
    std::vector<RefitBox> unions;
    std::vector<BvhNode> copy = bvh_nodes;  // (the blob holds the builder's own nodes)
    bvh_refit(copy, c.sched, sb, 1e-4f * bvh_extent + 1e-4f, unions);
    if (!sb.empty()) memcpy(&host[c.off_slot_bounds], sb.data(), sb.size() * sizeof(RefitBox));
    if (!unions.empty()) memcpy(&host[c.off_unions], unions.data(), unions.size() * sizeof(RefitBox));
    if (!c.sched.ids.empty()) memcpy(&host[c.off_sched], c.sched.ids.data(), c.sched.ids.size() * 4);
  }
  memcpy(&host[c.off_slot_of], c.slot_of.data(), m * 4);
  // entry n: the unit attenuation the depth-8 stack's empty levels point at
  memcpy(&host[c.off_att + 16 * n], &one, 16);
  if (n == 0) {
    const uint32_t stub = FR_STUB;
    memcpy(&host[c.off_rec + 60], &stub, 4);
  }
  return c;
}

}  // namespace fr
