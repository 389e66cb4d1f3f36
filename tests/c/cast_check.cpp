// cast_check.cpp — test harness (tests/test_cast_host.py): the ray queries' definition
// (fo-rma_amd/csrc/cast.h) as a CPU program, built with -fsanitize=address,undefined
// -fno-sanitize-recover=all -ffp-contract=off together with the host's scene packer and tree
// builder (fo-rma_amd/csrc/pack.cpp, bvh.cpp).
//   cast_check FILE   FILE holds u32 words: n, m, W, H, the bits of a camera's position,
//                     lower_left, horizontal and vertical (12 words), then n fr_prim (22 words
//                     each), then m rays (8 words each: o, pad, d, pad).
// For every ray it walks the list in order (cast_walk_list) and, where the scene has a tree and
// the ray passes cast_fallback, the tree (cast_walk_tree), and counts the rays whose winner or
// root bits differ. It also checks, for every pixel of the W x H view, that cast_ray of the
// pixel ray's o and d has the bits of gb_primary_ray, and, for every leaf slot, that a sphere's
// leaf-order record carries the product RN(r r) that sphere_root forms from the list record.
// For every ray that passes cast_fallback and whose list winner is a sphere, it checks in double
// that the ray passes the centre within bvh_sphere_bound (bvh.h), the ball the builder bounds the
// sphere by. Prints one line
//   info tree T segs S nodes N levels L reach R(hex) fallback F steps K mismatch M pixel_ray P rr Q bound B
// then one line per ray in hex: the list loop's id, the bits of t, N, P and the albedo (11 words),
// and a 12th word, 1 if the ray falls back. Exit status 1 if M, P, Q or B is not 0.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../fo-rma_amd/csrc/cast.h"
#include "../../fo-rma_amd/csrc/pack.h"

namespace {

float as_f32(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
bool same_ray(const fr::GbRay& a, const fr::GbRay& b) {
  const float x[13] = {a.o.x, a.o.y, a.o.z, a.d.x, a.d.y, a.d.z, a.inv.x, a.inv.y, a.inv.z, a.oinv.x, a.oinv.y, a.oinv.z, a.a};
  const float y[13] = {b.o.x, b.o.y, b.o.z, b.d.x, b.d.y, b.d.z, b.inv.x, b.inv.y, b.inv.z, b.oinv.x, b.oinv.y, b.oinv.z, b.a};
  return memcmp(x, y, sizeof(x)) == 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: cast_check FILE\n");
    return 2;
  }
  std::vector<uint32_t> in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t buf[1024];
  size_t got;
  while ((got = fread(buf, 4, 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  static_assert(sizeof(fr_prim) == 88, "22 words per primitive");
  if (in.size() < 16) return 2;
  const uint32_t n = in[0], m = in[1], W = in[2], H = in[3];
  if (W > 4096 || H > 4096 || in.size() != 16 + static_cast<size_t>(n) * 22 + static_cast<size_t>(m) * 8) return 2;
  float c[12];
  for (int k = 0; k < 12; ++k) c[k] = as_f32(in[4 + k]);
  const fr::GbCam cam{fr::V3{c[0], c[1], c[2]}, fr::V3{c[3], c[4], c[5]}, fr::V3{c[6], c[7], c[8]}, fr::V3{c[9], c[10], c[11]}};
  std::vector<fr_prim> prims(n);
  if (n) memcpy(prims.data(), in.data() + 16, static_cast<size_t>(n) * 88);
  const uint32_t* rays = in.data() + 16 + static_cast<size_t>(n) * 22;
  const fr::PackedScene ps = fr::pack_scene(prims, false);
  const unsigned char* blob = ps.bytes.data();
  fr::CastTables tb;
  tb.rec = reinterpret_cast<const float*>(blob + ps.off_rec);
  tb.lrec = reinterpret_cast<const float*>(blob + ps.off_lrec);
  tb.order = reinterpret_cast<const uint32_t*>(blob + ps.off_bvh_order);
  tb.nodes = reinterpret_cast<const fr::BvhNode*>(blob + ps.off_bvh);
  tb.segs = reinterpret_cast<const fr::BvhSegment*>(blob + ps.off_segs);
  tb.runs = reinterpret_cast<const uint32_t*>(blob + ps.off_runs);
  tb.n_runs = ps.n_runs;
  tb.n_segs = ps.facts.bvh_ok ? ps.facts.n_segs : 0u;
  const uint32_t* cls = reinterpret_cast<const uint32_t*>(blob + ps.off_cls);
  const float* att = reinterpret_cast<const float*>(blob + ps.off_att);
  const bool tree = tb.n_segs > 0;
  const float reach = fr::bvh_origin_reach(ps.facts.bvh_extent, ps.facts.bvh_sphere_rmin);

  // cast_ray of a pixel ray against gb_primary_ray
  uint32_t bad_pixel = 0;
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const fr::GbRay p = fr::gb_primary_ray(cam, x, y, W, H);
      if (!same_ray(p, fr::cast_ray(p.o, p.d))) ++bad_pixel;
    }

  // the sphere leaf records' product: sphere_root forms radius * radius from the list record
  uint32_t bad_rr = 0, n_nodes = 0;
  if (tree) {
    // (upper bounds: the tables are padded to 256 B, and the blob holds the padding)
    n_nodes = static_cast<uint32_t>((ps.off_bvh_order - ps.off_bvh) / sizeof(fr::BvhNode));
    const size_t slots = (ps.off_lrec - ps.off_bvh_order) / 4;
    // the slots in use are those a leaf references: walk every leaf of every tree
    std::vector<uint32_t> todo;
    for (uint32_t sg = 0; sg < tb.n_segs; ++sg)
      if (!tb.segs[sg].plane && tb.segs[sg].root != fr::kBvhEnd) todo.push_back(tb.segs[sg].root);
    while (!todo.empty()) {
      const uint32_t ref = todo.back();
      todo.pop_back();
      if (ref < fr::kBvhLeaf) {
        if (ref >= n_nodes) return 3;
        todo.push_back(tb.nodes[ref].ref[0]);
        todo.push_back(tb.nodes[ref].ref[1]);
        continue;
      }
      const uint32_t first = ref & ((1u << fr::kBvhSlotBits) - 1u), cnt = ((ref >> fr::kBvhSlotBits) & 15u) + 1u;
      for (uint32_t k = 0; k < cnt; ++k) {
        const size_t slot = first + k;
        if (slot >= slots) return 3;
        const uint32_t i = tb.order[slot];
        if (i >= n) return 3;
        const float* lw = tb.lrec + 16 * slot;
        const float* w = tb.rec + 16 * static_cast<size_t>(i);
        if (fr::cast_rec_kind(lw) != fr::cast_rec_kind(w)) ++bad_rr;
        if (fr::cast_rec_kind(w) == FR_SPHERE) {
          const float radius = w[3];
          const float rr = radius * radius;  // sphere_root's product (no contraction: one rounding)
          if (bits(rr) != bits(lw[3]) || memcmp(lw, w, 12) != 0) ++bad_rr;
        } else if (memcmp(lw, w, 64) != 0) {
          ++bad_rr;
        }
      }
    }
  }

  uint32_t n_fallback = 0, mismatch = 0, bad_bound = 0;
  unsigned long long steps = 0;
  std::vector<uint32_t> lines(static_cast<size_t>(m) * 12);
  for (uint32_t q = 0; q < m; ++q) {
    const uint32_t* w = rays + 8 * static_cast<size_t>(q);
    const fr::GbRay r = fr::cast_ray(fr::V3{as_f32(w[0]), as_f32(w[1]), as_f32(w[2])}, fr::V3{as_f32(w[4]), as_f32(w[5]), as_f32(w[6])});
    float closest;
    int best;
    fr::cast_walk_list(tb, r, closest, best);
    const bool fb = fr::cast_fallback(r, fr::cast_cull(r), reach);
    n_fallback += fb ? 1u : 0u;
    if (tree && !fb) {
      float tc;
      int tbest;
      uint32_t st = 0;
      fr::cast_walk_tree(tb, r, tc, tbest, &st);
      steps += st;
      if (tbest != best || bits(tc) != bits(closest)) {
        if (mismatch < 8)
          fprintf(stderr, "ray %u: list %d %08x tree %d %08x\n", q, best, bits(closest), tbest, bits(tc));
        ++mismatch;
      }
    }
    if (!fb && best >= 0 && prims[best].kind == FR_SPHERE) {
      // the distance at which the ray passes the winner's centre: |oc x d| / |d|
      const float* g = prims[best].g;
      const double oc[3] = {static_cast<double>(r.o.x) - g[0], static_cast<double>(r.o.y) - g[1], static_cast<double>(r.o.z) - g[2]};
      const double dd[3] = {r.d.x, r.d.y, r.d.z};
      const double cx[3] = {oc[1] * dd[2] - oc[2] * dd[1], oc[2] * dd[0] - oc[0] * dd[2], oc[0] * dd[1] - oc[1] * dd[0]};
      const double pass = sqrt((cx[0] * cx[0] + cx[1] * cx[1] + cx[2] * cx[2]) / (dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]));
      if (!(pass <= static_cast<double>(fr::bvh_sphere_bound(g, fabsf(g[3]), reach)))) ++bad_bound;
    }
    fr::GbPixel p = fr::gb_miss();
    if (best >= 0) {
      const fr::CastRec rec{tb.rec + 16 * static_cast<size_t>(best)};
      const float* a = att + 4 * static_cast<size_t>(best);
      p = fr::gb_hit(static_cast<uint32_t>(best), bits(rec.w[15]), cls[best], rec, fr::GbF4{a[0], a[1], a[2], a[3]}, r, closest);
    }
    const uint32_t line[12] = {fr::gb_id(p.g1), bits(p.g0.w), bits(p.g0.x), bits(p.g0.y), bits(p.g0.z), bits(p.g1.x),
                               bits(p.g1.y), bits(p.g1.z), bits(p.alb.x), bits(p.alb.y), bits(p.alb.z), fb ? 1u : 0u};
    memcpy(&lines[12 * static_cast<size_t>(q)], line, sizeof(line));
  }
  printf("info tree %u segs %u nodes %u levels %u reach %08x fallback %u steps %llu mismatch %u pixel_ray %u rr %u bound %u\n",
         tree ? 1u : 0u, tb.n_segs, n_nodes, ps.facts.bvh_levels, bits(reach), n_fallback, steps, mismatch, bad_pixel, bad_rr, bad_bound);
  for (uint32_t q = 0; q < m; ++q) {
    const uint32_t* l = &lines[12 * static_cast<size_t>(q)];
    printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %u\n", l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8],
           l[9], l[10], l[11]);
  }
  return mismatch || bad_pixel || bad_rr || bad_bound ? 1 : 0;
}
