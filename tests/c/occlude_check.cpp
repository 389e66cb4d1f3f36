// occlude_check.cpp — test harness (tests/test_occlude_host.py): the ranged closest hit and the
// any-hit walks of fo-rma_amd/csrc/cast.h as a CPU program, built with
// -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off together with the
// host's scene packer and tree builder (fo-rma_amd/csrc/pack.cpp, bvh.cpp).
//   occlude_check FILE   FILE holds u32 words: n, m, then n fr_prim (22 words each), then m rays
//                        (8 words each: o, pad, d, t_max).
// For every ray it walks the list from closest = t_max (cast_walk_list) and tests the list
// against t_max (occl_walk_list); where the scene has a tree and the ray passes cast_fallback it
// walks the tree both ways (cast_walk_tree, occl_walk_tree). It counts
//   ranged:  the rays whose ranged tree walk's winner or root bits differ from the ranged list's,
//   anyhit:  the rays whose any-hit tree walk differs from the any-hit list,
//   equiv:   the rays whose any-hit list differs from "the ranged list found a winner".
// Prints one line
//   info tree T fallback F steps K osteps L ranged A anyhit B equiv C
// (steps / osteps: node steps of the ranged / any-hit tree walks) then one line per ray in hex:
// the ranged list loop's id, the bits of t, N, P and the albedo (11 words), 1 if the ray falls
// back, and the any-hit list's answer. Exit status 1 if A, B or C is not 0.
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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: occlude_check FILE\n");
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
  if (in.size() < 2) return 2;
  const uint32_t n = in[0], m = in[1];
  if (in.size() != 2 + static_cast<size_t>(n) * 22 + static_cast<size_t>(m) * 8) return 2;
  std::vector<fr_prim> prims(n);
  if (n) memcpy(prims.data(), in.data() + 2, static_cast<size_t>(n) * 88);
  const uint32_t* rays = in.data() + 2 + static_cast<size_t>(n) * 22;
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

  uint32_t n_fallback = 0, bad_ranged = 0, bad_anyhit = 0, bad_equiv = 0;
  unsigned long long steps = 0, osteps = 0;
  std::vector<uint32_t> lines(static_cast<size_t>(m) * 13);
  for (uint32_t q = 0; q < m; ++q) {
    const uint32_t* w = rays + 8 * static_cast<size_t>(q);
    const fr::GbRay r = fr::cast_ray(fr::V3{as_f32(w[0]), as_f32(w[1]), as_f32(w[2])}, fr::V3{as_f32(w[4]), as_f32(w[5]), as_f32(w[6])});
    const float t_max = as_f32(w[7]);
    float closest;
    int best;
    fr::cast_walk_list(tb, r, closest, best, t_max);
    const bool occ = fr::occl_walk_list(tb, r, t_max);
    if (occ != (best >= 0)) {
      if (bad_equiv < 8) fprintf(stderr, "ray %u: any-hit list %d, ranged list winner %d\n", q, occ ? 1 : 0, best);
      ++bad_equiv;
    }
    const bool fb = fr::cast_fallback(r, fr::cast_cull(r), reach);
    n_fallback += fb ? 1u : 0u;
    if (tree && !fb) {
      float tc;
      int tbest;
      uint32_t st = 0, ost = 0;
      fr::cast_walk_tree(tb, r, tc, tbest, &st, t_max);
      steps += st;
      if (tbest != best || bits(tc) != bits(closest)) {
        if (bad_ranged < 8) fprintf(stderr, "ray %u: list %d %08x tree %d %08x\n", q, best, bits(closest), tbest, bits(tc));
        ++bad_ranged;
      }
      const bool tocc = fr::occl_walk_tree(tb, r, t_max, &ost);
      osteps += ost;
      if (tocc != occ) {
        if (bad_anyhit < 8) fprintf(stderr, "ray %u: any-hit list %d tree %d\n", q, occ ? 1 : 0, tocc ? 1 : 0);
        ++bad_anyhit;
      }
    }
    fr::GbPixel p = fr::gb_miss();
    if (best >= 0) {
      const fr::CastRec rec{tb.rec + 16 * static_cast<size_t>(best)};
      const float* a = att + 4 * static_cast<size_t>(best);
      p = fr::gb_hit(static_cast<uint32_t>(best), bits(rec.w[15]), cls[best], rec, fr::GbF4{a[0], a[1], a[2], a[3]}, r, closest);
    }
    const uint32_t line[13] = {fr::gb_id(p.g1), bits(p.g0.w), bits(p.g0.x), bits(p.g0.y), bits(p.g0.z), bits(p.g1.x), bits(p.g1.y),
                               bits(p.g1.z), bits(p.alb.x), bits(p.alb.y), bits(p.alb.z), fb ? 1u : 0u, occ ? 1u : 0u};
    memcpy(&lines[13 * static_cast<size_t>(q)], line, sizeof(line));
  }
  printf("info tree %u fallback %u steps %llu osteps %llu ranged %u anyhit %u equiv %u\n", tree ? 1u : 0u, n_fallback, steps,
         osteps, bad_ranged, bad_anyhit, bad_equiv);
  for (uint32_t q = 0; q < m; ++q) {
    const uint32_t* l = &lines[13 * static_cast<size_t>(q)];
    printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %u %u\n", l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8],
           l[9], l[10], l[11], l[12]);
  }
  return bad_ranged || bad_anyhit || bad_equiv ? 1 : 0;
}
