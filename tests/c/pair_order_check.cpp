// pair_order_check.cpp — host check of the mirrored box pair (rt_core.h slab_pair_root,
// slab_mirror_axis) against the list in order: slab3_fused + slab_root on the first box, then on
// the second with the first one's t as the bound. Built with -fsanitize=address,undefined and run
// directly (tests/test_pair_order_host.py). Prints one JSON line per pair shape; exits non-zero
// on the first mismatch of the hit decision, the winner's list index or the accepted t's bits.
//
// Shapes: scene_08's pairs (0, 1), (3, 4) and the shape of its boxes 2 and 5 set side by side, a
// separated pair on x and a touching pair on z, each in both list orders.
//
// Rays: every component of the origin and of the direction from {+-0, a denormal, 2^-101, 2^-100,
// 1, 2^125, FLT_MAX, inf (each with both signs), NaN, and the pair's plane coordinates on that
// axis with their neighbours one ulp away}. The box tests see a ray only through inv = RN(1 / d)
// clamped to +-2^100 and o inv per axis, and on the two shared axes only through the slab's two
// distances, so the combinations are taken over the distinct (inv, o inv) bit pairs of the
// mirrored axis and the distinct distance pairs of each shared axis: every combination of the
// components that the two forms can tell apart, each once. Bounds:
// FLT_MAX, and on a hit the accepted t itself (both forms must then refuse: t < t_max is strict)
// and its upper neighbour.
//
// With "ties" the program instead runs the constructed rays of a touching pair: origins strictly
// inside either box that leave through the shared plane (or away from it), |d| on the other axes
// small enough that this plane comes first. Prints per ray the shape's name, the two boxes
// (lo, hi of the first, then of the second), o, d, the winner's list index, t's bits and
// whether each box alone accepts that same t (a tie).
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../fo-rma_amd/csrc/rt_core.h"

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
static float from_bits(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}
static float up(float x) { return nextafterf(x, INFINITY); }
static float down(float x) { return nextafterf(x, -INFINITY); }

struct Box {
  float lo[3], hi[3];
};
struct Shape {
  const char* name;
  Box first, second;
  int axis;
};

// scene_08's coordinates as the packed records hold them
static const float k005 = from_bits(0x3d4ccccdu), k2995 = from_bits(0x41ef999au), k3005 = from_bits(0x41f06666u),
                   k3495 = from_bits(0x420bcccdu), k3505 = from_bits(0x420c3333u);

static std::vector<Shape> shapes() {
  const Box b0{{-k005, -30.0f, -35.0f}, {k005, 0.0f, 35.0f}}, b1{{-k005, 0.0f, -35.0f}, {k005, 30.0f, 35.0f}};
  const Box b2{{0.0f, -k3005, -35.0f}, {60.0f, -k2995, 35.0f}}, b5{{0.0f, k2995, -35.0f}, {60.0f, k3005, 35.0f}};
  const Box b3{{0.0f, -30.0f, k3495}, {60.0f, 30.0f, k3505}}, b4{{0.0f, -30.0f, -k3505}, {60.0f, 30.0f, -k3495}};
  const Box s0{{1.0f, -2.0f, -4.0f}, {3.0f, 2.0f, -2.0f}}, s1{{-3.0f, -2.0f, -4.0f}, {-1.0f, 2.0f, -2.0f}};
  const Box t0{{-1.0f, 0.5f, -2.0f}, {1.5f, 2.0f, 0.0f}}, t1{{-1.0f, 0.5f, 0.0f}, {1.5f, 2.0f, 2.0f}};
  return {{"scene08_0_1", b0, b1, 1}, {"scene08_1_0", b1, b0, 1}, {"scene08_3_4", b3, b4, 2}, {"scene08_4_3", b4, b3, 2},
          {"scene08_2_5", b2, b5, 1}, {"scene08_5_2", b5, b2, 1}, {"separated_x", s0, s1, 0}, {"separated_x_rev", s1, s0, 0},
          {"touching_z", t0, t1, 2},  {"touching_z_rev", t1, t0, 2}};
}

static fr::V3 v3(const float* p) { return fr::V3{p[0], p[1], p[2]}; }

// the list in order
static int in_order(const Shape& s, fr::V3 oinv, fr::V3 inv, float t_max, float& t_out) {
  float closest = t_max;
  int best = -1;
  const Box* bx[2] = {&s.first, &s.second};
  for (int i = 0; i < 2; ++i) {
    float t = 0.0f;
    if (fr::slab_root(fr::slab3_fused(v3(bx[i]->lo), v3(bx[i]->hi), oinv, inv), 0.001f, closest, t)) {
      closest = t;
      best = i;
    }
  }
  t_out = closest;
  return best;
}
// the pair form; the winner as a list index (0 = first)
static int paired(const Shape& s, fr::V3 oinv, fr::V3 inv, float t_max, float& t_out) {
  float t = 0.0f;
  bool first = false, h = false;
  const fr::V3 lo = v3(s.first.lo), hi = v3(s.first.hi);
  if (s.axis == 0) h = fr::slab_pair_root<0>(lo, hi, oinv, inv, 0.001f, t_max, t, first);
  if (s.axis == 1) h = fr::slab_pair_root<1>(lo, hi, oinv, inv, 0.001f, t_max, t, first);
  if (s.axis == 2) h = fr::slab_pair_root<2>(lo, hi, oinv, inv, 0.001f, t_max, t, first);
  t_out = h ? t : t_max;
  if (!h) return -1;
  return first ? 0 : 1;
}

static int compare(const Shape& s, fr::V3 oinv, fr::V3 inv, float t_max, unsigned long& hits, unsigned long& second_wins) {
  float ta = 0.0f, tb = 0.0f;
  const int a = in_order(s, oinv, inv, t_max, ta), b = paired(s, oinv, inv, t_max, tb);
  if (a != b || (a >= 0 && bits(ta) != bits(tb))) {
    fprintf(stderr,
            "pair_order_check: %s: in order (%d, %a) pair form (%d, %a) at inv (%a, %a, %a) oinv (%a, %a, %a) t_max %a\n",
            s.name, a, ta, b, tb, inv.x, inv.y, inv.z, oinv.x, oinv.y, oinv.z, t_max);
    return -1;
  }
  hits += a >= 0;
  second_wins += a == 1;
  return a >= 0 ? 1 : 0;
}

static std::vector<float> component_values(const Shape& s, int k) {
  const float mags[] = {0.0f, 0x1p-140f, 0x1p-101f, 0x1p-100f, 1.0f, 0x1p125f, FLT_MAX, INFINITY};
  std::vector<float> v;
  for (float m : mags) {
    v.push_back(m);
    v.push_back(-m);
  }
  v.push_back(NAN);
  for (const Box* b : {&s.first, &s.second})
    for (float c : {b->lo[k], b->hi[k]}) {
      v.push_back(c);
      v.push_back(up(c));
      v.push_back(down(c));
    }
  return v;
}

// One (inv, o inv) per distinct input of one axis over every (o, d) of its component values. On
// the mirrored axis an input is the bit pair (inv, o inv) itself. On a shared axis both forms see
// the ray only through the slab's two distances (slab_pair_d of lo and of hi, which the two boxes
// have in common), so an input is that pair of distances.
static std::vector<std::pair<float, float>> axis_inputs(const Shape& s, int k, unsigned long& combos) {
  const std::vector<float> vals = component_values(s, k);
  struct In {
    uint32_t a, b, inv, oinv;
  };
  std::vector<In> seen;
  for (float d : vals)
    for (float o : vals) {
      ++combos;
      const float inv = fr::box_inv_clamp(1.0f / d), oinv = o * inv;
      if (k == s.axis)
        seen.push_back({bits(inv), bits(oinv), bits(inv), bits(oinv)});
      else
        seen.push_back({bits(fr::slab_pair_d(s.first.lo[k], s.first.hi[k], s.first.lo[k], inv, oinv)),
                        bits(fr::slab_pair_d(s.first.lo[k], s.first.hi[k], s.first.hi[k], inv, oinv)), bits(inv), bits(oinv)});
    }
  std::sort(seen.begin(), seen.end(), [](const In& x, const In& y) {
    return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.inv != y.inv ? x.inv < y.inv : x.oinv < y.oinv;
  });
  std::vector<std::pair<float, float>> out;
  for (size_t i = 0; i < seen.size(); ++i)
    if (i == 0 || seen[i].a != seen[i - 1].a || seen[i].b != seen[i - 1].b)
      out.push_back({from_bits(seen[i].inv), from_bits(seen[i].oinv)});
  return out;
}

static int predicate_checks() {
  // what must and must not pair: slab_mirror_axis over two boxes' coordinates
  const auto axis = [](const Box& a, const Box& b) { return fr::slab_mirror_axis(a.lo, a.hi, b.lo, b.hi); };
  for (const Shape& s : shapes())
    if (axis(s.first, s.second) != s.axis) return fprintf(stderr, "pair_order_check: %s is not a pair\n", s.name), 1;
  const Box b{{-1.0f, 0.5f, -2.0f}, {1.5f, 2.0f, 0.0f}};
  Box m = b;  // the mirror image on z
  m.lo[2] = 0.0f, m.hi[2] = 2.0f;
  if (axis(b, m) != 2) return fprintf(stderr, "pair_order_check: the mirror image is not a pair\n"), 1;
  Box off = m;
  off.hi[2] = up(2.0f);  // one ulp off
  Box other = m;
  other.lo[0] = up(-1.0f);  // a shared slab one ulp off
  Box over = m;
  over.lo[2] = -1.0f, over.hi[2] = 2.0f;  // not a mirror image
  Box huge_a{{-1.0f, 0.5f, -0x1p28f}, {1.5f, 2.0f, -1.0f}}, huge_b{{-1.0f, 0.5f, 1.0f}, {1.5f, 2.0f, 0x1p28f}};
  Box flat_a{{-1.0f, 0.5f, 0.0f}, {1.5f, 2.0f, 0.0f}};
  Box straddle_a{{-1.0f, 0.5f, -1.0f}, {1.5f, 2.0f, 2.0f}}, straddle_b{{-1.0f, 0.5f, -2.0f}, {1.5f, 2.0f, 1.0f}};
  if (axis(b, off) != -1 || axis(b, other) != -1 || axis(b, over) != -1 || axis(b, b) != -1 ||
      axis(huge_a, huge_b) != -1 || axis(flat_a, flat_a) != -1 || axis(straddle_a, straddle_b) != -1)
    return fprintf(stderr, "pair_order_check: a pair that must not specialise does\n"), 1;
  return 0;
}

static int tie_rays() {
  for (const Shape& s : shapes()) {
    if (strncmp(s.name, "scene08_0_1", 11) && strncmp(s.name, "scene08_1_0", 11) && strncmp(s.name, "touching_z", 10))
      continue;
    const int ax = s.axis, u = (ax + 1) % 3, v = (ax + 2) % 3;
    // inside both shared slabs, near their lower faces; half the mirrored extent from the plane
    const float half = 0.5f * std::max(fabsf(s.first.lo[ax]), fabsf(s.first.hi[ax]));
    for (float side : {-1.0f, 1.0f})
      for (float dir : {-1.0f, 1.0f}) {
        float o[3], d[3];
        o[ax] = side * half, d[ax] = dir;
        o[u] = s.first.lo[u] + 0.25f * (s.first.hi[u] - s.first.lo[u]), d[u] = 0x1p-12f * (s.first.hi[u] - s.first.lo[u]);
        o[v] = s.first.lo[v] + 0.25f * (s.first.hi[v] - s.first.lo[v]), d[v] = -0x1p-12f * (s.first.hi[v] - s.first.lo[v]);
        const fr::V3 inv{fr::box_inv_clamp(1.0f / d[0]), fr::box_inv_clamp(1.0f / d[1]), fr::box_inv_clamp(1.0f / d[2])};
        const fr::V3 oinv{o[0] * inv.x, o[1] * inv.y, o[2] * inv.z};
        unsigned long hits = 0, second = 0;
        if (compare(s, oinv, inv, FLT_MAX, hits, second) < 0) return 1;
        float t = 0.0f;
        const int w = in_order(s, oinv, inv, FLT_MAX, t);
        // a tie: each box alone accepts the same t
        float t0 = 0.0f, t1 = 0.0f;
        const bool h0 = fr::slab_root(fr::slab3_fused(v3(s.first.lo), v3(s.first.hi), oinv, inv), 0.001f, FLT_MAX, t0);
        const bool h1 = fr::slab_root(fr::slab3_fused(v3(s.second.lo), v3(s.second.hi), oinv, inv), 0.001f, FLT_MAX, t1);
        printf("%s", s.name);
        for (const Box* b : {&s.first, &s.second})
          printf(" %a %a %a %a %a %a", b->lo[0], b->lo[1], b->lo[2], b->hi[0], b->hi[1], b->hi[2]);
        printf(" %a %a %a %a %a %a %d %08x %d\n", o[0], o[1], o[2], d[0], d[1], d[2], w, bits(t),
               int(h0 && h1 && bits(t0) == bits(t1)));
      }
  }
  return 0;
}

// every ray of one shape; the JSON line, or empty after a mismatch
static std::string run_shape(const Shape& s) {
  unsigned long combos[3] = {0, 0, 0}, rays = 0, tests = 0, hits = 0, second_wins = 0;
  std::vector<std::pair<float, float>> in[3];
  for (int k = 0; k < 3; ++k) in[k] = axis_inputs(s, k, combos[k]);
  for (auto& x : in[0])
    for (auto& y : in[1])
      for (auto& z : in[2]) {
        ++rays;
        const fr::V3 inv{x.first, y.first, z.first}, oinv{x.second, y.second, z.second};
        ++tests;
        const int h = compare(s, oinv, inv, FLT_MAX, hits, second_wins);
        if (h < 0) return "";
        if (h) {
          float t = 0.0f;
          in_order(s, oinv, inv, FLT_MAX, t);
          tests += 2;
          unsigned long none = 0, dummy = 0;
          if (compare(s, oinv, inv, t, none, dummy) < 0 || compare(s, oinv, inv, up(t), dummy, dummy) < 0) return "";
          if (none) return fprintf(stderr, "pair_order_check: %s: a hit at its own bound\n", s.name), "";
        }
      }
  char line[512];
  snprintf(line, sizeof line,
           "{\"shape\": \"%s\", \"axis\": %d, \"component_combos\": [%lu, %lu, %lu], \"distinct\": [%zu, %zu, %zu], "
           "\"rays\": %lu, \"tests\": %lu, \"hits\": %lu, \"second_wins\": %lu}\n",
           s.name, s.axis, combos[0], combos[1], combos[2], in[0].size(), in[1].size(), in[2].size(), rays, tests, hits,
           second_wins);
  return line;
}

int main(int argc, char** argv) {
  if (predicate_checks()) return 1;
  if (argc > 1 && !strcmp(argv[1], "ties")) return tie_rays();
  // the shapes are independent: one thread each
  const std::vector<Shape> sh = shapes();
  std::vector<std::string> lines(sh.size());
  std::vector<std::thread> th;
  for (size_t i = 0; i < sh.size(); ++i) th.emplace_back([&, i] { lines[i] = run_shape(sh[i]); });
  for (auto& t : th) t.join();
  for (const std::string& ln : lines) {
    if (ln.empty()) return 1;
    fputs(ln.c_str(), stdout);
  }
  return 0;
}
