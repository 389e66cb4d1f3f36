// guard_root_check.cpp — host check of the segment's reciprocal guard (rt_core.h recip_box_ok3)
// and of the box root selection (slab_root), against local copies of the forms they replace or
// were weighed against. Built with -fsanitize=address,undefined and run directly
// (tests/test_guard_root_host.py). Prints one JSON line; exits non-zero on the first violation.
//
// Guard. Components from {+-0, a denormal, 2^-101, 2^-100 and its neighbours, 1, 2^125, 2^126 and
// its neighbours, FLT_MAX, +-inf, NaN}, both signs, all triples:
//   - recip_box_ok3(d) implies the old per-component guard on every component (never fewer
//     segments to the fallback);
//   - on every component the old guard admits, the fallback's clamped IEEE reciprocal has the bits
//     of RN(1 / x), which is what the fast path returns there (recip_nr's contract, checked
//     exhaustively on the device): a triple the new guard refuses although the old one admitted
//     it gets the same reciprocals;
//   - a NaN or infinite component is always refused.
// With "triples" the program prints every triple and the reciprocals the contract asks for
// (RN(1 / x) clamped to +-2^100), for the device test to compare the kernel's against.
//
// Root. tn, tf, t_max from {NaN, +-inf, +-0, t_min and its neighbours, 1, 2, equal pairs}, all
// combinations: slab_root against the local copy of its expression (same decision, same t on a
// hit), and the candidate max(tn, t_min) < tf form that was not taken: it differs exactly where
// tn is NaN and tf is not (maxNum drops the NaN), which the program counts.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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

// the guard before: per component, 2^-100 <= |x| < 2^126
static bool old_ok(float x) {
  const float ax = fabsf(x);
  return (ax >= 0x1p-100f) & (ax < 0x1p126f);
}
// slab_root's expression before (and now)
static bool old_root(float tn, float tf, float t_min, float t_max, float& t) {
  t = tn > t_min ? tn : tf;
  return (t > t_min) & (t < t_max) & (tn < tf);
}
// the candidate: one max and one compare for the geometric part
static bool max_root(float tn, float tf, float t_min, float t_max, float& t) {
  t = tn > t_min ? tn : tf;
  return (fr::fmax_num(tn, t_min) < tf) & (t < t_max);
}

static std::vector<float> guard_values() {
  const float mags[] = {0.0f, 0x1p-140f, 0x1p-101f, down(0x1p-100f), 0x1p-100f, up(0x1p-100f), 1.0f, 0x1p125f,
                        down(0x1p126f), 0x1p126f, up(0x1p126f), FLT_MAX, INFINITY};
  std::vector<float> v;
  for (float m : mags) {
    v.push_back(m);
    v.push_back(-m);
  }
  v.push_back(NAN);
  v.push_back(from_bits(0xFFC00001u));  // a negative NaN with a payload
  return v;
}

static int fail(const char* what, float a, float b, float c) {
  fprintf(stderr, "guard_root_check: %s at (%a, %a, %a)\n", what, a, b, c);
  return 1;
}

int main(int argc, char** argv) {
  const bool print_triples = argc > 1 && !strcmp(argv[1], "triples");
  const std::vector<float> gv = guard_values();
  unsigned long triples = 0, new_ok_n = 0, old_ok_n = 0, refused_more = 0;
  for (float x : gv)
    for (float y : gv)
      for (float z : gv) {
        ++triples;
        const float d[3] = {x, y, z};
        const bool nk = fr::recip_box_ok3(fr::V3{x, y, z});
        const bool ok3 = old_ok(x) & old_ok(y) & old_ok(z);
        new_ok_n += nk;
        old_ok_n += ok3;
        refused_more += ok3 && !nk;
        if (nk && !ok3) return fail("new guard admits what the old one refused", x, y, z);
        for (int k = 0; k < 3; ++k) {
          const float fb = fr::box_inv_clamp(1.0f / d[k]);  // the fallback's value
          if ((isnan(d[k]) || isinf(d[k])) && nk) return fail("a NaN or infinite component admitted", x, y, z);
          if (old_ok(d[k])) {
            // the fast path's value is RN(1 / x) here; the clamp must be the identity on it
            if (bits(fb) != bits(1.0f / d[k])) return fail("fallback differs from RN(1/x) on the fast range", x, y, z);
            if (!(fabsf(fb) <= 0x1p100f)) return fail("reciprocal outside the clamp on the fast range", x, y, z);
          }
          if (isnan(fb) || fabsf(fb) > 0x1p100f) return fail("clamped reciprocal not in [-2^100, 2^100]", x, y, z);
        }
        if (print_triples)
          printf("%08x %08x %08x %08x %08x %08x\n", bits(x), bits(y), bits(z), bits(fr::box_inv_clamp(1.0f / x)),
                 bits(fr::box_inv_clamp(1.0f / y)), bits(fr::box_inv_clamp(1.0f / z)));
      }
  if (!refused_more) return fail("no triple reaches the conservative side", 0, 0, 0);

  const float t_min = 0.001f;
  const float rv[] = {NAN,  INFINITY,   -INFINITY, 0.0f, -0.0f, t_min, up(t_min), down(t_min),
                      1.0f, up(1.0f), 2.0f,      -1.0f};
  unsigned long roots = 0, hits = 0, max_form_differs = 0, max_form_differs_other = 0;
  for (float tn : rv)
    for (float tf : rv)
      for (float tm : rv) {
        ++roots;
        fr::Slab s{};
        s.tn = tn;
        s.tf = tf;
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
        const bool h0 = old_root(tn, tf, t_min, tm, t0);
        const bool h1 = fr::slab_root(s, t_min, tm, t1);
        const bool h2 = max_root(tn, tf, t_min, tm, t2);
        hits += h0;
        if (h0 != h1 || (h0 && bits(t0) != bits(t1))) return fail("slab_root differs from its reference", tn, tf, tm);
        if (h0 != h2 || (h0 && bits(t0) != bits(t2))) {
          ++max_form_differs;
          if (!(isnan(tn) && !isnan(tf))) ++max_form_differs_other;
        }
      }
  if (max_form_differs_other) return fail("the max form differs outside tn = NaN", 0, 0, 0);
  if (!print_triples)
    printf("{\"triples\": %lu, \"new_ok\": %lu, \"old_ok\": %lu, \"refused_more\": %lu, \"roots\": %lu, \"hits\": %lu, "
           "\"max_form_differs\": %lu}\n",
           triples, new_ok_n, old_ok_n, refused_more, roots, hits, max_form_differs);
  return 0;
}
