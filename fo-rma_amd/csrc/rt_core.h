// rt_core.h — f32 arithmetic of fo-rma's tracer hot path, shared by the gfx950
// kernel and the host-side camera setup of libforma_rt.
//
// Every expression keeps the reference's IEEE-f32 operation order, because path
// tracing is chaotic: one ulp in a hit distance or a rejection test changes the
// whole path. Build rules (enforced in the Makefile): -ffp-contract=off, no
// fast-math, correctly rounded '/' and sqrt on the device, no denormal flush.
//
// Reference mapping (paths relative to the reference root):
//   V3 ops ............ cpu_ray_tracer/primitives.rs:50-150 (dot :58-60, cross :62-68,
//                       unit_vector :70-72)
//   reflect/refract/schlick ... cpu_ray_tracer/utility.rs:27-54
//   random_in_unit_{circle,sphere} ... utility.rs:4-25 (rejection loops)
//   Rng ............... replaces rand::thread_rng() (rand 0.9.2, Cargo.lock:2735) with a
//                       counter-keyed xoshiro128+ stream per (seed, pixel, 16-sample block)
//   sphere_root ....... shapes/sphere.rs:23-51
//   plane_test ........ shapes/plane.rs:24-44 (stale-record quirk kept)
//   slab3/slab_root ... build-defined box, shaped like Sphere::hit
//   scatter_* ......... shapes/sphere.rs:84-152, shapes/plane.rs:101-122
//   sky ............... cpu_ray_tracer/tracer.rs:211-218
#pragma once
#include <stdint.h>

#if defined(__HIPCC_RTC__)
#define FR_HD __host__ __device__ __forceinline__  // hiprtc (trace_kernel.h's run-time build)
#elif defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define FR_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define FR_HD static inline
#endif

namespace fr {

struct V3 {
  float x, y, z;
};

FR_HD V3 mk(float x, float y, float z) { return V3{x, y, z}; }
FR_HD V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
FR_HD V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
FR_HD V3 mul(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
// f32 * Vec3 (primitives.rs:128-138) and Vec3 * f32 (:116-126) are the same products.
FR_HD V3 scl(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
FR_HD V3 divs(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }
// primitives.rs:58-60 — left to right, no fused multiply-add
FR_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
FR_HD V3 cross(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x};
}
FR_HD float length(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
FR_HD V3 unit(V3 a) { return divs(a, length(a)); }  // 3 divides, no reciprocal

// utility.rs:27-30: v - 2*dot(v,n)*n, evaluated as v - ((2*dot) * n)
FR_HD V3 reflect(V3 v, V3 n) { return sub(v, scl(2.0f * dot(v, n), n)); }

// utility.rs:49-54; powi(x,5) is lowered by LLVM's ExpandPowI (and compiler-rt's
// __powisf2) to x * ((x*x)*(x*x)); frozen here.
FR_HD float schlick(float cosine, float ref_idx) {
  float r0 = (1.0f - ref_idx) / (1.0f + ref_idx);
  r0 = r0 * r0;
  float x = 1.0f - cosine;
  float x2 = x * x;
  float x4 = x2 * x2;
  return r0 + (1.0f - r0) * (x * x4);
}

// ---------------------------------------------------------------------------
// RNG. One stream per (seed, pixel, key): key b for block b of 16 samples, and, when
// spp > 16, 2^31 | s / 4 for the 4-sample sub-blocks of the pixel's last block
// (trace_kernel.h stream_key). splitmix64 keys a xoshiro128+ 1.0 state (Blackman & Vigna's
// generator for floating-point output: only the upper bits are used); a stream's
// samples draw from it in sample order (the reference's save_image draws every sample
// from one sequential stream, tracer.rs:164-175). f32 = ((u32 ^ 2^31) >> 8) * 2^-24.
// ---------------------------------------------------------------------------
struct Rng {
  uint32_t s0, s1, s2, s3;
};

FR_HD uint64_t splitmix64_next(uint64_t& x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

FR_HD Rng rng_seed(uint64_t seed, uint32_t pixel, uint32_t block) {
  uint64_t x = seed ^ ((static_cast<uint64_t>(pixel) << 32) | static_cast<uint64_t>(block));
  uint64_t a = splitmix64_next(x);
  uint64_t b = splitmix64_next(x);
  return Rng{static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(b),
             static_cast<uint32_t>(b >> 32)};
}

FR_HD uint32_t rotl32(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

FR_HD uint32_t rng_next(Rng& r) {  // xoshiro128+ 1.0
  uint32_t result = r.s0 + r.s3;
  const uint32_t t = r.s1 << 9;
#if defined(__HIP_DEVICE_COMPILE__)
  // The draw is formed before the state moves on: it and the two words it read pass through one
  // empty asm, so the transition below cannot be scheduled ahead of the sum. Left free, the
  // compiler formed s0' and s3' early into fresh registers, kept the old words for a late sum,
  // and copied the new ones back at the next join (two v_mov_b32 per try of the lane loop).
  asm("" : "+v"(result), "+v"(r.s0), "+v"(r.s3));
  // the same state transition with gfx950's three-input v_bitop3_b32 (0x96 = a ^ b ^ c):
  // s2' = s2 ^ s0 ^ t, s1' = s1 ^ (s2 ^ s0), s0' = s0 ^ (s3 ^ s1), s3' = rotl(s3 ^ s1, 11);
  // 6 VALU per draw instead of 7 (LLVM does not form bitop3 from xor chains); C3 trace
  // 18.50 -> 18.15 ms, bit-identical to the plain sequence (the host's, below)
  const uint32_t s3x = r.s3 ^ r.s1;
  const uint32_t s1n = __builtin_amdgcn_bitop3_b32(r.s1, r.s2, r.s0, 0x96);
  const uint32_t s2n = __builtin_amdgcn_bitop3_b32(r.s2, r.s0, t, 0x96);
  r.s0 ^= s3x;
  r.s1 = s1n;
  r.s2 = s2n;
  r.s3 = rotl32(s3x, 11);
#else
  r.s2 ^= r.s0;
  r.s3 ^= r.s1;
  r.s1 ^= r.s2;
  r.s0 ^= r.s3;
  r.s2 ^= t;
  r.s3 = rotl32(r.s3, 11);
#endif
  return result;
}

// f32 in [0, 1): k = (u ^ 2^31) >> 8, r = k * 2^-24 (exact)
FR_HD float rng_f32(Rng& r) {
  return static_cast<float>((rng_next(r) ^ 0x80000000u) >> 8) * 5.9604644775390625e-08f;
}
// 2^24 rng_f32(r): the integer before the scale, as an f32 (exact)
FR_HD float rng_f32_scaled(Rng& r) { return static_cast<float>((rng_next(r) ^ 0x80000000u) >> 8); }

// 2*r - 1 for that r: (k - 2^23) * 2^-23 is exact in f32 and equals the arithmetic
// shift (int32)u >> 8 scaled by 2^-23, so shift + convert + scale replace the
// reference's 2*r - 1 bit for bit.
FR_HD float rng_signed_unit(Rng& r) {
  return static_cast<float>(static_cast<int32_t>(rng_next(r)) >> 8) * 1.1920928955078125e-07f;
}

// The same value scaled by 2^23: the integer (int32)u >> 8 as an f32 (exact). A
// rejection test on these, dot(k, k) >= 2^46, takes the same decision as dot(p, p) >= 1
// on p = k * 2^-23: every product and sum is the unscaled one times 2^46 exactly (f32
// rounding commutes with power-of-two scaling away from the denormal and overflow
// ranges, and 1 <= k*k <= 2^46 or k = 0). The accepted point is scaled once.
FR_HD float rng_signed_unit_scaled(Rng& r) { return static_cast<float>(static_cast<int32_t>(rng_next(r)) >> 8); }
constexpr float kSignedUnitScale = 1.1920928955078125e-07f;  // 2^-23
constexpr float kUnitBallScaled = 70368744177664.0f;         // 2^46

// utility.rs:4-13: p = 2*(r1, r2, 0) - (1, 1, 0), retry while dot(p,p) >= 1
// (trip-count hooks: trace_kernel.h's FR_DIAG builds define FR_DIAG_TRY and the counters
// before this header; empty everywhere else)
#ifdef FR_DIAG_TRY
#define FR_LENS_TRY() FR_DIAG_TRY(g_fr_diag_lens)
#define FR_RUS_TRY() FR_DIAG_TRY(g_fr_diag_rus)
#else
#define FR_LENS_TRY()
#define FR_RUS_TRY()
#endif
FR_HD V3 random_in_unit_circle(Rng& r) {
  float px, py;
  do {
    FR_LENS_TRY();
    px = rng_signed_unit(r);
    py = rng_signed_unit(r);
    // dot(p,p) = (px*px + py*py) + 0*0; adding +0 to a sum of squares is exact
  } while (px * px + py * py >= 1.0f);
  return V3{px, py, 0.0f};
}

// utility.rs:15-25: p = 2*(r1, r2, r3) - (1, 1, 1), retry while dot(p,p) >= 1
FR_HD V3 random_in_unit_sphere(Rng& r) {
  float px, py, pz;
  do {
    FR_RUS_TRY();
    px = rng_signed_unit(r);
    py = rng_signed_unit(r);
    pz = rng_signed_unit(r);
  } while (px * px + py * py + pz * pz >= 1.0f);
  return V3{px, py, pz};
}

// ---------------------------------------------------------------------------
// Primitives. The closest-hit loop (tracer.rs:190-200) only needs each test's
// accepted t; the hit record's point and normal are formed once for the winner
// (DESIGN.md §4.2 shows this equals the reference's shared-record updates).
// ---------------------------------------------------------------------------

// shapes/sphere.rs:23-51 without the record writes; a = dot(d, d) (loop-invariant).
// Both roots are formed unconditionally (no side effects) and the near one wins.
// rr = RN(radius * radius), the product the test forms (the BVH's leaf records carry it in
// place of the radius, pack.cpp)
FR_HD bool sphere_root_rr(V3 c, float rr, V3 o, V3 d, float a, float t_min, float t_max, float& t) {
  const V3 oc = sub(o, c);
  const float b = dot(oc, d);
  const float cc = dot(oc, oc) - rr;
  const float disc = b * b - a * cc;
  if (disc > 0.0f) {
    const float sq = sqrtf(disc);
    const float r1 = (-b - sq) / a;
    const float r2 = (-b + sq) / a;
    const bool c1 = r1 > t_min && r1 < t_max;
    const bool c2 = r2 > t_min && r2 < t_max;
    t = c1 ? r1 : r2;
    return c1 || c2;
  }
  return false;
}
FR_HD bool sphere_root(V3 c, float radius, V3 o, V3 d, float a, float t_min, float t_max, float& t) {
  return sphere_root_rr(c, radius * radius, o, d, a, t_min, t_max, t);
}

// shapes/plane.rs:24-44. denom is compared against the t-range; when it passes,
// the record's t (and p = point_at(t)) are written before the bounds test, so a
// failed test leaves them stale (returns 1); t may be negative. Returns 2 on a hit.
FR_HD int plane_test(V3 pos, V3 orient, V3 size, V3 o, V3 d, float t_min, float t_max, float& t) {
  const float denom = dot(orient, d);
  if (denom > t_min && denom < t_max) {
    t = dot(sub(pos, o), orient) / denom;
    const V3 p = add(o, scl(t, d));
    const bool in = p.x > pos.x - size.x && p.x < pos.x + size.x && p.y > pos.y - size.y &&
                    p.y < pos.y + size.y && p.z > pos.z - size.z && p.z < pos.z + size.z;
    return in ? 2 : 1;
  }
  return 0;
}

// Build-defined box. Per axis k, with inv_k = 1/d_k:
//   t0_k = (lo_k - o_k) * inv_k,  t1_k = (hi_k - o_k) * inv_k
//   near_k = minNum(t0_k, t1_k),  far_k = maxNum(t0_k, t1_k)   (IEEE 754-2008, NaN-ignoring)
//   tn = maxNum(maxNum(near_x, near_y), near_z),  tf = minNum(minNum(far_x, far_y), far_z)
// Hit iff tn < tf and one root lies in (t_min, t_max); the near root wins (Sphere::hit's
// two-root shape). The normal is the outward face normal of the first axis (x, y, z order)
// whose near (far) value equals tn (tf): -sign(d_k) on entry, +sign(d_k) on exit,
// with sign(0) counted negative. Zero signs never matter (t is only compared, never 0
// when accepted), so the hardware min/max agree with the host's fminf/fmaxf.
// v_min_f32 / v_max_f32 / v_min3_f32 directly: the generic lowering of fminf/fmaxf
// re-canonicalises operands it cannot prove canonical (every result of an asm statement),
// one v_max_f32 x, x, x per shared slab value in the scene kernel's list walk
FR_HD float fmin_num(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return fminf(a, b);
#endif
}
FR_HD float fmax_num(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return fmaxf(a, b);
#endif
}
// minNum(minNum(a, b), c) in one v_min3_f32 (device-checked against the chained v_min_f32
// and the host's fminf chain: test_device_max3_and_min3_match_fmaxf_fminf)
FR_HD float fmin3_num(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return fminf(fminf(a, b), c);
#endif
}

#if defined(__HIP__)
// v_rcp_f32 (1 ulp) refined by one FMA Newton step: r' = r + r (1 - x r). Equal to the
// correctly rounded 1.0f / x for every x whose exponent field is in [kRecipExpLo,
// kRecipExpHi] (exhaustively checked on the device: fr_selftest_recip,
// tests/test_gpu_parity.py::test_recip_nr_exhaustive); callers take 1.0f / x elsewhere.
__device__ __forceinline__ float recip_nr(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float r = __builtin_amdgcn_rcpf(x);
  const float e = __builtin_fmaf(-x, r, 1.0f);
  return __builtin_fmaf(e, r, r);
#else
  return 1.0f / x;  // not used on the host
#endif
}

// Reciprocal as the parity contract needs it (correctly rounded): recip_nr inside its
// exhaustively checked range, the full IEEE division otherwise (zero, denormals,
// |x| >= 2^126, inf, NaN). The fallback is a real branch, skipped by waves with no such lane.
__device__ __forceinline__ bool recip_nr_ok(float x) {
  const float ax = __builtin_fabsf(x);
  return (ax >= 0x1p-126f) & (ax < 0x1p126f);
}

// a / b correctly rounded, given y = RN(1 / b): q0 = a y and one FMA residual correction
// q0 + (a - b q0) y (Markstein's step; the compiler's IEEE sequence takes two, as its y is
// v_rcp_f32's 1-ulp estimate). Its v_div_scale / v_div_fmas / v_div_fixup steps are
// identities when a = +0 or |a| in [2^-100, 2^100] and |b| in [2^-100, 2^100] (no operand,
// quotient or residual near the denormal / overflow range), and there every operand pair
// scales to one in [1, 2) x [1, 2) by powers of two that scale both results exactly: all
// 2^46 such pairs are checked on the device (fr_selftest_div,
// tests/test_gpu_parity.py::test_div_rn_exhaustive). Used only where the operand ranges
// hold by construction.
__device__ __forceinline__ float div_rn(float a, float b, float y) {
  const float q0 = a * y;
  return __builtin_fmaf(__builtin_fmaf(-b, q0, a), y, q0);
}
#endif

#if defined(__HIP__)
// Correctly rounded sqrt(x) for x in [2^-96, 2^126]: v_sqrt_f32 and the compiler's two
// FMA residual corrections, without its denormal scaling and class fix-up (identities in
// that range; the same core as sky_t_fast, fr_selftest_ops op 14).
__device__ __forceinline__ float sqrt_core(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sdn = __uint_as_float(__float_as_uint(s) - 1u);
  const float sup = __uint_as_float(__float_as_uint(s) + 1u);
  const float rdn = __builtin_fmaf(-sdn, s, x);
  const float rup = __builtin_fmaf(-sup, s, x);
  float r = rdn <= 0.0f ? sdn : s;
  return rup > 0.0f ? sup : r;
#else
  return sqrtf(x);  // not used on the host
#endif
}

// The segment's part of sphere_root_fast: ya = RN(1 / a) and whether a = dot(d, d) is in
// [2^-60, 2^60] (recip_nr is exact there).
struct SphereSeg {
  float ya;
  bool ok;
};
__device__ __forceinline__ SphereSeg sphere_seg(float a) {
  return SphereSeg{recip_nr(a), (a >= 0x1p-60f) && (a <= 0x1p60f)};
}

// sphere_root bit for bit, with the root's sqrt and its two divisions by a done by their
// core sequences (sqrt_core, div_rn with the segment's ya) on lanes where disc is in
// [2^-96, 2^126], |b| <= 2^40 and a in [2^-60, 2^60]; other lanes take sphere_root's
// expressions. There |-b -+ sq| <= 2^41 and a root that can be accepted (> t_min = 0.001)
// has |numerator| >= 0.001 a >= 2^-70, so the numerator, the quotient (<= 2^101) and
// every intermediate are normal and div_rn is the correctly rounded quotient; a root below
// 0.001 in magnitude is below it by either sequence (a numerator under 2^-70 gives
// |q| < 2^-10 with an absolute error far below the gap), so both reject it. Checked against
// sphere_root on the device by fr_selftest_ops op 16 (tests/test_gpu_parity.py).
// (split in two so that a caller can mark the root step as its own region: the BVH leaf
// test, tools/isa_sections.py)
struct SphereDisc {
  float b, disc;
};
__device__ __forceinline__ SphereDisc sphere_disc_rr(V3 c, float rr, V3 o, V3 d, float a) {
  const V3 oc = sub(o, c);
  const float b = dot(oc, d);
  const float cc = dot(oc, oc) - rr;
  return SphereDisc{b, b * b - a * cc};
}
__device__ __forceinline__ SphereDisc sphere_disc(V3 c, float radius, V3 o, V3 d, float a) {
  return sphere_disc_rr(c, radius * radius, o, d, a);
}
// the roots of a sphere test whose discriminant is > 0
__device__ __forceinline__ bool sphere_roots_fast(SphereDisc q, float a, SphereSeg sg, float t_min, float t_max,
                                                  float& t) {
  const float b = q.b, disc = q.disc;
  {
    float r1, r2;
    const bool fast = static_cast<int>(sg.ok) & static_cast<int>(disc >= 0x1p-96f) & static_cast<int>(disc <= 0x1p126f) &
                      static_cast<int>(__builtin_fabsf(b) <= 0x1p40f);
    if (fast) {
      const float sq = sqrt_core(disc);
      r1 = div_rn(-b - sq, a, sg.ya);
      r2 = div_rn(-b + sq, a, sg.ya);
    } else {
      const float sq = sqrtf(disc);
      r1 = (-b - sq) / a;
      r2 = (-b + sq) / a;
    }
    const bool c1 = r1 > t_min && r1 < t_max;
    const bool c2 = r2 > t_min && r2 < t_max;
    t = c1 ? r1 : r2;
    return c1 || c2;
  }
}
__device__ __forceinline__ bool sphere_root_fast(V3 c, float radius, V3 o, V3 d, float a, SphereSeg sg,
                                                 float t_min, float t_max, float& t) {
  const SphereDisc q = sphere_disc(c, radius, o, d, a);
  if (q.disc > 0.0f) return sphere_roots_fast(q, a, sg, t_min, t_max, t);
  return false;
}
#endif

// maxNum(maxNum(a, b), c) in one v_max3_f32 (same IEEE-mode NaN rule as the chained
// v_max_f32; device-checked against fmaxf chains in test_device_max3_matches_fmaxf).
FR_HD float fmax3_num(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return fmaxf(fmaxf(a, b), c);
#endif
}

struct Slab {
  V3 t0, t1;  // slab distances per axis
  float tn, tf;
};

FR_HD Slab slab3(V3 lo, V3 hi, V3 o, V3 inv) {
  Slab s;
  // scalar f32 ops: packed v_pk_add/mul_f32 cost more issue time than two plain ops
  // (MI355X_MICROARCH.md, "vector-instruction ISSUE cost"; measured -2% here)
  s.t0 = V3{(lo.x - o.x) * inv.x, (lo.y - o.y) * inv.y, (lo.z - o.z) * inv.z};
  s.t1 = V3{(hi.x - o.x) * inv.x, (hi.y - o.y) * inv.y, (hi.z - o.z) * inv.z};
  s.tn = fmax3_num(fmin_num(s.t0.x, s.t1.x), fmin_num(s.t0.y, s.t1.y), fmin_num(s.t0.z, s.t1.z));
  s.tf = fmin3_num(fmax_num(s.t0.x, s.t1.x), fmax_num(s.t0.y, s.t1.y), fmax_num(s.t0.z, s.t1.z));
  return s;
}

// The same slab distances as fma(lo, inv, -o inv) with oinv = o inv precomputed: not
// the box primitive's exact arithmetic, only for the BVH's padded cull boxes (bvh.h).
// One slab distance fma(c, inv, -oinv). A plane at a compile-time 0 (the scene kernel's
// constants) is -oinv: 0 * inv is a zero for the finite (clamped) inv of the box test and the
// cull, so the two differ at most in the sign of a zero distance, which neither root
// selection (t > t_min) nor the face test (t equal to a distance) can see.
FR_HD float slab_d(float c, float inv, float oinv) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (__builtin_constant_p(c) && c == 0.0f) return -oinv;
#endif
  return fmaf(c, inv, -oinv);
}
// slab3_fused, per axis: the two slab distances t0, t1 and their near / far order.
//
// Symmetric pair. When lo and hi are compile-time constants (the scene kernel's records) with
// lo = -hi and 0 < hi <= kSlabSymMax, the distances are formed already sorted:
//   nr = fma(-hi, |inv|, -oinv),  fr = fma(hi, |inv|, -oinv)      (|inv| is a source modifier)
// and the v_min_f32 / v_max_f32 of the pair is not needed. {nr, fr} are the bits of {t0, t1}:
// for inv >= 0 they are the same operands, for inv < 0 the products (-hi)(-inv) and hi (-inv)
// are those of hi inv and lo inv exactly, sign included, so each fma has the operands of the
// other plane's. And nr <= fr whenever they are numbers, an fma being monotonic in its product.
//   - NaN: hi |inv| <= 2^27 2^100 is finite (kSlabSymMax and the clamp; an unbounded hi could
//     give fr = inf - inf beside a finite nr, which minNum / maxNum would both replace by nr), so
//     a distance is NaN only through oinv, which both share: both are NaN, as without the shortcut, and the
//     NaN-ignoring tn / tf see the same thing.
//   - inv = +-0 (d = +-inf): both products are zeros and both distances are -oinv, or zeros when
//     oinv is one; equal values have no order to get wrong.
//   - inv = +-2^100 (the clamp of a tiny or zero d): an ordinary finite inv, covered above.
//   - a zero distance (or two) may come out with the other sign than minNum / maxNum would pick:
//     §3.3 shows neither the root selection (t > t_min > 0) nor the face test (t == a
//     distance, +0 == -0) can see it.
// t0 / t1 hold nr / fr, the same two values: slab_normal's min / max of them are unchanged.
// Every other axis, every host build and every kernel whose records are loaded (is-constant
// is false there) takes the plain expressions.
constexpr float kSlabSymMax = 0x1p27f;
FR_HD bool slab_sym(float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_constant_p(lo) && __builtin_constant_p(hi) && lo == -hi && hi > 0.0f && hi <= kSlabSymMax;
#else
  (void)lo, (void)hi;
  return false;
#endif
}
// |inv| in a register of its own (device; one v_and per axis and segment, the statement being
// common to every use): with it each distance is an fma with a literal, where |inv| as a source
// modifier wants the literal in a scalar register, one s_mov per distinct coordinate
FR_HD float slab_abs_inv(float inv) {
  float a = __builtin_fabsf(inv);
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(a));
#endif
  return a;
}
// the distance of the plane at c (lo or hi) of an axis, and the axis's near / far distance
FR_HD float slab_pair_d(float lo, float hi, float c, float inv, float oinv) {
  return slab_sym(lo, hi) ? fmaf(c, slab_abs_inv(inv), -oinv) : slab_d(c, inv, oinv);
}
FR_HD float slab_near(float lo, float hi, float t0, float t1) { return slab_sym(lo, hi) ? t0 : fmin_num(t0, t1); }
FR_HD float slab_far(float lo, float hi, float t0, float t1) { return slab_sym(lo, hi) ? t1 : fmax_num(t0, t1); }
FR_HD Slab slab3_fused(V3 lo, V3 hi, V3 oinv, V3 inv) {
  Slab s;
  s.t0 = V3{slab_pair_d(lo.x, hi.x, lo.x, inv.x, oinv.x), slab_pair_d(lo.y, hi.y, lo.y, inv.y, oinv.y),
            slab_pair_d(lo.z, hi.z, lo.z, inv.z, oinv.z)};
  s.t1 = V3{slab_pair_d(lo.x, hi.x, hi.x, inv.x, oinv.x), slab_pair_d(lo.y, hi.y, hi.y, inv.y, oinv.y),
            slab_pair_d(lo.z, hi.z, hi.z, inv.z, oinv.z)};
  s.tn = fmax3_num(slab_near(lo.x, hi.x, s.t0.x, s.t1.x), slab_near(lo.y, hi.y, s.t0.y, s.t1.y),
                   slab_near(lo.z, hi.z, s.t0.z, s.t1.z));
  s.tf = fmin3_num(slab_far(lo.x, hi.x, s.t0.x, s.t1.x), slab_far(lo.y, hi.y, s.t0.y, s.t1.y),
                   slab_far(lo.z, hi.z, s.t0.z, s.t1.z));
  return s;
}

// The build-defined box's slab distances: fma(lo, inv, -(o inv))
// with inv = RN(1 / d) clamped to +-2^100, one rounding per distance instead of the two of
// (lo - o) * inv, and one instruction per distinct slab coordinate of the scene kernel (o inv
// is per segment): C3 14.84 -> 14.48 ms per streamed frame (profiles/r06e_ab_boxfma.log).
// The clamp keeps zero and tiny direction components finite (inf * lo - inf * o would be
// NaN). The oriented box keeps its own (lo - o) * inv form (slab3).
constexpr float kBoxInvClamp = 0x1p100f;
FR_HD float box_inv_clamp(float inv) { return fmin_num(fmax_num(inv, -kBoxInvClamp), kBoxInvClamp); }
// recip_nr's range narrowed to |x| >= 2^-100: there RN(1 / x) is within the clamp
FR_HD bool recip_box_ok(float x) {
  const float ax = __builtin_fabsf(x);
  return (ax >= 0x1p-100f) & (ax < 0x1p126f);
}
// The same guard for a segment's three components at once, conservative: ok only if
//   min3(|x|, |y|, |z|) >= 2^-100  and  (|x| + |y|) + |z| < 2^126
// (one v_min3_f32 and two adds with |.| source modifiers, two compares and one mask AND, for the
// six compares and five ANDs of three recip_box_ok).
//   - ok here => recip_box_ok of every component. A sum of non-negative terms rounds to no less
//     than its largest term (RN is monotonic), so a sum under 2^126 has every component under it;
//     a sum that overflows is +inf and fails. An infinite component makes the sum +inf; a NaN
//     component, which the NaN-ignoring min3 may skip, makes the sum NaN, and NaN < 2^126 is false.
//     That matters: the fallback turns a NaN reciprocal into -2^100 (box_inv_clamp's maxNum /
//     minNum), which recip_nr would not.
//   - It may refuse a segment whose components each pass (a sum at or over 2^126 of components
//     under it): that lane takes the IEEE division and the clamp, which equal the fast path
//     wherever both are valid: recip_nr is RN(1 / x) on its range, and |RN(1 / x)| <= 2^100 for
//     |x| >= 2^-100, where the clamp is the identity.
// (tests/c/guard_root_check.cpp goes through the triples at the thresholds; fr_selftest_boxinv
// returns the device's reciprocals for them.)
FR_HD float fmin3_abs(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_min3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return fminf(fminf(fabsf(a), fabsf(b)), fabsf(c));
#endif
}
FR_HD bool recip_box_ok3(V3 d) {
  const float sum = (__builtin_fabsf(d.x) + __builtin_fabsf(d.y)) + __builtin_fabsf(d.z);
  return (fmin3_abs(d.x, d.y, d.z) >= 0x1p-100f) & (sum < 0x1p126f);
}
#if defined(__HIP__)
// A segment's box reciprocals, RN(1 / d) clamped to +-2^100 per component: recip_nr under the
// guard, the IEEE division and the clamp on the lanes it refuses (a real branch, skipped by
// waves without such a lane)
__device__ __forceinline__ V3 seg_box_inv(V3 d) {
  V3 inv{recip_nr(d.x), recip_nr(d.y), recip_nr(d.z)};
  if (!recip_box_ok3(d)) {
    inv = V3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    inv = V3{box_inv_clamp(inv.x), box_inv_clamp(inv.y), box_inv_clamp(inv.z)};
  }
  return inv;
}
#endif
FR_HD Slab slab3_box(V3 lo, V3 hi, V3 o, V3 inv, V3 oinv) {
  (void)o;  // (slab3's signature; o enters through oinv)
  return slab3_fused(lo, hi, oinv, inv);
}

// Root selection: returns true and the accepted t if the box is hit in (t_min, t_max).
// Equivalent branch-free form of "near root if tn in (t_min, t_max), else far root if
// tf in (t_min, t_max), and tn < tf": when tn > t_min the far root can only be taken
// if tn >= t_max, and then tf > tn >= t_max fails too.
FR_HD bool slab_root(const Slab& s, float t_min, float t_max, float& t) {
  t = s.tn > t_min ? s.tn : s.tf;
  return (t > t_min) & (t < t_max) & (s.tn < s.tf);
}

FR_HD float comp(V3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

// Mirrored box pair. Two boxes that are adjacent in the list, share their
// slabs on two axes bit for bit and on the third axis AX are each other's reflection about 0:
// one at [-h2, -h1], the other at [h1, h2], 0 <= h1 < h2 <= kSlabSymMax (they may touch at 0).
// The scene kernel knows this at compile time (slab_mirror_axis over its constant records).
//
// The four plane distances of the axis are, as a set, the same for either sign of inv:
//   D1 = fma(-h2, |inv|, -oinv)  D2 = fma(-h1, |inv|, -oinv)  D3 = fma(h1, |inv|, -oinv)  D4 = fma(h2, |inv|, -oinv)
// (c inv for inv < 0 has the operands of (-c) |inv|, sign included, as for the symmetric slab
// above), and D1 <= D2 <= D3 <= D4 because an fma is monotonic in its product. The box the ray
// meets first, A, has (near, far) = (D1, D2) on the axis and the other, B, has (D3, D4): the
// bits that the min / max of each box's two distances give, without the four min / max. A is
// the box on the negative side when inv's sign bit is clear, else the one on the positive side.
//
// One candidate for the two. With g = "t > t_min and tn < tf" of slab_root, without t < t_max:
//   t_A <= tf_A <= D2 <= D3 <= tn_B <= t_B     when g_A and g_B
// (a root is tn or tf and tn < tf; min3 / max3 return no more / no less than an argument that
// is a number). So in list order, whichever of the two comes first:
//   - g_A and t_A < t_max: A is accepted. B is accepted before or after it only with
//     t_B < t_A, which cannot be, or, when B is first in the list, replaced by A only if
//     t_A < t_B strictly. The winner is A, except that equal roots leave the list's first box.
//   - g_A and not t_A < t_max: B fails too, t_B >= t_A.
//   - not g_A: B alone.
// Hence t = g_A ? t_A : t_B, hit = (g_A or g_B) and t < t_max, and the winner is the list's
// second box iff (A is second and g_A and not (g_B and t_A == t_B)) or (A is first and not
// g_A); the code forms the complement, "the first box wins", without complementing a mask. Equal
// accepted roots are above t_min, not zeros: the same bits.
//
// When the four D are not all numbers:
//   - h2 |inv| <= 2^27 2^100 is finite, so a D is NaN only through oinv, which all four share:
//     all NaN, as both boxes' distances are in list order. Then both boxes have the same tn and
//     tf from the other axes (the NaN-ignoring max3 / min3 skip the axis in both forms), t_A and
//     t_B are the same bits and g_A = g_B: the tie rule leaves the first box, as the strict
//     t < closest of the second test does.
//   - oinv = +-inf: the four D are that infinity, equal numbers.
//   - inv = +-0 (d = +-inf): the products are zeros and the four D are -oinv. For numbers
//     tn_A >= D1 = D2 >= tf_A, so neither box has tn < tf, in either form.
//   - a zero distance may carry the other sign than minNum / maxNum would pick; neither the
//     root selection nor the face test sees it (as for the symmetric slab).
// The plane at h1 = 0 goes through slab_d like any plane at 0. h1 = h2 (a flat box) is excluded.
template <int AX>
FR_HD bool slab_pair_root(V3 lo, V3 hi, V3 oinv, V3 inv, float t_min, float t_max, float& t, bool& first) {
  // lo, hi: the list's first box, the second one is its mirror image on AX; first: the winner
  // is the list's first box
  const float cl = comp(lo, AX), ch = comp(hi, AX);
  const bool first_low = ch <= 0.0f;  // the first box is the one on the negative side
  const float h1 = first_low ? -ch : cl, h2 = first_low ? -cl : ch;
  const float ai = slab_abs_inv(comp(inv, AX)), noi = -comp(oinv, AX);
  const float d1 = fmaf(-h2, ai, noi), d4 = fmaf(h2, ai, noi);
  const float d2 = h1 == 0.0f ? slab_d(0.0f, comp(inv, AX), comp(oinv, AX)) : fmaf(-h1, ai, noi);
  const float d3 = h1 == 0.0f ? d2 : fmaf(h1, ai, noi);
  // the two shared axes as slab3_fused forms them; AX's entries are replaced below
  const float x0 = slab_pair_d(lo.x, hi.x, lo.x, inv.x, oinv.x), x1 = slab_pair_d(lo.x, hi.x, hi.x, inv.x, oinv.x);
  const float y0 = slab_pair_d(lo.y, hi.y, lo.y, inv.y, oinv.y), y1 = slab_pair_d(lo.y, hi.y, hi.y, inv.y, oinv.y);
  const float z0 = slab_pair_d(lo.z, hi.z, lo.z, inv.z, oinv.z), z1 = slab_pair_d(lo.z, hi.z, hi.z, inv.z, oinv.z);
  const float nx = AX == 0 ? 0.0f : slab_near(lo.x, hi.x, x0, x1), fx = AX == 0 ? 0.0f : slab_far(lo.x, hi.x, x0, x1);
  const float ny = AX == 1 ? 0.0f : slab_near(lo.y, hi.y, y0, y1), fy = AX == 1 ? 0.0f : slab_far(lo.y, hi.y, y0, y1);
  const float nz = AX == 2 ? 0.0f : slab_near(lo.z, hi.z, z0, z1), fz = AX == 2 ? 0.0f : slab_far(lo.z, hi.z, z0, z1);
  const float tn_a = fmax3_num(AX == 0 ? d1 : nx, AX == 1 ? d1 : ny, AX == 2 ? d1 : nz);
  const float tf_a = fmin3_num(AX == 0 ? d2 : fx, AX == 1 ? d2 : fy, AX == 2 ? d2 : fz);
  const float tn_b = fmax3_num(AX == 0 ? d3 : nx, AX == 1 ? d3 : ny, AX == 2 ? d3 : nz);
  const float tf_b = fmin3_num(AX == 0 ? d4 : fx, AX == 1 ? d4 : fy, AX == 2 ? d4 : fz);
  const float t_a = tn_a > t_min ? tn_a : tf_a, t_b = tn_b > t_min ? tn_b : tf_b;
  const bool g_a = (t_a > t_min) & (tn_a < tf_a), g_b = (t_b > t_min) & (tn_b < tf_b);
  // A is the list's second box: the ray goes down (sign bit of inv) and the first box is the
  // lower one, or up and the first is the upper one. One sign compare, and no complement of a
  // mask: with T = g_b and t_a == t_b, A is used iff g_a and not (sec and T), and the winner is
  // the list's first box iff (A is used) != sec, that is g_a != sec != (g_a and sec and T).
  const int ib = __builtin_bit_cast(int, comp(inv, AX));
  const bool sec = first_low ? ib < 0 : ib >= 0;
  const bool tie = g_b & (t_a == t_b);
  t = g_a ? t_a : t_b;
  first = (g_a != sec) != ((g_a & sec) & tie);
  return (g_a | g_b) & (t < t_max);
}
// The axis on which box j is box i's mirror image in the sense above, or -1: for
// compile-time records (a constant expression).
constexpr bool slab_same_bits(float a, float b) {
  return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b);
}
constexpr bool slab_mirrored(float lo_i, float hi_i, float lo_j, float hi_j) {
  // i below j or j below i; bounds as numbers (a NaN fails every comparison)
  return lo_j == -hi_i && hi_j == -lo_i && lo_i < hi_i &&
         ((hi_i <= 0.0f && -lo_i <= kSlabSymMax) || (lo_i >= 0.0f && hi_i <= kSlabSymMax));
}
constexpr int slab_mirror_axis(const float (&lo_i)[3], const float (&hi_i)[3], const float (&lo_j)[3],
                               const float (&hi_j)[3]) {
  int axis = -1, same = 0;
  for (int k = 0; k < 3; ++k) {
    if (slab_same_bits(lo_i[k], lo_j[k]) && slab_same_bits(hi_i[k], hi_j[k]))
      ++same;
    else if (slab_mirrored(lo_i[k], hi_i[k], lo_j[k], hi_j[k]))
      axis = k;
  }
  return same == 2 ? axis : -1;
}

FR_HD V3 axis_normal(int k, float s) {
  return V3{k == 0 ? s : 0.0f, k == 1 ? s : 0.0f, k == 2 ? s : 0.0f};
}

// Outward normal of the accepted root t (t == tn: entry face, else exit face), in the
// frame whose ray direction is dd.
FR_HD V3 slab_normal(const Slab& s, float t, V3 dd) {
#if defined(__HIP_DEVICE_COMPILE__)
  // Branch-free form of the two cases below, for t == tn or t == tf (slab_root's roots;
  // the caller recomputes the winner's slab with the same operations): entry iff t == tn;
  // the first axis whose near (entry) or far (exit) distance equals t; the sign is
  // -sign(d_k) on entry and +sign(d_k) on exit, sign(0) counted negative. Selects on lane
  // masks instead of a divergent branch in which both cases ran for a mixed wave.
  // (both per-axis extremes formed up front: a conditional asm min/max became a branch)
  const bool entry = t == s.tn;
  const float mnx = fmin_num(s.t0.x, s.t1.x), mxx = fmax_num(s.t0.x, s.t1.x);
  const float mny = fmin_num(s.t0.y, s.t1.y), mxy = fmax_num(s.t0.y, s.t1.y);
  const bool kx = (entry ? mnx : mxx) == t;
  const bool ky = !kx && (entry ? mny : mxy) == t;
  const bool kz = !kx && !ky;
  const float dk = kx ? dd.x : (ky ? dd.y : dd.z);
  const float sg = ((dk > 0.0f) != entry) ? 1.0f : -1.0f;
  return V3{kx ? sg : 0.0f, ky ? sg : 0.0f, kz ? sg : 0.0f};
#else
  if (t == s.tn) {
    const int k = fmin_num(s.t0.x, s.t1.x) == s.tn ? 0 : (fmin_num(s.t0.y, s.t1.y) == s.tn ? 1 : 2);
    return axis_normal(k, comp(dd, k) > 0.0f ? -1.0f : 1.0f);
  }
  const int k = fmax_num(s.t0.x, s.t1.x) == s.tf ? 0 : (fmax_num(s.t0.y, s.t1.y) == s.tf ? 1 : 2);
  return axis_normal(k, comp(dd, k) > 0.0f ? 1.0f : -1.0f);
#endif
}

// Build-defined triangle: Moller-Trumbore in f32 with this order;
// e1 = v1 - v0, e2 = v2 - v0 come precomputed (same host f32 ops as the oracle's).
// NaN or infinite barycentrics (det = 0) fail the comparisons.
FR_HD bool tri_root(V3 v0, V3 e1, V3 e2, V3 o, V3 d, float t_min, float t_max, float& t) {
  const V3 pv = cross(d, e2);
  const float inv_det = 1.0f / dot(e1, pv);
  const V3 s = sub(o, v0);
  const float u = dot(s, pv) * inv_det;
  const V3 qv = cross(s, e1);
  const float v = dot(d, qv) * inv_det;
  t = dot(e2, qv) * inv_det;
  return (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f) & (t > t_min) & (t < t_max);
}

// Oriented box: the same slab test in the box frame (rows ax, ay, az of world->local).
struct ObbFrame {
  V3 dl, inv, ol;
};

FR_HD ObbFrame obb_frame(V3 c, V3 ax, V3 ay, V3 az, V3 o, V3 d) {
  ObbFrame f;
  const V3 oc = sub(o, c);
  f.ol = V3{dot(ax, oc), dot(ay, oc), dot(az, oc)};
  f.dl = V3{dot(ax, d), dot(ay, d), dot(az, d)};
  f.inv = V3{1.0f / f.dl.x, 1.0f / f.dl.y, 1.0f / f.dl.z};
  return f;
}

FR_HD V3 obb_normal(V3 ax, V3 ay, V3 az, const Slab& s, float t, V3 dl) {
  const V3 nl = slab_normal(s, t, dl);  // one component is +-1
  const float sg = nl.x + nl.y + nl.z;
  const V3 axis = nl.x != 0.0f ? ax : (nl.y != 0.0f ? ay : az);
  return scl(sg, axis);
}

// ---------------------------------------------------------------------------
// Scatter. Effective classes after the per-shape fallbacks (sphere.rs:56-69,
// plane.rs:48-59): boxes follow the sphere's material table.
// ---------------------------------------------------------------------------
enum ScatterClass : uint32_t { SC_LAMBERT = 0, SC_METAL = 1, SC_DIELECTRIC = 2, SC_LIGHT = 3, SC_NONE = 4 };

// sphere.rs:84-89 / 147-152, plane.rs:101-106: target = (p + n) + rus; dir = target - p
FR_HD V3 scatter_lambert(V3 p, V3 n, Rng& r) {
  const V3 target = add(add(p, n), random_in_unit_sphere(r));
  return sub(target, p);
}

// sphere.rs:91-105, plane.rs:108-122: rus is drawn even when fuzz = 0
FR_HD bool scatter_metal(V3 d, V3 p_unused, V3 n, float fuzz, Rng& r, V3& dir) {
  (void)p_unused;
  const V3 refl = reflect(unit(d), n);
  dir = add(refl, scl(fuzz, random_in_unit_sphere(r)));
  return dot(dir, n) > 0.0f;
}

// sphere.rs:107-145 (ref_idx 1.3; attenuation = colour, applied by the caller)
FR_HD V3 scatter_dielectric(V3 d, V3 n, Rng& r) {
  const float ref_idx = 1.3f;
  const V3 reflected = reflect(d, n);
  V3 outward;
  float ni, cosine;
  const float dn = dot(d, n);
  if (dn > 0.0f) {
    outward = sub(V3{0.0f, 0.0f, 0.0f}, n);
    ni = ref_idx;
    cosine = ref_idx * dot(d, n) / length(d);
  } else {
    outward = n;
    ni = 1.0f / ref_idx;
    cosine = -dot(d, n) / length(d);
  }
  // utility.rs:37-47
  const V3 uv = unit(d);
  const float dt = dot(uv, outward);
  const float disc = 1.0f - ni * ni * (1.0f - dt * dt);
  V3 refracted = V3{0.0f, 0.0f, 0.0f};
  float reflect_prob;
  if (disc > 0.0f) {
    refracted = sub(scl(ni, sub(uv, scl(dt, outward))), scl(sqrtf(disc), outward));
    reflect_prob = schlick(cosine, ref_idx);
  } else {
    reflect_prob = 1.0f;
  }
  return rng_f32(r) < reflect_prob ? reflected : refracted;
}

// tracer.rs:211-218
// split in two for the deferred unwind (render.hip): the blend parameter t, and the colour
FR_HD float sky_t(V3 d) {
  const V3 ud = unit(d);
  return 0.5f * (ud.y + 1.0f);
}
// sky_t from the two values it depends on, d.y and dot(d, d) in length()'s order: the same
// operations (a division by the correctly rounded sqrt, then the blend parameter)
FR_HD float sky_t_from(float dy, float dd) { return 0.5f * (dy / sqrtf(dd) + 1.0f); }
FR_HD V3 sky_from_t(float t) { return add(scl(1.0f - t, V3{1.0f, 1.0f, 1.0f}), scl(t, V3{0.5f, 0.7f, 1.0f})); }
FR_HD V3 sky(V3 d) { return sky_from_t(sky_t(d)); }

#if defined(__HIP__)
// sky_t (tracer.rs:211-218's blend parameter 0.5 (unit(d).y + 1)) with the correctly
// rounded sqrt and division done by their core sequences where the operands allow it:
// v_sqrt_f32 and the compiler's two FMA residual corrections without the denormal
// scaling and class fix-up (identities for dd in [2^-96, 2^126]); and d.y / len by
// div_rn(d.y, len, recip_nr(len)) (recip_nr exact for len's exponent range there, div_rn's
// steps identities for |d.y| in {0} u [2^-100, 2^63], and |d.y| <= len <= 2^63). A d.y
// below 2^-100 in magnitude needs no guard of its own: with len >= 2^-48 both sequences
// give |q| < 2^-50 (the core one's residual may be denormal there), and 1 + q = 1 either
// way. Other lanes take the plain expression. Bit-identical to sky_t: fr_selftest_ops op 14.
__device__ __forceinline__ float sky_t_fast_from(float dy, float dd) {
  const bool fast = (dd >= 0x1p-96f) & (dd <= 0x1p126f);
  if (fast) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float s = __builtin_amdgcn_sqrtf(dd);
    const float sdn = __uint_as_float(__float_as_uint(s) - 1u);
    const float sup = __uint_as_float(__float_as_uint(s) + 1u);
    const float rdn = __builtin_fmaf(-sdn, s, dd);
    const float rup = __builtin_fmaf(-sup, s, dd);
    float len = rdn <= 0.0f ? sdn : s;
    len = rup > 0.0f ? sup : len;
    const float q = div_rn(dy, len, recip_nr(len));
    return 0.5f * (q + 1.0f);
#endif
  }
  return sky_t_from(dy, dd);  // = sky_t(d): the same operations on the same values
}
__device__ __forceinline__ float sky_t_fast(V3 d) {
  return sky_t_fast_from(d.y, d.x * d.x + d.y * d.y + d.z * d.z);  // length()'s sum, in its order
}
#endif

// tracer.rs:182-184: Rust `as u8` saturates (NaN -> 0) and truncates toward zero.
FR_HD uint8_t to_u8(float c) {
  const float s = sqrtf(c) * 255.0f;
  if (!(s > 0.0f)) return 0;
  if (s >= 255.0f) return 255;
  return static_cast<uint8_t>(s);
}

// Rust `f32 as u8` of a value already in byte units: NaN -> 0, saturating, truncation
FR_HD uint8_t as_u8_trunc(float v) {
  if (!(v > 0.0f)) return 0;
  if (v >= 255.0f) return 255;
  return static_cast<uint8_t>(v);
}

}  // namespace fr
