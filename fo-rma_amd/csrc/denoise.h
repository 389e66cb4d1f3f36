// denoise.h — the variance-guided filter of a progressive accumulation (fr_ctx_denoise,
// DESIGN.md §4.5d): an a-trous wavelet filter (SVGF's spatial part) steered by the per-pixel
// variance of the mean that A, Q and the counts already give. Its f32 arithmetic, shared by the
// kernels (denoise.hip) and a CPU program (tests/c/denoise_check.cpp), and the launch. Every
// named operation rounds once in f32; the build rules of rt_core.h hold (no contraction, IEEE
// '/' and sqrt).
//
// The variance map that comes out is what the filter steered by: the variance of the mean,
// carried through the taps' weights as if the taps were independent and the weights fixed. It
// is NOT an error estimate of the filtered picture: the filter trades variance for bias, and on
// the oracle's frames the map read 23 to 46 times under the real squared error.
#pragma once
#include <stdint.h>
#include <string.h>

#include "accum_error.h"
#include "rt_core.h"

namespace fr {

constexpr float kDnEps = 0x1p-20f;     // FR_DN_EPS: keeps the edge-stopping scale above zero
constexpr float kDnMeanMax = 0x1p40f;  // FR_DN_MEAN_MAX: a valid pixel's |mean| per channel
constexpr float kDnVarMax = 0x1p80f;   // FR_DN_VAR_MAX: a valid pixel's variance of the mean
constexpr uint32_t kDnLevelsDefault = 4, kDnLevelsMax = 6;  // FR_DN_LEVELS_DEFAULT
constexpr float kDnKDefault = 4.0f, kDnKMax = 1024.0f;      // FR_DN_K_DEFAULT

// A pixel of the ping and pong buffers, 16 bytes: the colour and the variance of the mean.
// Validity is decided once, by dn_prep, and kept in var's sign bit: var is a sum of clamped
// variances over a positive count, so it is in [+0, +inf] and never NaN, and its sign bit is
// free. Set: the pixel is invalid, no tap reads it and every level copies it as it is;
// dn_var takes the bit off again.
struct DnPixel {
  float r, g, b, var;
};
constexpr uint32_t kDnInvalidBit = 0x80000000u;

FR_HD uint32_t dn_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
FR_HD float dn_float(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
FR_HD bool dn_valid(DnPixel p) { return (dn_bits(p.var) & kDnInvalidBit) == 0u; }
FR_HD float dn_var(DnPixel p) { return dn_float(dn_bits(p.var) & ~kDnInvalidBit); }

// Prep: C = (m_r, m_g, m_b) and var = ((v_r + v_g) + v_b) / fn of accum_var, fn = (float)n
// samples per pixel, fk = (float)(K - 1) for K >= 2 frames. Valid iff |m_c| <= kDnMeanMax in
// every channel and var <= kDnVarMax: a comparison with NaN is false, so a NaN or infinite
// pixel is invalid.
FR_HD DnPixel dn_prep(V3 a, V3 q, float fn, float fk) {
  DnPixel p;
  const float vr = accum_var(a.x, q.x, fn, fk, p.r);
  const float vg = accum_var(a.y, q.y, fn, fk, p.g);
  const float vb = accum_var(a.z, q.z, fn, fk, p.b);
  const float var = ((vr + vg) + vb) / fn;
  const bool ok = (__builtin_fabsf(p.r) <= kDnMeanMax) & (__builtin_fabsf(p.g) <= kDnMeanMax) &
                  (__builtin_fabsf(p.b) <= kDnMeanMax) & (var <= kDnVarMax);
  p.var = ok ? var : dn_float(dn_bits(var) | kDnInvalidBit);
  return p;
}

// The B3 spline (1/16, 1/4, 3/8, 1/4, 1/16) of tap d in -2..2 and the (1, 2, 1) of the 3x3
// variance prefilter; their products are exact in f32.
FR_HD float dn_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1 ? 0.25f : 0.0625f); }
FR_HD float dn_b(int d) { return d == 0 ? 2.0f : 1.0f; }

// One level at (x, y) of a W x H image with step s = 1 << level; fetch(x, y) returns the
// previous level's pixel for coordinates inside the image. An invalid pixel is returned as it
// is. For a valid one:
//   g     = sum(wt var_q) / sum(wt) over the valid 3x3 neighbours at distance 1, wt = b b
//   sden  = k g + kDnEps
//   per tap q = p + s (dx, dy), dy outer and dx inner, -2..2, inside the image and valid:
//     d2 = (d_r d_r + d_g d_g) + d_b d_b with d = C_q - C_p, wc = sden / (sden + d2),
//     w = (h h) wc, sumc += w C_q, sumv += (w w) var_q, sumw += w
//   C' = sumc / sumw, var' = sumv / (sumw sumw)
// The centre tap has d2 = 0, so wc = 1 exactly and sumw >= 9/64; with the two caps every
// intermediate is finite: nothing a valid pixel yields is NaN. A skipped tap (outside, or
// invalid) reads the centre pixel instead and is selected away, so the loads do not depend on
// one another.
template <class Fetch>
FR_HD DnPixel dn_level(const Fetch& fetch, int x, int y, int W, int H, int s, float k) {
  const DnPixel p = fetch(x, y);
  if (!dn_valid(p)) return p;
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      const bool in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H);
      const DnPixel q = fetch(in ? qx : x, in ? qy : y);
      const bool ok = in & dn_valid(q);
      const float wt = dn_b(dy) * dn_b(dx);
      gs = ok ? gs + wt * q.var : gs;
      gw = ok ? gw + wt : gw;
    }
  }
  const float g = gs / gw;
  const float sden = k * g + kDnEps;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sumv = 0.0f, sumw = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + s * dx, qy = y + s * dy;
      const bool in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H);
      const DnPixel q = fetch(in ? qx : x, in ? qy : y);
      const bool ok = in & dn_valid(q);
      const float dr = q.r - p.r, dg = q.g - p.g, db = q.b - p.b;
      const float d2 = (dr * dr + dg * dg) + db * db;
      const float wc = sden / (sden + d2);
      const float w = (dn_h(dy) * dn_h(dx)) * wc;
      sr = ok ? sr + w * q.r : sr;
      sg = ok ? sg + w * q.g : sg;
      sb = ok ? sb + w * q.b : sb;
      sumv = ok ? sumv + (w * w) * q.var : sumv;
      sumw = ok ? sumw + w : sumw;
    }
  }
  DnPixel o;
  o.r = sr / sumw;
  o.g = sg / sumw;
  o.b = sb / sumw;
  o.var = sumv / (sumw * sumw);
  return o;
}

// ---- the feature-guided filter (fr_ctx_denoise_guided) ----------------
// The same a-trous filter, each non-centre tap's weight extended by the first hit's features
// (fr_ctx_gbuffer: gbuffer.h), which carry no noise: the normal N, the point P, the root t and
// the primitive id of the pinhole primary ray, and the primitive's attenuation ("albedo").
constexpr float kDnFeatMax = 0x1p40f;    // FR_DN_FEAT_MAX: a valid hit pixel's t and |P_c|
constexpr float kDnNormalMax = 0x1p10f;  // FR_DN_NORMAL_MAX: a valid hit pixel's |N_c|
constexpr float kDnAlbMin = 0x1p-6f;     // FR_DN_ALB_MIN, FR_DN_ALB_MAX: an albedo component outside
constexpr float kDnAlbMax = 0x1p6f;      //   [min, max] (or NaN) demodulates as 1
constexpr float kDnSigmaZDefault = 0x1p-5f, kDnSigmaZMax = 1024.0f;      // FR_DN_SIGMA_Z_DEFAULT
constexpr uint32_t kDnNormalPow2Default = 4u, kDnNormalPow2Max = 8u;     // FR_DN_NORMAL_POW2_DEFAULT
constexpr uint32_t kDnMiss = 0xFFFFFFFFu;                                // gbuffer.h's kGbMiss

// A pixel's features: the two 16-byte words of the G-buffer, G0 = (N, t) and G1 = (P, bits(id)).
struct DnFeat {
  V3 n;
  float t;
  V3 p;
  uint32_t id;
};

FR_HD float dn_alb(float a) { return (a >= kDnAlbMin && a <= kDnAlbMax) ? a : 1.0f; }
FR_HD V3 dn_alb(V3 alb, bool demodulate) {
  return demodulate ? V3{dn_alb(alb.x), dn_alb(alb.y), dn_alb(alb.z)} : V3{1.0f, 1.0f, 1.0f};
}

// Guided prep: dn_prep's m, var and validity; a hit pixel is also invalid unless t <= kDnFeatMax,
// |P_c| <= kDnFeatMax and |N_c| <= kDnNormalMax in every component (comparisons with NaN are
// false). With demodulate, a_c = dn_alb(alb_c), C_c = m_c / a_c and
// var = ((v_r / (a_r a_r) + v_g / (a_g a_g)) + v_b / (a_b a_b)) / fn; without, the pixel is
// dn_prep's. v_c is in [+0, +inf] and a_c a_c in [2^-12, 2^12], so var is in [+0, +inf], never
// NaN, and its sign bit stays free for the validity.
FR_HD DnPixel dn_prep_guided(V3 a, V3 q, float fn, float fk, DnFeat f, V3 alb, bool demodulate) {
  DnPixel p = dn_prep(a, q, fn, fk);
  bool ok = dn_valid(p);
  if (demodulate) {
    const V3 al = dn_alb(alb, true);
    float m;
    const float vr = accum_var(a.x, q.x, fn, fk, m);
    const float vg = accum_var(a.y, q.y, fn, fk, m);
    const float vb = accum_var(a.z, q.z, fn, fk, m);
    p.r = p.r / al.x;
    p.g = p.g / al.y;
    p.b = p.b / al.z;
    p.var = ((vr / (al.x * al.x) + vg / (al.y * al.y)) + vb / (al.z * al.z)) / fn;
  } else {
    p.var = dn_var(p);
  }
  const bool feat_ok = (f.t <= kDnFeatMax) & (__builtin_fabsf(f.p.x) <= kDnFeatMax) &
                       (__builtin_fabsf(f.p.y) <= kDnFeatMax) & (__builtin_fabsf(f.p.z) <= kDnFeatMax) &
                       (__builtin_fabsf(f.n.x) <= kDnNormalMax) & (__builtin_fabsf(f.n.y) <= kDnNormalMax) &
                       (__builtin_fabsf(f.n.z) <= kDnNormalMax);
  ok = ok & ((f.id == kDnMiss) | feat_ok);
  p.var = ok ? p.var : dn_float(dn_bits(p.var) | kDnInvalidBit);
  return p;
}

// The last level's picture: mean_c = C'_c a_c with demodulate, C'_c without, for every pixel.
FR_HD V3 dn_remodulate(DnPixel o, V3 alb, bool demodulate) {
  if (!demodulate) return V3{o.r, o.g, o.b};
  const V3 al = dn_alb(alb, true);
  return V3{o.r * al.x, o.g * al.y, o.b * al.z};
}

// One guided level: dn_level's loops, order and variance prefilter; feat(x, y) returns the
// features of a pixel inside the image. A tap is also skipped unless it and the centre are both
// hits or both misses. For a non-centre tap between two hits:
//   c  = (N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z, c = c > 0 ? c : 0, wn = c squared normal_pow2 times
//   e  = (N_p.x D.x + N_p.y D.y) + N_p.z D.z with D = P_q - P_p: the tap's distance from the
//        centre's tangent plane
//   z  = sigma_z t_p, zden = z z + kDnEps, wz = zden / (zden + e e): that distance relative to the
//        depth, so a ground plane seen at a grazing angle is not under-filtered
//   w  = (((h h) wc) wn) wz
// Between two misses, and for the centre tap by definition, wn = wz = 1, so sumw >= 9/64 as in
// dn_level. Under the caps a valid pixel has |C_c| <= 2^46 and var < 2^93 (demodulated), so d2 <
// 2^96 and sden < 2^104 are finite; |D_c| <= 2^41 and |N_c| <= 2^10 give |e| < 2^53 and e e <
// 2^106; z <= 2^50, so zden is in [2^-20, 2^101] and wz in [0, 1], never NaN. c is at most
// 3 2^20; wn is finite whenever c^(2^normal_pow2) is, which holds for every c <= 1.25 at
// every normal_pow2 <= 8 (unit normals: c <= 1 up to rounding) and for every c under the cap at
// normal_pow2 <= 2. A pair of normals longer than that can overflow wn to +inf at a large
// normal_pow2, and a sum can then be inf or NaN: the caps bound the features, they do not make
// them unit vectors. Nothing else a valid pixel yields is NaN.
template <class Fetch, class FetchFeat>
FR_HD DnPixel dn_level_guided(const Fetch& fetch, const FetchFeat& feat, int x, int y, int W, int H, int s, float k,
                              float sigma_z, uint32_t normal_pow2) {
  const DnPixel p = fetch(x, y);
  if (!dn_valid(p)) return p;
  const DnFeat fp = feat(x, y);
  const bool miss_p = fp.id == kDnMiss;
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx, qy = y + dy;
      const bool in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H);
      const DnPixel q = fetch(in ? qx : x, in ? qy : y);
      const bool ok = in & dn_valid(q);
      const float wt = dn_b(dy) * dn_b(dx);
      gs = ok ? gs + wt * q.var : gs;
      gw = ok ? gw + wt : gw;
    }
  }
  const float g = gs / gw;
  const float sden = k * g + kDnEps;
  const float z = sigma_z * fp.t;
  const float zden = z * z + kDnEps;
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sumv = 0.0f, sumw = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + s * dx, qy = y + s * dy;
      const bool in = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H);
      const int fx = in ? qx : x, fy = in ? qy : y;
      const DnPixel q = fetch(fx, fy);
      const DnFeat fq = feat(fx, fy);
      const bool miss_q = fq.id == kDnMiss;
      const bool ok = in & dn_valid(q) & (miss_q == miss_p);
      const float dr = q.r - p.r, dg = q.g - p.g, db = q.b - p.b;
      const float d2 = (dr * dr + dg * dg) + db * db;
      const float wc = sden / (sden + d2);
      float wn = 1.0f, wz = 1.0f;
      if (dx != 0 || dy != 0) {  // (compile-time: the loops are unrolled)
        float c = (fp.n.x * fq.n.x + fp.n.y * fq.n.y) + fp.n.z * fq.n.z;
        c = c > 0.0f ? c : 0.0f;
        for (uint32_t j = 0; j < normal_pow2; ++j) c = c * c;
        const V3 dp = sub(fq.p, fp.p);
        const float e = (fp.n.x * dp.x + fp.n.y * dp.y) + fp.n.z * dp.z;
        const float wzh = zden / (zden + e * e);
        wn = miss_p ? 1.0f : c;
        wz = miss_p ? 1.0f : wzh;
      }
      const float w = (((dn_h(dy) * dn_h(dx)) * wc) * wn) * wz;
      sr = ok ? sr + w * q.r : sr;
      sg = ok ? sg + w * q.g : sg;
      sb = ok ? sb + w * q.b : sb;
      sumv = ok ? sumv + (w * w) * q.var : sumv;
      sumw = ok ? sumw + w : sumw;
    }
  }
  DnPixel o;
  o.r = sr / sumw;
  o.g = sg / sumw;
  o.b = sb / sumw;
  o.var = sumv / (sumw * sumw);
  return o;
}

}  // namespace fr

#if defined(__HIPCC__) || defined(__HIP__)
#include "kparams.h"

namespace fr {

constexpr uint32_t kDnTileW = 32, kDnTileH = 8;  // a level's workgroup: 32 x 8 pixels

// Enqueues prep and `levels` levels on `stream`: A and Q (3 f32 per pixel slot of kp's shard,
// which must be the whole image) with each tile's n_t and K_t, or with the uniform n and K
// when n_t is null, into ping; then ping -> pong -> ping ...; the last level also writes
// mean_rgb (W*H*3 f32), rgb8 (W*H*3 u8) and var (W*H f32). ping, pong: W*H DnPixel each.
hipError_t launch_denoise(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                          const uint32_t* n_t, const uint32_t* k_t, uint32_t n, uint32_t frames, uint32_t levels,
                          float k, DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8, float* var);

// The levels alone, on prep's pixels already in ping (fr_ctx_temporal writes its own): `levels`
// launches ping -> pong -> ping ..., the last one's outputs as launch_denoise's.
hipError_t launch_denoise_levels(hipStream_t stream, uint32_t width, uint32_t height, uint32_t levels, float k,
                                 DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8, float* var);

// The guided filter (fr_ctx_denoise_guided): launch_denoise's arguments, the features g0, g1
// and alb (W*H float4 each, fr_ctx_gbuffer's) and the guide. The last level's var is the
// demodulated-space variance the filter steered by.
struct DnGuide {
  float sigma_z;
  uint32_t normal_pow2, demodulate;
};
hipError_t launch_denoise_guided(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                                 const uint32_t* n_t, const uint32_t* k_t, uint32_t n, uint32_t frames,
                                 uint32_t levels, float k, const DnGuide& guide, const float4* g0, const float4* g1,
                                 const float4* alb, DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8,
                                 float* var);
hipError_t launch_denoise_guided_levels(hipStream_t stream, uint32_t width, uint32_t height, uint32_t levels, float k,
                                        const DnGuide& guide, const float4* g0, const float4* g1, const float4* alb,
                                        DnPixel* ping, DnPixel* pong, float* mean_rgb, uint8_t* rgb8, float* var);

}  // namespace fr
#endif
