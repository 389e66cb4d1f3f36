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

}  // namespace fr
#endif
