// temporal.h — temporal reuse of a progressive accumulation across a camera move
// (fr_ctx_temporal): the accumulators of the previous view, reprojected through
// the first-hit features of both views (gbuffer.h), are added per pixel to the live accumulation
// of the current view; the sum is shown as it is or through the a-trous levels of denoise.h.
// Its f32 arithmetic, shared by the kernels (temporal.hip) and a CPU program
// (tests/c/temporal_check.cpp), and the launches. Every named operation rounds once in f32; the
// build rules of rt_core.h hold (no contraction, IEEE '/').
//
// History of a view: per image pixel y * W + x the totals (A_T[3], Q_T[3], n_T, K_T) as of the
// view's last fr_ctx_temporal call, n_T and K_T in f32, as two 16-byte words TA = (A_T, n_T) and
// TQ = (Q_T, K_T), beside the view's G-buffer words G0 = (N, t), G1 = (P, id) and its camera.
#pragma once
#include <stdint.h>
#include <string.h>

#include "denoise.h"
#include "gbuffer.h"

namespace fr {

constexpr uint32_t kTpNone = 0xFFFFFFFFu;  // FR_TP_NONE: the source of a pixel without one
// FR_TP_REASON_*: why a pixel has the prior it has
enum TpReason : uint32_t {
  kTpReused = 0,     // the source pixel's totals, scaled to the cap, are the prior
  kTpNoHistory = 1,  // the context holds no history (every pixel of such a call)
  kTpMiss = 2,       // the pixel's primary ray hits nothing
  kTpOffscreen = 3,  // P is behind the previous camera or projects outside its frame
  kTpId = 4,         // the source pixel shows another primitive (or nothing)
  kTpNormal = 5,     // dot(N, N0) < normal_min
  kTpPlane = 6,      // the source's point is too far from the pixel's tangent plane
  kTpHistory = 7,    // the source's totals are empty or not finite
};
constexpr float kTpNMaxDefault = 32.0f, kTpNMaxSpecularDefault = 4.0f;  // FR_TP_N_MAX_DEFAULT, ..._SPECULAR_DEFAULT
constexpr float kTpSigmaZDefault = 0x1p-5f, kTpNormalMinDefault = 0.9f;  // FR_TP_SIGMA_Z_DEFAULT, FR_TP_NORMAL_MIN_DEFAULT
constexpr float kTpNMaxMax = 0x1p24f;                                     // FR_TP_N_MAX_MAX

// fr_temporal's four numbers
struct TpOpt {
  float n_max, n_max_specular, sigma_z, normal_min;
};

// The previous camera as the projection reads it: e = ll - pos, nrm = cross(hor, ver),
// hh = dot(hor, hor), vv = dot(ver, ver), computed once per view by this function on the host.
struct TpCam {
  V3 pos, e, hor, ver, nrm;
  float hh, vv;
};
FR_HD TpCam tp_cam(const GbCam& c) {
  return TpCam{c.pos, sub(c.ll, c.pos), c.hor, c.ver, cross(c.hor, c.ver), dot(c.hor, c.hor), dot(c.ver, c.ver)};
}

// P of the new view into the previous camera's W x H frame: gb_primary_ray inverted, the
// reference's H - y row rule included.
//   q = P - pos, s = dot(e, nrm) / dot(q, nrm), r = s q - e
//   u = dot(r, hor) / hh, v = dot(r, ver) / vv, fx = floor(u W), fy = floor(v H)
// Valid iff s > 0, 0 <= fx < W and 1 <= fy <= H, compared on the floats (a NaN fails); the source
// pixel is then (x0, y0) = (fx, H - fy), inside the image.
FR_HD bool tp_project(const TpCam& c, V3 p, uint32_t W, uint32_t H, uint32_t& x0, uint32_t& y0) {
  const V3 q = sub(p, c.pos);
  const float s = dot(c.e, c.nrm) / dot(q, c.nrm);
  const V3 r = sub(scl(s, q), c.e);
  const float u = dot(r, c.hor) / c.hh;
  const float v = dot(r, c.ver) / c.vv;
  const float fw = static_cast<float>(W), fh = static_cast<float>(H);
  const float fx = __builtin_floorf(u * fw), fy = __builtin_floorf(v * fh);
  const bool ok = (s > 0.0f) & (fx >= 0.0f) & (fx < fw) & (fy >= 1.0f) & (fy <= fh);
  x0 = ok ? static_cast<uint32_t>(fx) : 0u;
  y0 = ok ? H - static_cast<uint32_t>(fy) : 0u;
  return ok;
}

FR_HD bool tp_finite(float x) { return (x - x) == 0.0f; }

// The source pixel (features f0, totals ta = (A_T, n_T), tq = (Q_T, K_T)) against the pixel
// (features f, a hit): kTpReused, or the first test it fails, in this order:
//   id:     f0.id == f.id
//   normal: dot(N, N0) >= normal_min
//   plane:  d = dot(N, P0 - P), z = sigma_z t, d d <= z z + kDnEps
//   totals: n_T > 0 and every A_T and Q_T channel finite
FR_HD uint32_t tp_accept(const TpOpt& o, const DnFeat& f, const DnFeat& f0, GbF4 ta, GbF4 tq) {
  if (f0.id != f.id) return kTpId;
  if (!(dot(f.n, f0.n) >= o.normal_min)) return kTpNormal;
  const float d = dot(f.n, sub(f0.p, f.p));
  const float z = o.sigma_z * f.t;
  if (!(d * d <= z * z + kDnEps)) return kTpPlane;
  const bool fin = tp_finite(ta.x) && tp_finite(ta.y) && tp_finite(ta.z) && tp_finite(tq.x) && tp_finite(tq.y) &&
                   tp_finite(tq.z);
  if (!(ta.w > 0.0f) || !fin) return kTpHistory;
  return kTpReused;
}

// The cap of a pixel whose hit primitive has effective scatter class cls (pack.h's table):
// first-hit reprojection ghosts on mirrors and glass, which take the smaller cap.
FR_HD float tp_cap(const TpOpt& o, uint32_t cls) {
  return (cls == SC_METAL || cls == SC_DIELECTRIC) ? o.n_max_specular : o.n_max;
}

// A pixel's prior: two 16-byte words PA = (A', n'), PQ = (Q', K'), its source y0 W + x0 (or
// kTpNone) and its reason.
struct TpPrior {
  GbF4 a, q;
  uint32_t source, reason;
};
FR_HD TpPrior tp_no_prior(uint32_t reason) {
  return TpPrior{GbF4{0.0f, 0.0f, 0.0f, 0.0f}, GbF4{0.0f, 0.0f, 0.0f, 0.0f}, kTpNone, reason};
}

// An accepted source scaled to the cap: f = n_T > cap ? cap / n_T : 1, A' = A_T f, Q' = Q_T f,
// n' = n_T f, K' = 1 + (K_T - 1) f. Scaling A, Q and n by f scales the scatter Q - A A / n by f,
// and scaling K - 1 by f keeps the per-sample variance estimate. f = 0 (a cap of 0, or one that
// underflows against n_T) is no reuse: the prior is all zeros, K' included; the source and the
// reason stay, they say where the history lies.
FR_HD TpPrior tp_scale(float cap, GbF4 ta, GbF4 tq, uint32_t source) {
  const float f = ta.w > cap ? cap / ta.w : 1.0f;
  TpPrior p = tp_no_prior(kTpReused);
  p.source = source;
  if (!(f > 0.0f)) return p;
  p.a = GbF4{ta.x * f, ta.y * f, ta.z * f, ta.w * f};
  p.q = GbF4{tq.x * f, tq.y * f, tq.z * f, 1.0f + (tq.w - 1.0f) * f};
  return p;
}

// Reprojection of one pixel with features f (cls: its primitive's class, read only for a hit).
// hist(j, f0, ta, tq) loads the previous view's pixel j.
template <class Hist>
FR_HD TpPrior tp_reproject(const TpCam& c, const TpOpt& o, const DnFeat& f, uint32_t cls, uint32_t W, uint32_t H,
                           const Hist& hist) {
  if (f.id == kGbMiss) return tp_no_prior(kTpMiss);
  uint32_t x0, y0;
  if (!tp_project(c, f.p, W, H, x0, y0)) return tp_no_prior(kTpOffscreen);
  const uint32_t j = y0 * W + x0;
  DnFeat f0;
  GbF4 ta, tq;
  hist(j, f0, ta, tq);
  const uint32_t why = tp_accept(o, f, f0, ta, tq);
  if (why != kTpReused) {
    TpPrior p = tp_no_prior(why);
    p.source = j;
    return p;
  }
  return tp_scale(tp_cap(o, cls), ta, tq, j);
}

// The totals of a pixel: the live accumulation's A, Q and counts plus the prior.
//   A_T = A + A', Q_T = Q + Q', n_T = (float)n + n', K_T = (float)K + K'
struct TpTotals {
  GbF4 a, q;
};
FR_HD TpTotals tp_totals(V3 a, V3 q, uint32_t n, uint32_t frames, GbF4 pa, GbF4 pq) {
  return TpTotals{GbF4{a.x + pa.x, a.y + pa.y, a.z + pa.z, static_cast<float>(n) + pa.w},
                  GbF4{q.x + pq.x, q.y + pq.y, q.z + pq.z, static_cast<float>(frames) + pq.w}};
}

// dn_prep_guided's feature test (a miss has none).
FR_HD bool tp_feat_ok(const DnFeat& f) {
  const bool ok = (f.t <= kDnFeatMax) & (__builtin_fabsf(f.p.x) <= kDnFeatMax) & (__builtin_fabsf(f.p.y) <= kDnFeatMax) &
                  (__builtin_fabsf(f.p.z) <= kDnFeatMax) & (__builtin_fabsf(f.n.x) <= kDnNormalMax) &
                  (__builtin_fabsf(f.n.y) <= kDnNormalMax) & (__builtin_fabsf(f.n.z) <= kDnNormalMax);
  return (f.id == kDnMiss) | ok;
}

// The filter's pixel of the totals. K_T >= 2: dn_prep (guided: dn_prep_guided) of
// (A_T, Q_T, n_T, K_T - 1). K_T < 2 is a first frame without accepted history, which has no
// variance: with m_c = A_T_c / n_T, C_c = m_c (m_c / a_c with demodulate, a = dn_alb),
//   g = max((C_r + C_g) + C_b, kErrFloor), var = (g g) / n_T
// a relative standard error of 1 on accum_rel_error's denominator. A miss is the exception: the
// sky is a function of the direction alone, its only noise is the jitter inside the pixel, and
// a relative error of 1 there lets the unguided levels blur the sky into the objects (DESIGN.md
// §5): a miss without history takes var = 0, so no tap moves it far and it stays a tap of its
// neighbours at their own scale. Valid iff |m_c| <= kDnMeanMax
// in every channel and var <= kDnVarMax (and, guided, tp_feat_ok): the caps of dn_prep.
FR_HD DnPixel tp_first_frame(const TpTotals& t, bool guided, const DnFeat& f, V3 alb, bool demodulate, bool miss) {
  const float fn = t.a.w;
  const float mr = t.a.x / fn, mg = t.a.y / fn, mb = t.a.z / fn;
  DnPixel p{mr, mg, mb, 0.0f};
  if (guided && demodulate) {
    const V3 al = dn_alb(alb, true);
    p.r = mr / al.x;
    p.g = mg / al.y;
    p.b = mb / al.z;
  }
  const float g = fmax_num((p.r + p.g) + p.b, kErrFloor);
  const float var = miss ? 0.0f : (g * g) / fn;
  bool ok = (__builtin_fabsf(mr) <= kDnMeanMax) & (__builtin_fabsf(mg) <= kDnMeanMax) &
            (__builtin_fabsf(mb) <= kDnMeanMax) & (var <= kDnVarMax);
  if (guided) ok = ok & tp_feat_ok(f);
  p.var = ok ? var : dn_float(dn_bits(var) | kDnInvalidBit);
  return p;
}
FR_HD DnPixel tp_prep(const TpTotals& t, bool miss) {  // miss: the pixel's id is kGbMiss
  if (t.q.w < 2.0f) return tp_first_frame(t, false, DnFeat{}, V3{1.0f, 1.0f, 1.0f}, false, miss);
  return dn_prep(V3{t.a.x, t.a.y, t.a.z}, V3{t.q.x, t.q.y, t.q.z}, t.a.w, t.q.w - 1.0f);
}
FR_HD DnPixel tp_prep_guided(const TpTotals& t, const DnFeat& f, V3 alb, bool demodulate) {
  if (t.q.w < 2.0f) return tp_first_frame(t, true, f, alb, demodulate, f.id == kGbMiss);
  return dn_prep_guided(V3{t.a.x, t.a.y, t.a.z}, V3{t.q.x, t.q.y, t.q.z}, t.a.w, t.q.w - 1.0f, f, alb, demodulate);
}

}  // namespace fr

#if defined(__HIPCC__) || defined(__HIP__)
#include "kparams.h"

namespace fr {

// The reprojection, once per new accumulation: one thread per pixel of the W x H image. g0, g1:
// the new view's G-buffer; cls: the scene's effective scatter classes, n_prims of them; h_g0,
// h_g1, h_ta, h_tq: the previous view's G-buffer words and totals. Writes the prior's two words,
// the source map and the reason codes, W*H each.
hipError_t launch_temporal_reproject(hipStream_t stream, const TpCam& cam, const TpOpt& opt, uint32_t W, uint32_t H,
                                     const float4* g0, const float4* g1, const uint32_t* cls, uint32_t n_prims,
                                     const float4* h_g0, const float4* h_g1, const float4* h_ta, const float4* h_tq,
                                     float4* prior_a, float4* prior_q, uint32_t* source, uint32_t* reason);

// Totals and prep, every call: one thread per pixel slot of kp's shard (the whole image), the
// counts as launch_denoise reads them. Writes TA and TQ (W*H float4 each, by image pixel) and
// the filter's pixel into ping. g1: the view's G-buffer word with the id, always read. g0 and alb
// null: unguided (tp_prep); else tp_prep_guided.
hipError_t launch_temporal_prep(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                                const uint32_t* n_t, const uint32_t* k_t, uint32_t n, uint32_t frames,
                                const float4* prior_a, const float4* prior_q, float4* ta, float4* tq, const float4* g0,
                                const float4* g1, const float4* alb, uint32_t demodulate, DnPixel* ping);

// levels = 0: the mean (remodulated when alb is not null and demodulate is set), the u8 image and
// the variance straight from prep's pixels.
hipError_t launch_temporal_finalise(hipStream_t stream, uint32_t W, uint32_t H, const DnPixel* ping, const float4* alb,
                                    uint32_t demodulate, float* mean_rgb, uint8_t* rgb8, float* var);

}  // namespace fr
#endif
