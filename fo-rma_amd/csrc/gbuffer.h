// gbuffer.h — the first-hit feature buffers of a view (fr_ctx_gbuffer): per
// pixel the primary ray's closest primitive, its own accepted root t, the normal N at that
// root, the point P = o + t d and the primitive's attenuation. Its f32 arithmetic, shared by the
// kernel (gbuffer.hip) and a CPU program (tests/c/gbuffer_check.cpp), and the launch. Every
// named operation rounds once in f32; the build rules of rt_core.h hold (no contraction, IEEE
// '/' and sqrt).
//
// The primary ray of pixel (x, y) is camera.rs get_ray with the jitter fixed at 0.5 and no lens
// offset (lens_radius is ignored: the buffers are those of the pinhole view):
//   u = ((float)x + 0.5) / (float)W,  v = ((float)(H - y) + 0.5) / (float)H
//   o = position,  d = ((lower_left + u horizontal) + v vertical) - position
// The closest hit is the reference loop (tracer.rs:190-200): list order, t_min = 0.001, t_max =
// the closest root so far, strict comparisons, each kind's test in rt_core.h's plain IEEE form
// (the forms the trace kernel's fast sequences are checked against). t is the winner's own
// root, not the shared record's last written t: a plane after the winner that passes its
// denominator test and fails its bounds leaves the record's t stale, and the
// feature buffers do not carry that quirk.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/forma_rt.h"
#include "rt_core.h"

namespace fr {

constexpr uint32_t kGbMiss = 0xFFFFFFFFu;  // FR_GBUFFER_MISS: the id of a pixel whose ray hits nothing
constexpr float kGbTMin = 0.001f;

// The camera.rs fields the primary ray reads.
struct GbCam {
  V3 pos, ll, hor, ver;
};

struct GbRay {
  V3 o, d;
  // per ray: the box test's reciprocals RN(1 / d_k) clamped to +-2^100 and o_k inv_k
  // (rt_core.h slab3_box), and dot(d, d) of the sphere test
  V3 inv, oinv;
  float a;
};

FR_HD GbRay gb_primary_ray(const GbCam& c, uint32_t x, uint32_t y, uint32_t W, uint32_t H) {
  const float u = (static_cast<float>(x) + 0.5f) / static_cast<float>(W);
  const float v = (static_cast<float>(H - y) + 0.5f) / static_cast<float>(H);
  GbRay r;
  r.o = c.pos;
  r.d = sub(add(add(c.ll, scl(u, c.hor)), scl(v, c.ver)), c.pos);
  r.inv = V3{box_inv_clamp(1.0f / r.d.x), box_inv_clamp(1.0f / r.d.y), box_inv_clamp(1.0f / r.d.z)};
  r.oinv = V3{r.o.x * r.inv.x, r.o.y * r.inv.y, r.o.z * r.inv.z};
  r.a = dot(r.d, r.d);
  return r;
}

template <class F4>
FR_HD V3 gb_xyz(const F4& a) {
  return V3{a.x, a.y, a.z};
}

// One primitive of kind K against the ray in (kGbTMin, t_max): true and its accepted root.
// rec[k] is the k-th 16-byte word of the primitive's 64-byte record (pack.cpp), a value with
// members x, y, z, w.
template <uint32_t K, class Rec>
FR_HD bool gb_test(const Rec& rec, const GbRay& r, float t_max, float& t) {
  if (K == FR_AABB) {
    return slab_root(slab3_box(gb_xyz(rec[0]), gb_xyz(rec[1]), r.o, r.inv, r.oinv), kGbTMin, t_max, t);
  } else if (K == FR_SPHERE) {
    const auto g = rec[0];
    return sphere_root(gb_xyz(g), g.w, r.o, r.d, r.a, kGbTMin, t_max, t);
  } else if (K == FR_PLANE) {
    return plane_test(gb_xyz(rec[0]), gb_xyz(rec[1]), gb_xyz(rec[2]), r.o, r.d, kGbTMin, t_max, t) == 2;
  } else if (K == FR_TRIANGLE) {
    return tri_root(gb_xyz(rec[0]), gb_xyz(rec[1]), gb_xyz(rec[2]), r.o, r.d, kGbTMin, t_max, t);
  } else if (K == FR_OBB) {
    const auto a = rec[0], b = rec[1], c = rec[2], e = rec[3];
    const ObbFrame f = obb_frame(gb_xyz(a), gb_xyz(b), gb_xyz(c), gb_xyz(e), r.o, r.d);
    return slab_root(slab3(V3{-a.w, -b.w, -c.w}, V3{a.w, b.w, c.w}, f.ol, f.inv), kGbTMin, t_max, t);
  }
  return false;  // FR_STUB: never hits (aabb.rs:21-34, rectangle.rs:21-34)
}

// The winner's normal at its root t, as the hit functions write it to the record: kind is the
// record's (the bits of rec[3].w), cls its effective ScatterClass (a triangle's winding normal
// faces the ray unless it is dielectric).
template <class Rec>
FR_HD V3 gb_normal(uint32_t kind, uint32_t cls, const Rec& rec, const GbRay& r, float t) {
  if (kind == FR_AABB) return slab_normal(slab3_box(gb_xyz(rec[0]), gb_xyz(rec[1]), r.o, r.inv, r.oinv), t, r.d);
  if (kind == FR_SPHERE) {
    const auto g = rec[0];
    return divs(sub(add(r.o, scl(t, r.d)), gb_xyz(g)), g.w);
  }
  if (kind == FR_PLANE) return scl(-1.0f, gb_xyz(rec[1]));
  if (kind == FR_TRIANGLE) {
    const V3 n = gb_xyz(rec[3]);
    return (cls != SC_DIELECTRIC && dot(n, r.d) > 0.0f) ? scl(-1.0f, n) : n;
  }
  const auto a = rec[0], b = rec[1], c = rec[2], e = rec[3];
  const ObbFrame f = obb_frame(gb_xyz(a), gb_xyz(b), gb_xyz(c), gb_xyz(e), r.o, r.d);
  const Slab sl = slab3(V3{-a.w, -b.w, -c.w}, V3{a.w, b.w, c.w}, f.ol, f.inv);
  return obb_normal(gb_xyz(b), gb_xyz(c), gb_xyz(e), sl, t, f.dl);
}

// A pixel's two 16-byte words and its albedo: G0 = (N, t), G1 = (P, bits(id)), alb = (rgb, 0).
struct GbF4 {
  float x, y, z, w;
};
struct GbPixel {
  GbF4 g0, g1, alb;
};

FR_HD float gb_id_as_float(uint32_t id) {
  float f;
  memcpy(&f, &id, 4);
  return f;
}
FR_HD uint32_t gb_id(GbF4 g1) {
  uint32_t u;
  memcpy(&u, &g1.w, 4);
  return u;
}

FR_HD GbPixel gb_miss() {
  return GbPixel{GbF4{0.0f, 0.0f, 0.0f, 0.0f}, GbF4{0.0f, 0.0f, 0.0f, gb_id_as_float(kGbMiss)},
                 GbF4{1.0f, 1.0f, 1.0f, 0.0f}};
}

// att: the winner's entry of the attenuation table (colour, or 1 for the light class).
template <class Rec, class F4>
FR_HD GbPixel gb_hit(uint32_t id, uint32_t kind, uint32_t cls, const Rec& rec, const F4& att, const GbRay& r, float t) {
  const V3 n = gb_normal(kind, cls, rec, r, t);
  const V3 p = add(r.o, scl(t, r.d));
  return GbPixel{GbF4{n.x, n.y, n.z, t}, GbF4{p.x, p.y, p.z, gb_id_as_float(id)}, GbF4{att.x, att.y, att.z, 0.0f}};
}

}  // namespace fr

#if defined(__HIPCC__) || defined(__HIP__)

namespace fr {

constexpr uint32_t kGbTileW = 32, kGbTileH = 8;  // the workgroup: 32 x 8 pixels, as a denoise level's

// The scene tables the pass reads (pack.h): the records and their kind runs, in list order, the
// effective scatter classes and the attenuations.
struct GbScene {
  const float4* rec;
  const uint4* runs;
  const uint32_t* cls;
  const float4* att;
  uint32_t n_runs, n;
};

// Enqueues the pass on `stream`: one thread per pixel of the W x H image; g0, g1 and alb are
// W*H float4 each, indexed y * W + x.
hipError_t launch_gbuffer(hipStream_t stream, const GbScene& sc, const GbCam& cam, uint32_t W, uint32_t H, float4* g0,
                          float4* g1, float4* alb);

}  // namespace fr
#endif
