// gbuffer_check.cpp — test harness (tests/test_gbuffer_host.py): the first-hit feature buffers
// (fr_ctx_gbuffer) as a CPU program, built with -fsanitize=address,undefined
// -fno-sanitize-recover=all -ffp-contract=off together with the host's scene packer
// (fo-rma_amd/csrc/pack.cpp, bvh.cpp).
//   gbuffer_check FILE   FILE holds u32 words: W, H, n, the bits of the camera's position,
//                        lower_left, horizontal and vertical (12 words), then n fr_prim (22 words
//                        each). Prints one line per pixel in row-major order, in hex: the id,
//                        the bits of t, of N, of P and of the albedo (11 words).
// The arithmetic is the header the kernel compiles (fo-rma_amd/csrc/gbuffer.h) over the records
// the library packs, so a restatement that equals these bits restates the kernel.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../fo-rma_amd/csrc/gbuffer.h"
#include "../../fo-rma_amd/csrc/pack.h"

namespace {

struct Rec {
  const float* w;  // 16 words
  fr::GbF4 operator[](int k) const { return fr::GbF4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]}; }
};

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

template <uint32_t K>
void test_one(const Rec& rec, const fr::GbRay& r, uint32_t i, float& closest, int& best) {
  float t = 0.0f;
  if (fr::gb_test<K>(rec, r, closest, t)) {
    closest = t;
    best = static_cast<int>(i);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: gbuffer_check FILE\n");
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
  if (in.size() < 15) return 2;
  const uint32_t W = in[0], H = in[1], n = in[2];
  if (!W || !H || W > 4096 || H > 4096 || in.size() != 15 + static_cast<size_t>(n) * 22) return 2;
  fr::GbCam cam;
  float c[12];
  for (int k = 0; k < 12; ++k) c[k] = as_f32(in[3 + k]);
  cam.pos = fr::V3{c[0], c[1], c[2]};
  cam.ll = fr::V3{c[3], c[4], c[5]};
  cam.hor = fr::V3{c[6], c[7], c[8]};
  cam.ver = fr::V3{c[9], c[10], c[11]};
  std::vector<fr_prim> prims(n);
  if (n) memcpy(prims.data(), in.data() + 15, static_cast<size_t>(n) * 88);
  const fr::PackedScene ps = fr::pack_scene(prims, false);
  const unsigned char* blob = ps.bytes.data();
  const float* recs = reinterpret_cast<const float*>(blob + ps.off_rec);
  const uint32_t* cls = reinterpret_cast<const uint32_t*>(blob + ps.off_cls);
  const float* att = reinterpret_cast<const float*>(blob + ps.off_att);
  const uint32_t* runs = reinterpret_cast<const uint32_t*>(blob + ps.off_runs);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const fr::GbRay r = fr::gb_primary_ray(cam, x, y, W, H);
      float closest = 3.40282347e+38f;
      int best = -1;
      // the kernel's walk: the list in order, as its kind runs
      for (uint32_t rr = 0; rr < ps.n_runs; ++rr) {
        const uint32_t k = runs[4 * rr], i0 = runs[4 * rr + 1], i1 = runs[4 * rr + 2];
        for (uint32_t i = i0; i < i1; ++i) {
          const Rec rec{recs + 16 * static_cast<size_t>(i)};
          if (k == FR_AABB) test_one<FR_AABB>(rec, r, i, closest, best);
          else if (k == FR_SPHERE) test_one<FR_SPHERE>(rec, r, i, closest, best);
          else if (k == FR_PLANE) test_one<FR_PLANE>(rec, r, i, closest, best);
          else if (k == FR_TRIANGLE) test_one<FR_TRIANGLE>(rec, r, i, closest, best);
          else if (k == FR_OBB) test_one<FR_OBB>(rec, r, i, closest, best);
        }
      }
      fr::GbPixel p = fr::gb_miss();
      if (best >= 0) {
        const Rec rec{recs + 16 * static_cast<size_t>(best)};
        const float* a = att + 4 * static_cast<size_t>(best);
        p = fr::gb_hit(static_cast<uint32_t>(best), bits(rec.w[15]), cls[best], rec, fr::GbF4{a[0], a[1], a[2], a[3]}, r,
                       closest);
      }
      printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", fr::gb_id(p.g1), bits(p.g0.w), bits(p.g0.x),
             bits(p.g0.y), bits(p.g0.z), bits(p.g1.x), bits(p.g1.y), bits(p.g1.z), bits(p.alb.x), bits(p.alb.y),
             bits(p.alb.z));
    }
  return 0;
}
