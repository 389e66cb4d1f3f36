// denoise_guided_check.cpp — test harness (tests/test_denoise_guided_host.py): the feature-guided
// filter of a progressive accumulation (fr_ctx_denoise_guided) as a CPU program, built with
// -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   denoise_guided_check FILE   FILE holds u32 words: W, H, levels, the bits of k, the bits of
//                        sigma_z, normal_pow2, demodulate, then A (W*H*3 f32 bits), Q (W*H*3), n
//                        (W*H, each pixel's tile's n_t), K (W*H, K_t), G0 (W*H*4: N, t), G1
//                        (W*H*4: P, id) and the albedo (W*H*3). Prints one line per pixel in
//                        row-major order, in hex: the bits of the filtered mean r g b, the bits
//                        of var, the u8 r g b, and 1 if the pixel is valid.
// The arithmetic is the header the kernels compile (fo-rma_amd/csrc/denoise.h), so a numpy
// restatement that equals these bits restates the kernels.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../fo-rma_amd/csrc/denoise.h"

namespace {

struct Fetch {
  const fr::DnPixel* px;
  int W;
  fr::DnPixel operator()(int x, int y) const { return px[static_cast<size_t>(y) * W + x]; }
};

float as_f32(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

struct FetchFeat {
  const uint32_t *g0, *g1;
  int W;
  fr::DnFeat operator()(int x, int y) const {
    const size_t i = static_cast<size_t>(y) * W + x;
    return fr::DnFeat{fr::V3{as_f32(g0[4 * i]), as_f32(g0[4 * i + 1]), as_f32(g0[4 * i + 2])}, as_f32(g0[4 * i + 3]),
                      fr::V3{as_f32(g1[4 * i]), as_f32(g1[4 * i + 1]), as_f32(g1[4 * i + 2])}, g1[4 * i + 3]};
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: denoise_guided_check FILE\n");
    return 2;
  }
  std::vector<uint32_t> in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t buf[1024];
  size_t got;
  while ((got = fread(buf, 4, 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  if (in.size() < 7) return 2;
  const uint32_t W = in[0], H = in[1], levels = in[2], pow2 = in[5];
  const float k = as_f32(in[3]), sigma_z = as_f32(in[4]);
  const bool demod = in[6] != 0u;
  const size_t n_px = static_cast<size_t>(W) * H;
  if (!W || !H || W > 4096 || H > 4096 || levels < 1 || levels > fr::kDnLevelsMax || pow2 > fr::kDnNormalPow2Max ||
      in[6] > 1u || in.size() != 7 + n_px * 19)
    return 2;
  const uint32_t *a = in.data() + 7, *q = a + 3 * n_px, *n = q + 3 * n_px, *kt = n + n_px, *g0 = kt + n_px,
                 *g1 = g0 + 4 * n_px, *alb = g1 + 4 * n_px;
  const FetchFeat feat{g0, g1, static_cast<int>(W)};
  auto alb_at = [&](size_t i) { return fr::V3{as_f32(alb[3 * i]), as_f32(alb[3 * i + 1]), as_f32(alb[3 * i + 2])}; };
  std::vector<fr::DnPixel> ping(n_px), pong(n_px);
  for (size_t i = 0; i < n_px; ++i) {
    const fr::V3 av{as_f32(a[3 * i]), as_f32(a[3 * i + 1]), as_f32(a[3 * i + 2])};
    const fr::V3 qv{as_f32(q[3 * i]), as_f32(q[3 * i + 1]), as_f32(q[3 * i + 2])};
    ping[i] = fr::dn_prep_guided(av, qv, static_cast<float>(n[i]), static_cast<float>(kt[i] - 1u),
                                 feat(static_cast<int>(i % W), static_cast<int>(i / W)), alb_at(i), demod);
  }
  for (uint32_t l = 0; l < levels; ++l) {
    const Fetch fetch{ping.data(), static_cast<int>(W)};
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x)
        pong[static_cast<size_t>(y) * W + x] =
            fr::dn_level_guided(fetch, feat, static_cast<int>(x), static_cast<int>(y), static_cast<int>(W),
                                static_cast<int>(H), 1 << l, k, sigma_z, pow2);
    ping.swap(pong);
  }
  for (size_t i = 0; i < n_px; ++i) {
    const fr::DnPixel p = ping[i];
    const fr::V3 m = fr::dn_remodulate(p, alb_at(i), demod);
    printf("%08x %08x %08x %08x %02x %02x %02x %d\n", fr::dn_bits(m.x), fr::dn_bits(m.y), fr::dn_bits(m.z),
           fr::dn_bits(fr::dn_var(p)), fr::to_u8(m.x), fr::to_u8(m.y), fr::to_u8(m.z), fr::dn_valid(p) ? 1 : 0);
  }
  return 0;
}
