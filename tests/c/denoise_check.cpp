// denoise_check.cpp — test harness (tests/test_denoise_host.py): the variance-guided filter of
// a progressive accumulation (fr_ctx_denoise) as a CPU program, built with
// -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   denoise_check FILE   FILE holds u32 words: W, H, levels, the bits of k, then A (W*H*3 f32
//                        bits), Q (W*H*3), n (W*H, each pixel's tile's n_t) and K (W*H, K_t).
//                        Prints one line per pixel in row-major order, in hex: the bits of the
//                        filtered mean r g b, the bits of var, the u8 r g b, and 1 if the pixel
//                        is valid.
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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: denoise_check FILE\n");
    return 2;
  }
  std::vector<uint32_t> in;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t buf[1024];
  size_t got;
  while ((got = fread(buf, 4, 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  if (in.size() < 4) return 2;
  const uint32_t W = in[0], H = in[1], levels = in[2];
  const float k = as_f32(in[3]);
  const size_t n_px = static_cast<size_t>(W) * H;
  if (!W || !H || W > 4096 || H > 4096 || levels < 1 || levels > fr::kDnLevelsMax || in.size() != 4 + n_px * 8) return 2;
  const uint32_t *a = in.data() + 4, *q = a + 3 * n_px, *n = q + 3 * n_px, *kt = n + n_px;
  std::vector<fr::DnPixel> ping(n_px), pong(n_px);
  for (size_t i = 0; i < n_px; ++i) {
    const fr::V3 av{as_f32(a[3 * i]), as_f32(a[3 * i + 1]), as_f32(a[3 * i + 2])};
    const fr::V3 qv{as_f32(q[3 * i]), as_f32(q[3 * i + 1]), as_f32(q[3 * i + 2])};
    ping[i] = fr::dn_prep(av, qv, static_cast<float>(n[i]), static_cast<float>(kt[i] - 1u));
  }
  for (uint32_t l = 0; l < levels; ++l) {
    const Fetch fetch{ping.data(), static_cast<int>(W)};
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x)
        pong[static_cast<size_t>(y) * W + x] = fr::dn_level(fetch, static_cast<int>(x), static_cast<int>(y),
                                                            static_cast<int>(W), static_cast<int>(H), 1 << l, k);
    ping.swap(pong);
  }
  for (size_t i = 0; i < n_px; ++i) {
    const fr::DnPixel p = ping[i];
    printf("%08x %08x %08x %08x %02x %02x %02x %d\n", fr::dn_bits(p.r), fr::dn_bits(p.g), fr::dn_bits(p.b),
           fr::dn_bits(fr::dn_var(p)), fr::to_u8(p.r), fr::to_u8(p.g), fr::to_u8(p.b), fr::dn_valid(p) ? 1 : 0);
  }
  return 0;
}
