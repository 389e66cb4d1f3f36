// temporal_check.cpp — test harness (tests/test_temporal_host.py): temporal reuse of a progressive
// accumulation (fr_ctx_temporal) as a CPU program, built with -fsanitize=address,undefined
// -fno-sanitize-recover=all -ffp-contract=off and linked with plan.cpp.
//   temporal_check view FILE   One call for one view. FILE holds u32 words: W, H, levels, the bits
//                        of k, guided (0 or 1), the bits of the guide's sigma_z, normal_pow2,
//                        demodulate, the bits of n_max, n_max_specular, sigma_z and normal_min,
//                        has_history (0: an empty prior; 1: reproject) and n_prims; then the scene's
//                        classes (n_prims), the previous camera (12 f32 bits: position, lower_left,
//                        horizontal, vertical), A (W*H*3 f32 bits), Q (W*H*3), n (W*H, each pixel's
//                        tile's n_t), K (W*H), G0 (W*H*4: N, t), G1 (W*H*4: P, id), the albedo
//                        (W*H*3) and, with has_history, the previous view's G0, G1, TA (W*H*4:
//                        A_T, n_T) and TQ (W*H*4: Q_T, K_T). Prints one line per pixel in row-major
//                        order, in hex: PA (4 words), PQ (4), TA (4), TQ (4), the source, the
//                        reason, the bits of the mean r g b, the bits of var, the u8 r g b, and 1
//                        if the pixel is valid.
//   temporal_check step CALL...   temporal_step over a sequence of calls on one state. A CALL is
//                        gen:scene_uid:width:height:max_depth, or "reset"
//                        (fr_ctx_temporal_reset). Prints one line per call: the action and the
//                        read and write buffers.
// The arithmetic is the header the kernels compile (fo-rma_amd/csrc/temporal.h), so a numpy
// restatement that equals these bits restates the kernels.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../fo-rma_amd/csrc/plan.h"
#include "../../fo-rma_amd/csrc/internal.h"
#include "../../fo-rma_amd/csrc/temporal.h"

// A host-only build makes no device copies of a scene.
namespace fr {
void release_device_copies(fr_scene* s) { s->copies.clear(); }
}  // namespace fr

namespace {

float as_f32(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

fr::V3 v3_at(const uint32_t* w) { return fr::V3{as_f32(w[0]), as_f32(w[1]), as_f32(w[2])}; }
fr::GbF4 f4_at(const uint32_t* w) { return fr::GbF4{as_f32(w[0]), as_f32(w[1]), as_f32(w[2]), as_f32(w[3])}; }

struct Fetch {
  const fr::DnPixel* px;
  int W;
  fr::DnPixel operator()(int x, int y) const { return px[static_cast<size_t>(y) * W + x]; }
};

struct FetchFeat {
  const uint32_t *g0, *g1;
  int W;
  fr::DnFeat at(size_t i) const {
    return fr::DnFeat{v3_at(g0 + 4 * i), as_f32(g0[4 * i + 3]), v3_at(g1 + 4 * i), g1[4 * i + 3]};
  }
  fr::DnFeat operator()(int x, int y) const { return at(static_cast<size_t>(y) * W + x); }
};

struct Hist {
  FetchFeat feat;
  const uint32_t *ta, *tq;
  size_t n_px;
  void operator()(uint32_t j, fr::DnFeat& f0, fr::GbF4& a, fr::GbF4& q) const {
    if (j >= n_px) abort();  // tp_project's range
    f0 = feat.at(j);
    a = f4_at(ta + 4 * j);
    q = f4_at(tq + 4 * j);
  }
};

void print_f4(fr::GbF4 v) { printf("%08x %08x %08x %08x ", fr::dn_bits(v.x), fr::dn_bits(v.y), fr::dn_bits(v.z), fr::dn_bits(v.w)); }

int run_steps(int argc, char** argv) {
  fr::TemporalState st;
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "reset")) {
      st = fr::TemporalState{};
      printf("reset\n");
      continue;
    }
    unsigned long long gen, uid;
    unsigned w, h, d;
    if (sscanf(argv[i], "%llu:%llu:%u:%u:%u", &gen, &uid, &w, &h, &d) != 5) return 2;
    const fr::TemporalStep s = fr::temporal_step(st, gen, fr::TemporalKey{uid, w, h, d});
    const char* name = s.action == fr::TemporalAction::kKeep        ? "keep"
                       : s.action == fr::TemporalAction::kReproject ? "reproject"
                                                                    : "empty";
    printf("%s %u %u\n", name, s.read, s.write);
    st = s.next;
  }
  return 0;
}

int run_view(const char* path) {
  std::vector<uint32_t> in;
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t buf[1024];
  size_t got;
  while ((got = fread(buf, 4, 1024, f)) > 0) in.insert(in.end(), buf, buf + got);
  fclose(f);
  constexpr size_t kHead = 14;
  if (in.size() < kHead) return 2;
  const uint32_t W = in[0], H = in[1], levels = in[2], guided = in[4], pow2 = in[6], demod_w = in[7];
  const float k = as_f32(in[3]), g_sigma_z = as_f32(in[5]);
  const fr::TpOpt opt{as_f32(in[8]), as_f32(in[9]), as_f32(in[10]), as_f32(in[11])};
  const uint32_t has_hist = in[12], n_prims = in[13];
  const size_t n_px = static_cast<size_t>(W) * H;
  if (!W || !H || W > 4096 || H > 4096 || levels > fr::kDnLevelsMax || pow2 > fr::kDnNormalPow2Max || guided > 1u ||
      demod_w > 1u || has_hist > 1u || n_prims > (1u << 20) ||
      in.size() != kHead + n_prims + 12 + n_px * (19 + (has_hist ? 16 : 0)))
    return 2;
  const bool demod = demod_w != 0u;
  const uint32_t *cls = in.data() + kHead, *cam = cls + n_prims, *a = cam + 12, *q = a + 3 * n_px, *n = q + 3 * n_px,
                 *kt = n + n_px, *g0 = kt + n_px, *g1 = g0 + 4 * n_px, *alb = g1 + 4 * n_px;
  const uint32_t* h_g0 = has_hist ? alb + 3 * n_px : nullptr;
  const uint32_t *h_g1 = has_hist ? h_g0 + 4 * n_px : nullptr, *h_ta = has_hist ? h_g0 + 8 * n_px : nullptr,
                 *h_tq = has_hist ? h_g0 + 12 * n_px : nullptr;
  const FetchFeat feat{g0, g1, static_cast<int>(W)};
  const fr::TpCam pc = fr::tp_cam(fr::GbCam{v3_at(cam), v3_at(cam + 3), v3_at(cam + 6), v3_at(cam + 9)});
  const Hist hist{FetchFeat{h_g0, h_g1, static_cast<int>(W)}, h_ta, h_tq, n_px};
  std::vector<fr::TpPrior> prior(n_px);
  std::vector<fr::TpTotals> tot(n_px);
  std::vector<fr::DnPixel> ping(n_px), pong(n_px);
  for (size_t i = 0; i < n_px; ++i) {
    const fr::DnFeat fi = feat.at(i);
    if (has_hist) {
      const uint32_t c = fi.id < n_prims ? cls[fi.id] : static_cast<uint32_t>(fr::SC_NONE);
      prior[i] = fr::tp_reproject(pc, opt, fi, c, W, H, hist);
    } else {
      prior[i] = fr::tp_no_prior(fr::kTpNoHistory);
    }
    tot[i] = fr::tp_totals(v3_at(a + 3 * i), v3_at(q + 3 * i), n[i], kt[i], prior[i].a, prior[i].q);
    ping[i] = guided ? fr::tp_prep_guided(tot[i], fi, v3_at(alb + 3 * i), demod) : fr::tp_prep(tot[i], fi.id == fr::kGbMiss);
  }
  for (uint32_t l = 0; l < levels; ++l) {
    const Fetch fetch{ping.data(), static_cast<int>(W)};
    for (uint32_t y = 0; y < H; ++y)
      for (uint32_t x = 0; x < W; ++x)
        pong[static_cast<size_t>(y) * W + x] =
            guided ? fr::dn_level_guided(fetch, feat, static_cast<int>(x), static_cast<int>(y), static_cast<int>(W),
                                         static_cast<int>(H), 1 << l, k, g_sigma_z, pow2)
                   : fr::dn_level(fetch, static_cast<int>(x), static_cast<int>(y), static_cast<int>(W),
                                  static_cast<int>(H), 1 << l, k);
    ping.swap(pong);
  }
  for (size_t i = 0; i < n_px; ++i) {
    const fr::DnPixel p = ping[i];
    const fr::V3 m = guided ? fr::dn_remodulate(p, v3_at(alb + 3 * i), demod) : fr::V3{p.r, p.g, p.b};
    print_f4(prior[i].a);
    print_f4(prior[i].q);
    print_f4(tot[i].a);
    print_f4(tot[i].q);
    printf("%08x %08x %08x %08x %08x %08x %02x %02x %02x %d\n", prior[i].source, prior[i].reason, fr::dn_bits(m.x),
           fr::dn_bits(m.y), fr::dn_bits(m.z), fr::dn_bits(fr::dn_var(p)), fr::to_u8(m.x), fr::to_u8(m.y), fr::to_u8(m.z),
           fr::dn_valid(p) ? 1 : 0);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "step")) return run_steps(argc, argv);
  if (argc == 3 && !strcmp(argv[1], "view")) return run_view(argv[2]);
  fprintf(stderr, "usage: temporal_check view FILE | temporal_check step CALL...\n");
  return 2;
}
