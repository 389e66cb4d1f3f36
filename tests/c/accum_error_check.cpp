// accum_error_check.cpp — test harness (tests/test_accum_error_host.py): the error estimate of
// progressive accumulation (FR_FLAG_ACCUM_ERROR) as a CPU program, built with
// -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   decision      walks the continue / restart decision (plan.cpp: accum_key, accum_step) with
//                 the flag on and off, and check_params' two refusals; one JSON line per step
//   terms FILE    rows of 3 x u32 {S bits, spp, Q bits}: prints the bits of S^2 / spp and of
//                 Q + S^2 / spp (accum_error.h: accum_sq_term), one row per line, in hex
//   rel FILE      rows of 8 x u32 {A r g b bits, Q r g b bits, n, K}: prints the bits of rel
//                 (accum_error.h: accum_rel_error)
// The arithmetic is the header the sum and error kernels compile, so a numpy restatement
// that equals these bits restates the kernels.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../fo-rma_amd/csrc/accum_error.h"
#include "../../fo-rma_amd/csrc/internal.h"
#include "../../fo-rma_amd/csrc/plan.h"
#include "../../include/forma_rt.h"

// A host-only build makes no device copies of a scene.
namespace fr {
void release_device_copies(fr_scene* s) { s->copies.clear(); }
}  // namespace fr

static fr::AccumState g_state;

static int frame(const char* name, uint64_t uid, const fr_camera& cam, const fr_params& p) {
  if (fr::check_params(&p) != FR_OK) return 1;
  fr::AccumStep step;
  const int rc = fr::accum_step(g_state, fr::accum_key(uid, cam, p), p.spp, &step);
  if (rc || !step.next.live) return 1;
  g_state = step.next;
  printf("{\"case\": \"%s\", \"start\": %d, \"frames\": %u, \"samples\": %u, \"has_q\": %d}\n", name, step.start ? 1 : 0,
         g_state.frames, g_state.samples, g_state.has_q ? 1 : 0);
  return 0;
}

static int decision() {
  fr_camera cam;
  if (fr_camera_init(&cam, 33, 17) != FR_OK) return 2;
  fr_params p{};
  p.width = 33, p.height = 17, p.spp = 4, p.max_depth = 8, p.seed = 1, p.strip_rows = fr::kStripRows;
  p.shard_index = 0, p.shard_count = 1;
  const uint32_t on = FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR | FR_FLAG_WRITE_U8, off = FR_FLAG_ACCUMULATE | FR_FLAG_WRITE_U8;
  int bad = 0;
  p.flags = on;
  bad |= frame("on", 7, cam, p);
  p.seed = 2, p.spp = 16;  // seed and spp are not part of the view
  bad |= frame("on_again", 7, cam, p);
  p.flags = off;
  bad |= frame("off", 7, cam, p);
  bad |= frame("off_again", 7, cam, p);
  p.flags = on;
  bad |= frame("on_after_off", 7, cam, p);
  g_state = fr::AccumState{};  // fr_ctx_accum_reset
  bad |= frame("reset", 7, cam, p);
  bad |= frame("on_again", 7, cam, p);
  p.flags = FR_FLAG_ACCUM_ERROR | FR_FLAG_WRITE_U8;
  int rc = fr::check_params(&p);  // (before fr_last_error is read)
  printf("{\"case\": \"without_accumulate\", \"rc\": %d, \"error\": \"%s\"}\n", rc, fr_last_error());
  p.flags = on, p.spp = 0;
  rc = fr::check_params(&p);
  printf("{\"case\": \"spp_zero\", \"rc\": %d, \"error\": \"%s\"}\n", rc, fr_last_error());
  p.flags = off;  // a frame without samples may still accumulate without the flag
  printf("{\"case\": \"spp_zero_plain_accumulate\", \"rc\": %d}\n", fr::check_params(&p));
  return bad;
}

static bool read_rows(const char* path, size_t words, std::vector<uint32_t>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint32_t buf[1024];
  size_t n;
  while ((n = fread(buf, 4, 1024, f)) > 0) out->insert(out->end(), buf, buf + n);
  fclose(f);
  return out->size() % words == 0;
}

static float as_f32(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint32_t as_u32(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "decision") == 0) return decision();
  std::vector<uint32_t> in;
  if (argc == 3 && strcmp(argv[1], "terms") == 0) {
    if (!read_rows(argv[2], 3, &in)) return 2;
    for (size_t i = 0; i < in.size(); i += 3) {
      const float t = fr::accum_sq_term(as_f32(in[i]), static_cast<float>(in[i + 1]));
      printf("%08x %08x\n", as_u32(t), as_u32(as_f32(in[i + 2]) + t));
    }
    return 0;
  }
  if (argc == 3 && strcmp(argv[1], "rel") == 0) {
    if (!read_rows(argv[2], 8, &in)) return 2;
    for (size_t i = 0; i < in.size(); i += 8) {
      const fr::V3 a{as_f32(in[i]), as_f32(in[i + 1]), as_f32(in[i + 2])};
      const fr::V3 q{as_f32(in[i + 3]), as_f32(in[i + 4]), as_f32(in[i + 5])};
      const float rel = fr::accum_rel_error(a, q, static_cast<float>(in[i + 6]), static_cast<float>(in[i + 7] - 1u));
      printf("%08x\n", as_u32(rel));
    }
    return 0;
  }
  fprintf(stderr, "usage: accum_error_check decision | terms FILE | rel FILE\n");
  return 2;
}
