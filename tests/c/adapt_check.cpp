// adapt_check.cpp — test harness (tests/test_adaptive_host.py): the plan of an adaptive frame
// (FR_FLAG_ADAPTIVE) and the tiled bookkeeping beside AccumState (fo-rma_amd/csrc/plan.cpp) as a
// CPU program, built like tests/c/plan_check.cpp, printing what they decide.
//
//   adapt_check plan TILES W H SPP    the adaptive frame's plan for an active list of TILES tiles
//                                     (the headline scene's facts, 256 CUs), and the plain plan
//   adapt_check decision              a walk through continue / FR_EARG / empty list / totals
// One JSON line per case on stdout.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/forma_rt.h"
#include "../../fo-rma_amd/csrc/internal.h"
#include "../../fo-rma_amd/csrc/plan.h"

namespace fr {
void release_device_copies(fr_scene* s) { s->copies.clear(); }
}  // namespace fr

static fr_params params(uint32_t w, uint32_t h, uint32_t spp, uint32_t flags) {
  fr_params p{};
  p.width = w, p.height = h, p.spp = spp, p.max_depth = 8, p.seed = 1, p.flags = flags;
  p.strip_rows = fr::kStripRows, p.shard_count = 1;
  return p;
}

static void print_plan(const char* name, const fr::FramePlan& fp) {
  const fr::KParams& kp = fp.kp;
  uint32_t m, s;
  fr::fastdiv_magic(kp.n_tiles, m, s);
  printf("{\"plan\": \"%s\", \"rc\": 0, \"n_tiles\": %u, \"P\": %u, \"ks\": %u, \"flags\": %u, \"nblocks\": %u, "
         "\"per_block\": %zu, \"slot_bytes\": %zu, \"running_bytes\": %zu, \"passes\": %d, \"nfs\": %d, "
         "\"magic_ok\": %d, \"tiles_per_row\": %u, \"list\": %d, \"kernel\": \"%s\", \"pass\": [",
         name, kp.n_tiles, kp.P, kp.ks, kp.flags, fp.nblocks, fp.per_block, fp.slot_bytes, fp.running_bytes, fp.passes,
         fp.nfs, m == kp.tiles_magic && s == kp.tiles_shift, kp.tiles_per_row, kp.tile_list != nullptr,
         fr::kernel_id(fp.sel).name.c_str());
  for (int pass = 0; pass < fp.passes; ++pass) {
    const fr::PassPlan pp = fr::pass_plan(fp, pass);
    printf("%s[%u, %u, %u, %u, %u]", pass ? ", " : "", pp.b0, pp.nb, pp.n_items, pp.n_coarse, pp.b_fine);
  }
  printf("]}\n");
}

static int do_plan(uint32_t tiles, uint32_t w, uint32_t h, uint32_t spp) {
  fr::SceneFacts sf;
  sf.n = 6, sf.kinds = 1u << FR_AABB, sf.diffuse = true;
  const uint32_t acc = FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR;
  for (int adaptive = 0; adaptive < 2; ++adaptive) {
    const fr_params p = params(w, h, spp, FR_FLAG_WRITE_U8 | acc | (adaptive ? FR_FLAG_ADAPTIVE : 0u));
    int rc = fr::check_params(&p);
    fr::FramePlan fp;
    if (!rc)
      rc = fr::make_plan(p, 5.0f, sf, 256, size_t(256) << 30, fr::read_plan_env(), false, fr::PlanHistory{}, &fp,
                         adaptive ? &tiles : nullptr);
    if (rc) {
      printf("{\"plan\": \"%s\", \"rc\": %d, \"error\": \"%s\"}\n", adaptive ? "adaptive" : "plain", rc, fr_last_error());
      continue;
    }
    print_plan(adaptive ? "adaptive" : "plain", fp);
  }
  return 0;
}

static void step(const char* name, fr::AccumState& st, fr::TiledState& tiled, const fr::AccumKey& key, uint32_t spp,
                 bool adaptive) {
  fr::AdaptiveFrame af = fr::AdaptiveFrame::kTrace;
  int rc = adaptive ? fr::adaptive_step(st, tiled, key, &af) : FR_OK;
  fr::AccumStep s;
  const bool empty = !rc && af == fr::AdaptiveFrame::kEmpty;
  if (!rc && !empty) rc = fr::accum_step(st, key, spp, &s);
  if (rc) {
    printf("{\"case\": \"%s\", \"rc\": %d, \"error\": \"%s\", \"frames\": %u, \"samples\": %u}\n", name, rc,
           fr_last_error(), st.live ? st.frames : 0u, st.live ? st.samples : 0u);
    return;
  }
  if (!empty) {
    st = s.next;
    if (s.start) tiled = fr::TiledState{};
  }
  printf("{\"case\": \"%s\", \"rc\": 0, \"empty\": %d, \"start\": %d, \"frames\": %u, \"samples\": %u, \"tiled\": %d}\n",
         name, empty, !empty && s.start, st.frames, st.samples, tiled.tiled);
}

static int do_decision() {
  const uint32_t flags = FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR;
  fr_camera cam{};
  cam.position[0] = 1.0f;
  const fr::AccumKey key = fr::accum_key(7, cam, params(33, 17, 16, flags));
  fr_camera moved = cam;
  moved.position[0] = 2.0f;
  const fr::AccumKey key2 = fr::accum_key(7, moved, params(33, 17, 16, flags));
  fr::AccumState st;
  fr::TiledState tiled;
  step("adaptive_first", st, tiled, key, 16, true);        // would start a new accumulation
  step("plain_1", st, tiled, key, 16, false);
  step("plain_2", st, tiled, key, 16, false);
  step("adaptive_untiled", st, tiled, key, 16, true);      // no fr_ctx_adapt yet
  tiled = fr::TiledState{true, 15, 7, 400};                // fr_ctx_adapt: 7 of 15 tiles
  step("adaptive_7", st, tiled, key, 16, true);
  step("plain_in_tiled", st, tiled, key, 4, false);        // every tile advances; the totals too
  tiled.active_tiles = 0, tiled.active_pixels = 0;         // fr_ctx_adapt: nothing left
  step("adaptive_empty", st, tiled, key, 16, true);        // nothing moves
  step("adaptive_moved", st, tiled, key2, 16, true);       // the camera moved: FR_EARG, state as it was
  step("plain_moved", st, tiled, key2, 16, false);         // a new, uniform accumulation
  step("adaptive_after_restart", st, tiled, key2, 16, true);
  st.samples = 0xFFFFFFF0u;                                 // the 32-bit check reads the total
  tiled = fr::TiledState{true, 15, 1, 64};
  step("adaptive_overflow", st, tiled, key2, 16, true);
  for (uint32_t f : {FR_FLAG_ADAPTIVE, FR_FLAG_ADAPTIVE | FR_FLAG_ACCUMULATE, FR_FLAG_ADAPTIVE | flags}) {
    const fr_params p = params(33, 17, 16, f);
    const int rc = fr::check_params(&p);
    printf("{\"case\": \"flags_%u\", \"rc\": %d, \"error\": \"%s\"}\n", f, rc, rc ? fr_last_error() : "");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && strcmp(argv[1], "plan") == 0)
    return do_plan(static_cast<uint32_t>(atoi(argv[2])), static_cast<uint32_t>(atoi(argv[3])),
                   static_cast<uint32_t>(atoi(argv[4])), static_cast<uint32_t>(atoi(argv[5])));
  if (argc == 2 && strcmp(argv[1], "decision") == 0) return do_decision();
  fprintf(stderr, "usage: %s plan TILES W H SPP | decision\n", argv[0]);
  return 2;
}
